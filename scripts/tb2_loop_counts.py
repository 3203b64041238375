"""Instruction counts of a fused kernel's main loop from its gfx950 assembly (CPU only).

Compiles sq_phi4.hip to assembly with the flags of stochquant_amd/build.py (or
reads --asm), takes the kernel instance whose demangled template arguments are
--inst, finds its main loop -- the longest span closed by a backward branch --
and prints, per plane iteration (the span covers --unroll of them), the VALU
instructions by mnemonic group and the scalar and memory counts.

    python scripts/tb2_loop_counts.py [--asm file.s] [--inst 1,0,1,0,1,0] [--kernel phi4_tb2_kernel]
"""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def assembly(src):
    sys.path.insert(0, ROOT)
    from stochquant_amd.build import COMMON, HIPCC, ARCH
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "k.s")
        subprocess.run([HIPCC] + COMMON + [f"--offload-arch={ARCH}", "-x", "hip", "--cuda-device-only", "-S", src,
                                           "-o", out], check=True)
        return open(out).read()


def mangled(kernel, inst):
    args = "".join(f"L{'b' if i != 2 else 'i'}{v}E" for i, v in enumerate(inst))
    return f"{len(kernel)}{kernel}I{args}E"


def body(text, tag):
    lines = text.splitlines()
    start = next(i for i, l in enumerate(lines) if l.startswith("_Z") and tag in l.split(":")[0] and ":" in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    return lines[start:end + 1]


def main_loop(lines):
    """The instructions of the outermost loop with the most of them, by the
    compiler's own block annotations ("in Loop: Header=BBn_m", "Parent Loop",
    "This Loop Header"), so blocks laid out away from the loop still count."""
    loops, cur = collections.defaultdict(list), None
    for i, l in enumerate(lines):
        m = re.match(r"^(?:\.(LBB\d+_\d+):|; %bb\.\d+:)\s*(;.*)?$", l)
        if m:
            note = m.group(2) or ""
            j = i + 1
            while j < len(lines) and lines[j].startswith(" ") and lines[j].strip().startswith(";"):
                note += lines[j]  # the annotation's continuation lines
                j += 1
            o = re.search(r"(?:Header=|Parent Loop )(BB\d+_\d+)", note)
            cur = o.group(1) if o else (m.group(1) if "Loop Header" in note else None)
        elif cur and l.startswith("\t") and not l.strip().startswith((".", ";")):
            loops[cur].append(l)
    return max(loops.values(), key=len) if loops else []


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--asm")
    ap.add_argument("--kernel", default="phi4_tb2_kernel")
    ap.add_argument("--inst", default="1,0,1,0,1,0")
    ap.add_argument("--unroll", type=int, default=3)
    a = ap.parse_args()
    text = open(a.asm).read() if a.asm else assembly(os.path.join(ROOT, "stochquant_amd", "csrc", "sq_phi4.hip"))
    loop = main_loop(body(text, mangled(a.kernel, [int(v) for v in a.inst.split(",")])))
    ops = [l.split()[0] for l in loop if l.startswith("\t") and not l.strip().startswith((".", ";"))]
    c = collections.Counter(ops)
    valu = {k: v for k, v in c.items() if k.startswith("v_")}
    u = a.unroll
    print(f"{a.kernel}<{a.inst}> main loop: {len(ops)} instructions over {u} plane iterations")
    print(f"per plane iteration: VALU {sum(valu.values()) / u:.1f}  SALU/branch "
          f"{sum(v for k, v in c.items() if k.startswith('s_')) / u:.1f}  "
          f"VMEM {sum(v for k, v in c.items() if k.startswith('buffer_')) / u:.1f}  "
          f"LDS {sum(v for k, v in c.items() if k.startswith('ds_')) / u:.1f}")
    for k in ("v_mad_u64_u32", "v_bitop3_b32", "v_readfirstlane_b32", "v_xor_b32_e32", "v_add_u32_e32"):
        print(f"  {k:22s} {c.get(k, 0) / u:.1f}")
    print("  scalar: " + " ".join(f"{k}={v / u:.1f}" for k, v in sorted(c.items())
                                  if k.startswith(("s_mul", "s_xor", "s_add", "s_cmp", "s_cselect", "s_cbranch"))))


if __name__ == "__main__":
    main()
