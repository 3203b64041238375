"""In-tree build of libstochquant.so and tauhost.o for gfx950 (hipcc, no cmake).

    python -m stochquant_amd.build            # build if sources changed
    python -m stochquant_amd.build --force

Outputs (git-ignored, shipped to the GPU box with the working tree):
    stochquant_amd/lib/libstochquant.so
    stochquant_amd/bin/tauhost.o          (also linked as ./tauhost.o at the repo root,
                                           where taumain.py expects it)
"""
import argparse
import concurrent.futures as cf
import hashlib
import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
OBJ = os.path.join(PKG, "_obj")
LIBDIR = os.path.join(PKG, "lib")
BINDIR = os.path.join(PKG, "bin")
LIB = os.path.join(LIBDIR, "libstochquant.so")
TAUHOST = os.path.join(BINDIR, "tauhost.o")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIPCC = os.path.join(ROCM, "bin", "hipcc")
ARCH = os.environ.get("SQ_OFFLOAD_ARCH", "gfx950")

DEVICE_SOURCES = ["sq_phi4.hip", "sq_phi4_run.hip", "sq_qm1d.hip", "sq_qm1d_ens.hip", "sq_qm1d_gs.hip", "sq_phi4_ens.hip",
                  "sq_phi4_ens_flow.hip", "sq_phi4_ens_flow_frames.hip", "sq_phi4_ens_mala.hip", "sq_phi4_ens_hmc.hip", "sq_phi4_ens_exchange.hip", "sq_phi4_ens_cluster.hip",
                  "sq_phi4_ens_cluster_improved.hip", "sq_phi4_ens_digest.hip", "sq_selftest.hip", "sq_p2p.hip", "sq_fields.hip"]
HOST_SOURCES = ["sq_core.cpp", "sq_comm.cpp", "sq_phi4_create.cpp", "sq_phi4_plan.cpp", "sq_phi4_steps.cpp",
                "sq_phi4_frames.cpp", "sq_phi4_fields.cpp", "sq_qm1d_host.cpp", "sq_ens.cpp", "sq_phi4_ens.cpp",
                "sq_phi4_ens_frames.cpp", "sq_phi4_ens_corr.cpp", "sq_phi4_ens_flow.cpp", "sq_phi4_ens_samplers.cpp",
                "sq_phi4_ens_ckpt_format.cpp", "sq_phi4_ens_ckpt.cpp", "sq_diag.cpp", "sq_io.cpp"]
HEADERS = ["sq_internal.h", "sq_ctx.h", "sq_buf.h", "sq_phi4_ens_host.h", "sq_rng.h", "sq_noise_consts.h", "sq_dpp.h", "sq_glibcf.h", "sq_ens.h", "sq_phi4_ens.h",
           "sq_qm1d_math.h", "sq_json.h", "sq_phi4_ens_ckpt_format.h"]
# per device source, the project's device files it includes, directly or through one of them: other device
# sources, the *_dev.h device headers and the ensemble's launch header (tests/test_build_table.py scans the
# sources and holds this table to them)
_ENS = ["sq_phi4_ens_dev.h", "sq_phi4_ens_launch.h", "sq_phi4.hip"]
INCLUDES = {"sq_phi4_run.hip": ["sq_phi4.hip"], "sq_phi4_ens.hip": _ENS,
            "sq_phi4_ens_flow.hip": ["sq_phi4_ens_flow_dev.h"] + _ENS,
            "sq_phi4_ens_flow_frames.hip": ["sq_phi4_ens_flow_dev.h"] + _ENS,
            "sq_phi4_ens_mala.hip": ["sq_phi4_ens_mala_dev.h"] + _ENS,
            "sq_phi4_ens_hmc.hip": ["sq_phi4_ens_mala_dev.h"] + _ENS,
            "sq_phi4_ens_exchange.hip": _ENS,
            "sq_phi4_ens_cluster.hip": ["sq_phi4_ens_cluster_dev.h"] + _ENS,
            "sq_phi4_ens_cluster_improved.hip": ["sq_phi4_ens_cluster_dev.h"] + _ENS}
# per-source flags beside COMMON.  sq_phi4_ens_mala.hip: the step loop calls the double exp once per step, and
# machine LICM hoists the twenty-odd 64-bit constants of its polynomial out of the loop into vector registers,
# where they stay for the whole call: the K = 8 instances then spill to private memory.  The kernels of that file
# keep their own loop-invariant values out of registers on purpose (the opaque copies in ens_step), so the pass
# has nothing to give them.  sq_phi4_ens_hmc.hip: the same exp behind every trajectory.
EXTRA_FLAGS = {"sq_phi4_ens_mala.hip": ["-mllvm", "-disable-machine-licm"],
               "sq_phi4_ens_hmc.hip": ["-mllvm", "-disable-machine-licm"]}
COMMON = ["-O3", "-fPIC", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-Wall",
          "-Wno-unused-function"]


def compile_command(src, path=None):
    """The compile line of device or host source `src` (a name of DEVICE_SOURCES / HOST_SOURCES), without its
    output: COMMON, the source's EXTRA_FLAGS, the arch.  path: compile that file in its place (a variant)."""
    return [HIPCC] + COMMON + EXTRA_FLAGS.get(src, []) + [f"--offload-arch={ARCH}", "-x", "hip", "-c",
                                                         path or os.path.join(CSRC, src)]


def _digest(paths, extra):
    h = hashlib.sha256()
    for p in paths:
        with open(p, "rb") as fh:
            h.update(fh.read())
    h.update(" ".join(extra).encode())
    return h.hexdigest()


def build_id(objs):
    """"phi4:<h> lib:<h>": sha256 (16 hex) of the φ⁴ kernels' object, and of every object in link order."""
    def h(paths):
        d = hashlib.sha256()
        for p in paths:
            with open(p, "rb") as fh:
                d.update(fh.read())
        return d.hexdigest()[:16]
    phi4 = [o for o in objs if os.path.basename(o) == "sq_phi4.hip.o"]
    return f"phi4:{h(phi4)} lib:{h(objs)}"


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("build failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)
    return r


def build(force=False, verbose=False):
    """Compile every HIP translation unit for gfx950 and link the library + executable."""
    os.makedirs(OBJ, exist_ok=True)
    os.makedirs(LIBDIR, exist_ok=True)
    os.makedirs(BINDIR, exist_ok=True)
    hdrs = [os.path.join(CSRC, h) for h in HEADERS] + [os.path.join(ROOT, "include", "stochquant.h")]
    jobs = []
    for src in DEVICE_SOURCES + HOST_SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ, src + ".o")
        cmd = compile_command(src)
        stamp = o + ".sha"
        dig = _digest([s] + [os.path.join(CSRC, d) for d in INCLUDES.get(src, [])] + hdrs, cmd[1:-2])
        if not force and os.path.exists(o) and os.path.exists(stamp) and open(stamp).read() == dig:
            continue
        jobs.append((cmd + ["-o", o], stamp, dig))
    with cf.ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 4)) as ex:
        for (cmd, stamp, dig), _ in zip(jobs, ex.map(lambda j: _run(j[0]), jobs)):
            with open(stamp, "w") as fh:
                fh.write(dig)
            if verbose:
                print(" ".join(cmd))
    objs = [os.path.join(OBJ, s + ".o") for s in DEVICE_SOURCES + HOST_SOURCES]
    bid = build_id(objs)
    bid_obj = os.path.join(OBJ, "sq_build_id.cpp.o")
    bid_stamp = bid_obj + ".sha"
    if jobs or force or not os.path.exists(bid_obj) or not os.path.exists(bid_stamp) or \
            open(bid_stamp).read() != bid:
        # the identity of the objects just built, compiled into the library (sq_build_id)
        _run([HIPCC] + COMMON + ["-x", "c++", f'-DSQ_BUILD_ID="{bid}"', "-c",
                                 os.path.join(CSRC, "sq_build_id.cpp"), "-o", bid_obj])
        with open(bid_stamp, "w") as fh:
            fh.write(bid)
        jobs.append(None)
    if jobs or force or not os.path.exists(LIB):
        _run([HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB] + objs + [bid_obj]
             + [f"-L{ROCM}/lib", "-lrccl", f"-Wl,-rpath,{ROCM}/lib"])
    th_src = os.path.join(CSRC, "tauhost.cpp")
    if jobs or force or not os.path.exists(TAUHOST) or \
            os.path.getmtime(th_src) > os.path.getmtime(TAUHOST):
        _run(["g++", "-O2", "-std=c++17", "-Wall", "-o", TAUHOST, th_src,
              f"-L{LIBDIR}", "-lstochquant", "-Wl,-rpath,$ORIGIN/../lib", f"-Wl,-rpath,{ROCM}/lib", "-lm"])
    root_link = os.path.join(ROOT, "tauhost.o")
    try:
        if os.path.islink(root_link) or os.path.exists(root_link):
            os.remove(root_link)
        os.symlink(os.path.relpath(TAUHOST, ROOT), root_link)
    except OSError:
        shutil.copy2(TAUHOST, root_link)
    return LIB


def build_oracle(verbose=False):
    """Build oracle/liboracle.so (test infrastructure) with its Makefile."""
    odir = os.path.join(ROOT, "oracle")
    r = subprocess.run(["make", "-C", odir, "-j4"], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("oracle build failed:\n" + r.stdout + r.stderr)
    if verbose:
        print(r.stdout)
    build_reference(verbose=verbose)
    return os.path.join(odir, "liboracle.so")


def build_reference(verbose=False):
    """Where the reference's sources exist (SQ_REFERENCE_DIR, default
    /root/reference), compile them unmodified into oracle/_ref/ by the recipe of
    oracle/ref/Makefile, for the differential tests of
    tests/test_reference_parity.py.  Nothing happens where they do not exist."""
    ref = os.environ.get("SQ_REFERENCE_DIR", "/root/reference")
    if not (os.path.isfile(os.path.join(ref, "tau_kernel.cl")) and os.path.isfile(os.path.join(ref, "tauhost.c"))):
        return None
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle", "ref"), f"REF={os.path.abspath(ref)}"],
                       capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("reference build failed:\n" + r.stdout + r.stderr)
    if verbose:
        print(r.stdout)
    return os.path.join(ROOT, "oracle", "_ref")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--force", action="store_true")
    ap.add_argument("-v", "--verbose", action="store_true")
    a = ap.parse_args(argv)
    print(build(force=a.force, verbose=a.verbose))
    print(build_oracle(verbose=a.verbose))


if __name__ == "__main__":
    sys.exit(main())
