"""The phi^4 ensemble checkpoint's format check (csrc/sq_phi4_ens_ckpt_format.cpp: pure host C++, no HIP) as a
stand-alone program under the address and undefined-behaviour sanitizers (tests/ckpt_format_check.cpp), in the idiom
of test_buf.py: over a corpus written here it must say "accepted" for the valid set alone, "refused" for the rest,
and the sanitizers must have nothing to report.  The corpus: a valid set made by the NumPy writer
(tests/phi4_ens_checkpoint_format.py), its .json cut at every length, and 200 single-byte substitutions at fixed-seed
positions in each of the three files, and 200 more in the metadata drawn from JSON's own alphabet.  One exception: a substitution that leaves the metadata's meaning unchanged
(white space, a digit of an informative decimal copy) is accepted; the NumPy reader says which those are.

The field digests of a sizeable file are taken on several threads (from 1 MiB of fields on).  A second set, nine
lattices of 32,768 sites, crosses that threshold: it runs under the same two sanitizers, and once more in a build
with the thread sanitizer where this machine's g++ has a working one."""
import os
import subprocess

import numpy as np
import pytest

import phi4_ens_checkpoint_format as fmt

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "stochquant_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ckpt_check") / "ckpt_format_check")
    return build(out, "address,undefined")


def build(out, sanitize):
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", f"-fsanitize={sanitize}", "-fno-sanitize-recover=all",
                    "-pthread", "-o", out, os.path.join(HERE, "ckpt_format_check.cpp"),
                    os.path.join(CSRC, "sq_phi4_ens_ckpt_format.cpp")], check=True)
    return out


def run(exe, *args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, errors="replace")
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout + r.stderr
    return r.stdout.splitlines()


def valid_set(d):
    """A checkpoint with every optional section, momenta, flow levels and a ladder; awkward values inside."""
    dims, R, loops = (8, 2, 2), 3, 4
    rng = np.random.default_rng(11)
    phi = rng.standard_normal((R, 2, 2, 8)).astype(np.float32)
    phi[0, 0, 0, :4] = [-0.0, np.nan, np.inf, -np.inf]
    st = fmt.default_state(dims, R, loops, M=2, F=2, frame_records=True, mala=True, hmc=True)
    st["step"][:] = (1 << 40) + 5
    st["corr_G"][:] = rng.standard_normal(st["corr_G"].shape)
    st["frame_V"][1] = np.inf
    path = os.path.join(d, "ck")
    fmt.write(path, phi, st, loops=loops, clamp=1000.0, exchange_round=(1 << 40) + 5, cluster_sweep=(1 << 33) + 1,
              ladder=3, momenta=[(1, 0), (0, 1)], flow_levels=[1, 3], flow_eps=0.01)
    return path


def test_the_valid_set_is_accepted(exe, tmp_path):
    path = valid_set(str(tmp_path))
    fmt.read(path)
    assert run(exe, "--path", path) == ["accepted"]


def test_the_metadata_cut_at_every_length_is_refused(exe, tmp_path):
    path = valid_set(str(tmp_path))
    n = os.path.getsize(path + ".json")
    assert run(exe, "--prefixes", path + ".json") == [f"prefixes {n} refused {n}"]
    with open(path + ".json", "rb") as fh:
        text = fh.read()
    for k in (0, 1, n // 2, n - 1):  # and the NumPy reader agrees where it is asked
        with pytest.raises(fmt.Refused):
            fmt.parse_meta(text[:k])


def test_single_byte_substitutions_are_refused_unless_the_meaning_stays(exe, tmp_path):
    path = valid_set(str(tmp_path))
    names = {"json": path + ".json", "state": path + ".state", "field": path}
    orig = {}
    for k, p in names.items():
        with open(p, "rb") as fh:
            orig[k] = fh.read()
    rng = np.random.default_rng(2024)
    lines, expect = [], []
    # the fourth corpus probes the grammar: bytes of JSON's own alphabet into the metadata
    alphabet = b' \t\n\r0123456789-+.eE,:[]{}"\\anulltruefalse'
    for tag in ("json", "state", "field", "json_alphabet"):
        which = tag.split("_")[0]
        data = orig[which]
        for i in range(200):
            pos = int(rng.integers(len(data)))
            if tag == "json_alphabet":
                new = next(b for b in (alphabet[int(k)] for k in rng.integers(len(alphabet), size=64)) if b != data[pos])
            else:
                new = int(rng.integers(255))
                new += new >= data[pos]  # another byte
            mutated = data[:pos] + bytes([new]) + data[pos + 1:]
            p = os.path.join(str(tmp_path), f"{tag}_{i}")
            with open(p, "wb") as fh:
                fh.write(mutated)
            triple = dict(names, **{which: p})
            lines.append("\t".join(triple[k] for k in ("json", "state", "field")))
            same = False
            if which == "json":  # the one exception: the reader takes it, with the meaning of the original
                try:
                    same = fmt.meaning(fmt.parse_meta(mutated)) == fmt.meaning(fmt.parse_meta(data))
                except fmt.Refused:
                    pass
            expect.append(same)
    manifest = os.path.join(str(tmp_path), "manifest")
    with open(manifest, "w") as fh:
        fh.write("\n".join(lines) + "\n")
    got = run(exe, "--sets", manifest)
    assert len(got) == len(expect) == 800
    wrong = [(lines[i].split("\t"), got[i]) for i in range(800) if (got[i] == "accepted") != expect[i]]
    assert not wrong, wrong[:5]
    assert all(g == "accepted" or g.startswith("refused: ") for g in got)
    assert sum(expect) < 60  # the corpus is a corpus of refusals


def large_set(d):
    """Nine lattices of (64, 256, 2): 1.1 MiB of fields, above the size at which the digests go onto threads."""
    dims, R, loops = (64, 256, 2), 9, 2
    phi = np.random.default_rng(4).standard_normal((R, 2, 256, 64)).astype(np.float32)
    path = os.path.join(d, "big")
    fmt.write(path, phi, fmt.default_state(dims, R, loops), loops=loops)
    bad = os.path.join(d, "big_flipped")
    with open(path, "rb") as fh:
        b = bytearray(fh.read())
    b[len(b) - 5 * 4 * 32768 - 3] ^= 0x04  # replica 3
    with open(bad, "wb") as fh:
        fh.write(bytes(b))
    manifest = os.path.join(d, "manifest_big")
    with open(manifest, "w") as fh:
        fh.write("\t".join((path + ".json", path + ".state", path)) + "\n")
        fh.write("\t".join((path + ".json", path + ".state", bad)) + "\n")
    return manifest


def test_the_threaded_digest_under_address_and_ub_sanitizers(exe, tmp_path):
    got = run(exe, "--sets", large_set(str(tmp_path)))
    assert got[0] == "accepted" and got[1].startswith("refused: the field of replica 3"), got


def test_the_threaded_digest_under_the_thread_sanitizer(tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("#include <thread>\nint main() { std::thread t([] {}); t.join(); }\n")
    ok = subprocess.run(["g++", "-fsanitize=thread", "-pthread", "-o", str(tmp_path / "probe"), str(probe)],
                        capture_output=True).returncode == 0 and \
        subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode == 0
    if not ok:
        pytest.skip("g++ has no working thread sanitizer on this machine")
    tsan = build(str(tmp_path / "ckpt_format_check_tsan"), "thread")
    got = run(tsan, "--sets", large_set(str(tmp_path)))
    assert got[0] == "accepted" and got[1].startswith("refused: the field of replica 3"), got
