"""The phi^4 ensemble's checkpoint and field digest without a GPU: the library exports the four calls and
_lib.SIGNATURES binds them, the ABI version stays 6, null arguments are argument errors, the header carries the
format, the sources are in the build lists, the kernel spills nothing, and sq_phi4_ensemble_checkpoint_info with
verify -- which needs no device -- accepts checkpoints written by the NumPy writer of
tests/phi4_ens_checkpoint_format.py and refuses, with SQ_E_ARG and a message naming the cause, every damaged one."""
import ctypes
import json
import os

import numpy as np
import pytest

import phi4_ens_checkpoint_format as fmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"sq_phi4_ensemble_save": 2, "sq_phi4_ensemble_load": 3, "sq_phi4_ensemble_checkpoint_info": 4,
         "sq_phi4_ensemble_digest": 4}
DIMS, R, LOOPS = (8, 2, 2), 3, 4


def test_library_exports_the_calls(sqlib):
    from stochquant_amd import _lib
    S = _lib.SIGNATURES
    for name, nargs in CALLS.items():
        assert hasattr(sqlib, name), name
        restype, argtypes = S[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs, name
    assert S["sq_phi4_ensemble_save"][1] == [ctypes.c_void_p, ctypes.c_char_p]
    assert S["sq_phi4_ensemble_load"][1] == [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int]
    a = S["sq_phi4_ensemble_checkpoint_info"][1]
    assert a[0] is ctypes.c_char_p and a[1] is ctypes.c_int and a[2]._type_ is ctypes.c_longlong and \
        a[3]._type_ is ctypes.c_double
    a = S["sq_phi4_ensemble_digest"][1]
    assert a[:3] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int] and a[3]._type_ is ctypes.c_ulonglong
    assert len([n for n in S if n.startswith("sq_phi4_ens_")]) == 72  # the closed family stays closed


def test_abi_version_is_still_6(sqlib):
    from stochquant_amd import _lib
    assert sqlib.sq_abi_version() == _lib.ABI_VERSION == 6


def test_null_arguments_are_argument_errors(sqlib):
    info = (ctypes.c_longlong * 8)()
    out = (ctypes.c_ulonglong * 1)()
    for call in (lambda: sqlib.sq_phi4_ensemble_save(None, b"x"), lambda: sqlib.sq_phi4_ensemble_save(None, None),
                 lambda: sqlib.sq_phi4_ensemble_load(None, b"x", 0), lambda: sqlib.sq_phi4_ensemble_load(None, None, 1),
                 lambda: sqlib.sq_phi4_ensemble_checkpoint_info(None, 0, info, None),
                 lambda: sqlib.sq_phi4_ensemble_checkpoint_info(b"x", 1, None, None),
                 lambda: sqlib.sq_phi4_ensemble_digest(None, 0, 1, out),
                 lambda: sqlib.sq_phi4_ensemble_digest(None, 0, 0, None)):
        assert call() == -1
        assert sqlib.sq_last_error().decode() != ""


def test_header_carries_the_format():
    with open(os.path.join(ROOT, "include", "stochquant.h")) as fh:
        h = fh.read()
    for name in CALLS:
        assert f"int {name}(" in h, name
    for word in ("0xBF58476D1CE4E5B9", "0x94D049BB133111EB", "x ^= x >> 30", "x ^= x >> 27", "x ^= x >> 31",
                 "(uint64(i) << 32) | bits32(phi_r[i])", "Not saved, by decision", "stochquant-phi4-ensemble",
                 "state_digest", "meta_digest", "field_digest", "8-byte boundary", "the .json last", "fields_only",
                 "restarts at zero", "frame_records", "exchange_stats", "cluster_stats", "Seeds come"):
        assert word in h, word
    for name, _, _ in fmt.section_table((8, 8, 8), 2, 3, 1, 1):
        assert name in h, name
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        d = fh.read()
    assert "sq_phi4_ensemble_save" in d and "meta_digest" in d


def test_the_sources_are_in_the_build_lists():
    from stochquant_amd import build
    assert "sq_phi4_ens_digest.hip" in build.DEVICE_SOURCES and "sq_phi4_ens_digest.hip" not in build.INCLUDES
    assert "sq_phi4_ens_ckpt_format.cpp" in build.HOST_SOURCES and "sq_phi4_ens_ckpt.cpp" in build.HOST_SOURCES
    for f, banned in (("sq_phi4_ens_ckpt_format.cpp", ("hip", "sq_internal.h", "sq_ctx.h")),
                      ("sq_phi4_ens_ckpt_format.h", ("hip",)), ("sq_json.h", ("hip",))):
        with open(os.path.join(build.CSRC, f)) as fh:
            inc = [ln for ln in fh.read().splitlines() if ln.lstrip().startswith("#include")]
        assert not [ln for ln in inc if any(b in ln for b in banned)], (f, inc)  # the format is pure host C++
    with open(os.path.join(build.CSRC, "sq_io.cpp")) as fh:
        io = fh.read()
    assert '#include "sq_json.h"' in io and "strtoull" not in io  # the helpers were lifted, not copied


def test_the_digest_kernel_spills_nothing(sqlib):
    from stochquant_amd import isa_check
    md = isa_check.kernel_metadata(os.path.join(ROOT, "stochquant_amd", "lib", "libstochquant.so"))
    k = {n: v for n, v in md.items() if "phi4_ens_digest_kernel" in n}
    assert len(k) == 1, sorted(k)
    v = next(iter(k.values()))
    assert v.get("private", 0) == 0 and v.get("vgpr_spill", 0) == 0 and v.get("sgpr_spill", 0) == 0, v


# ---- checkpoint_info(verify) against the NumPy writer ----
def make(d, optional=True, **kw):
    rng = np.random.default_rng(5)
    phi = rng.standard_normal((R, DIMS[2], DIMS[1], DIMS[0])).astype(np.float32)
    phi[1, 0, 0, :4] = [-0.0, np.nan, np.inf, -np.inf]
    M, F = (2, 2) if optional else (0, 0)
    st = fmt.default_state(DIMS, R, LOOPS, M=M, F=F, frame_records=optional, mala=optional, hmc=optional)
    st["corr_G"][:] = rng.standard_normal(st["corr_G"].shape)
    path = os.path.join(str(d), "ck")
    args = dict(loops=LOOPS, clamp=250.0, adapt_dtau=False)
    if optional:
        args.update(ladder=3, momenta=[(1, 0), (0, 1)], flow_levels=[0, 2], flow_eps=0.02, flow_m2=0.5)
    args.update(kw)
    return path, fmt.write(path, phi, st, **args), phi, st


def info(sqlib, path, verify=1):
    out = (ctypes.c_longlong * 8)()
    clamp = ctypes.c_double(-1.0)
    rc = sqlib.sq_phi4_ensemble_checkpoint_info(os.fsencode(path), verify, out, ctypes.byref(clamp))
    return rc, list(out), clamp.value, sqlib.sq_last_error().decode()


@pytest.mark.parametrize("optional", [True, False])
def test_info_accepts_what_the_numpy_writer_made(sqlib, tmp_path, optional):
    path, m, phi, st = make(tmp_path, optional)
    rc, out, clamp, msg = info(sqlib, path)
    assert rc == 0, msg
    assert out == [1, 8, 2, 2, R, LOOPS, 0, len(st)] and clamp == 250.0
    assert info(sqlib, path, 0)[:3] == (0, out, 250.0)
    assert sqlib.sq_phi4_ensemble_checkpoint_info(os.fsencode(path), 1, (ctypes.c_longlong * 8)(), None) == 0
    from stochquant_amd import Phi4Ensemble
    assert Phi4Ensemble.checkpoint_info(path, verify=True) == {
        "version": 1, "shape": (8, 2, 2), "replicas": R, "loops": LOOPS, "adapt_dtau": False, "sections": len(st),
        "clamp": 250.0}
    got_m, got_phi, got_st = fmt.read(path)  # and the reader reads its writer
    assert got_phi.view(np.uint32).tolist() == phi.view(np.uint32).tolist() and list(got_st) == list(st)
    assert m["field_digest"] == [fmt.field_digest(phi[r]) for r in range(R)]


def rewrite(path, change):
    with open(path + ".json") as fh:
        m = json.load(fh)
    change(m)
    m["meta_digest"] = fmt.meta_digest(m)
    fmt.write_meta(path, m)


def flip(path, pos, bit=0):
    with open(path, "r+b") as fh:
        fh.seek(pos)
        b = fh.read(1)[0]
        fh.seek(pos)
        fh.write(bytes([b ^ (1 << bit)]))


def resize(path, delta):
    with open(path, "rb") as fh:
        b = fh.read()
    with open(path, "wb") as fh:
        fh.write(b[:delta] if delta < 0 else b + b"\0" * delta)


def append(path, b):
    with open(path, "ab") as fh:
        fh.write(b)


def other_npy(path, a):
    np.save(path + ".tmp.npy", a)
    os.replace(path + ".tmp.npy", path)


def drop(m, name):
    m["sections"] = [s for s in m["sections"] if s["name"] != name]


def section(m, name):
    return next(s for s in m["sections"] if s["name"] == name)


DAMAGE = {
    "no json": (lambda p: os.remove(p + ".json"), "cannot read"),
    "no state": (lambda p: os.remove(p + ".state"), "cannot read"),
    "no field": (lambda p: os.remove(p), "cannot read"),
    "version 2": (lambda p: rewrite(p, lambda m: m.update(version=2)), "version 2"),
    "format name": (lambda p: rewrite(p, lambda m: m.update(format="stochquant-phi4-slab")), "format"),
    "npy dtype": (lambda p: other_npy(p, np.zeros((R, 2, 2, 8), dtype=np.float64)), "dtype"),
    "npy fortran": (lambda p: other_npy(p, np.asfortranarray(np.ones((R, 2, 2, 8), dtype=np.float32))), "Fortran"),
    "npy shape": (lambda p: other_npy(p, np.zeros((R, 2, 8, 2), dtype=np.float32)), "shape"),
    "field short": (lambda p: resize(p, -1), "bytes"),
    "field long": (lambda p: resize(p, 1), "bytes"),
    "field bit": (lambda p: flip(p, os.path.getsize(p) - 7, 3), "replica 2"),
    "state bit": (lambda p: flip(p + ".state", 41, 6), "state file"),
    "unknown section": (lambda p: rewrite(p, lambda m: section(m, "walkers").update(name="walkerz")), "unknown section"),
    "missing section": (lambda p: rewrite(p, lambda m: drop(m, "cluster_stats")), "cluster_stats"),
    "shape vs R": (lambda p: rewrite(p, lambda m: section(m, "seed").update(shape=[R + 1])), "seed"),
    "offset past end": (lambda p: rewrite(p, lambda m: section(m, "cluster_stats").update(offset=m["state_bytes"])),
                        "past the end"),
    "overlap": (lambda p: rewrite(p, lambda m: section(m, "step").update(offset=section(m, "seed")["offset"])),
                "overlap"),
    "Lx 12": (lambda p: rewrite(p, lambda m: m.update(dims=[12, 2, 2])), "Lx in {8, 16, 32, 64}"),
    "R 0": (lambda p: rewrite(p, lambda m: m.update(R=0)), "R must be"),
    # beyond the issue's list: what only the metadata's own digest, or the library's own rules, can catch
    "round changed": (lambda p: rewrite(p, lambda m: None) or flip(p + ".json", _digit(p, "exchange_round")), "meta_digest"),
    "ladder 2": (lambda p: rewrite(p, lambda m: m.update(ladder=2)), "ladder"),
    "momentum outside": (lambda p: rewrite(p, lambda m: m.update(momenta=[[8, 0], [0, 1]])), "momentum"),
    "levels descend": (lambda p: rewrite(p, lambda m: m.update(flow_levels=[2, 2])), "flow_levels"),
    "trailing newline": (lambda p: append(p + ".json", b"\n"), None),
}


def _digit(path, key):
    with open(path + ".json", "rb") as fh:
        t = fh.read()
    return t.index(b'"%s": ' % key.encode()) + len(key) + 4  # its first digit: bit 0 makes another digit


@pytest.mark.parametrize("what", sorted(DAMAGE))
def test_info_refuses_a_damaged_checkpoint(sqlib, tmp_path, what):
    path, _, _, _ = make(tmp_path)
    assert info(sqlib, path)[0] == 0
    damage, word = DAMAGE[what]
    damage(path)
    rc, _, _, msg = info(sqlib, path)
    if word is None:  # white space behind the brace changes nothing: both readers take it
        assert rc == 0 and fmt.read(path)
        return
    assert rc == -1 and word in msg, (rc, msg)
    with pytest.raises(fmt.Refused):  # the NumPy reader refuses it too
        fmt.read(path)


def test_info_on_a_shape_without_room_for_momenta(sqlib, tmp_path):
    """(8, 2, 2048) is a legal shape whose one LDS image leaves no room for momentum projections: a checkpoint of
    it without momenta is whole, one with momenta is refused as sq_phi4_ens_set_momenta refuses them."""
    dims = (8, 2, 2048)
    phi = np.zeros((1, 2048, 2, 8), dtype=np.float32)
    path = os.path.join(str(tmp_path), "tall")
    fmt.write(path, phi, fmt.default_state(dims, 1, LOOPS), loops=LOOPS)
    rc, out, _, msg = info(sqlib, path)
    assert rc == 0 and out[1:5] == [8, 2, 2048, 1], msg
    fmt.write(path, phi, fmt.default_state(dims, 1, LOOPS, M=1), loops=LOOPS, momenta=[(1, 0)])
    rc, _, _, msg = info(sqlib, path)
    assert rc == -1 and "momenta" in msg and "LDS" in msg, msg
    assert info(sqlib, path, 0)[0] == 0


def test_info_applies_the_parameter_bound(sqlib, tmp_path):
    """A set of files that is whole but holds a replica sq_phi4_ens_create would refuse."""
    path, m, phi, st = make(tmp_path)
    st["dtau"][1] = -0.01
    fmt.write(path, phi, st, loops=LOOPS, clamp=250.0, adapt_dtau=False, ladder=3, momenta=[(1, 0), (0, 1)],
              flow_levels=[0, 2], flow_eps=0.02, flow_m2=0.5)
    rc, _, _, msg = info(sqlib, path)
    assert rc == -1 and "replica 1" in msg
    assert info(sqlib, path, 0)[0] == 0  # without verify only the metadata is read


def test_the_python_digest_is_the_definition():
    """mix and the sum, written out site by site in Python integers."""
    rng = np.random.default_rng(9)
    row = rng.standard_normal(32).astype(np.float32)
    row[:3] = [-0.0, np.nan, np.inf]
    mask, d = (1 << 64) - 1, 0
    for i, w in enumerate(row.view(np.uint32).tolist()):
        x = (i << 32) | w
        x ^= x >> 30
        x = (x * 0xBF58476D1CE4E5B9) & mask
        x ^= x >> 27
        x = (x * 0x94D049BB133111EB) & mask
        x ^= x >> 31
        d = (d + x) & mask
    assert fmt.field_digest(row) == d
    assert fmt.digest_bytes(row.tobytes() + b"\x07") == (d + int(fmt.mix((32 << 32) | 7))) & mask  # zero-padded
