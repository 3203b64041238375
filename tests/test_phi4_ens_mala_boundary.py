"""The phi^4 ensemble's Metropolis-adjusted Langevin step without a GPU: the
library exports the three calls and _lib.SIGNATURES binds them, the ABI version
stays 6, the header documents them and SQ_SCHEME_MALA, arguments are checked
before any device work, Phi4Ensemble refuses what MALA does not run with before
any library call, the existing shape queries give what they gave (the MALA
launch takes its work-group shape and LDS layout from them, unchanged), the
accept stream is the fourth noise stream, and no instance of the resident MALA
kernel uses private memory."""
import ctypes
import inspect
import os
import re

import pytest

from test_phi4_ens_heun_boundary import _bare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"sq_phi4_ens_step_mala": 6, "sq_phi4_ens_mala_stats": 4, "sq_phi4_ens_mala_reset": 3}


def test_library_exports_the_mala_calls(sqlib):
    from stochquant_amd import _lib
    for name, nargs in CALLS.items():
        assert hasattr(sqlib, name), name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs, name
    a = _lib.SIGNATURES["sq_phi4_ens_step_mala"][1]
    assert a[1:3] == [ctypes.c_int, ctypes.c_int] and a[4] is ctypes.c_int
    assert a[3] is a[5] and a[3]._type_ is ctypes.c_double
    assert _lib.SIGNATURES["sq_phi4_ens_mala_stats"][1][3]._type_ is ctypes.c_longlong


def test_abi_version_is_still_6(sqlib):
    from stochquant_amd import _lib
    assert sqlib.sq_abi_version() == _lib.ABI_VERSION == 6


def test_header_documents_the_step():
    with open(os.path.join(ROOT, "include", "stochquant.h")) as fh:
        h = fh.read()
    assert re.search(r"#define\s+SQ_SCHEME_MALA\s+2\b", h)
    assert re.search(r"#define\s+SQ_SCHEME_EULER\s+0\b", h) and re.search(r"#define\s+SQ_SCHEME_HEUN\s+1\b", h)
    for name in CALLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*sq_phi4_ens\s*\*", h), name
        assert h.count(name) >= 2, name          # the prototype and the text
    for word in ("dH = [2 h (S(p) - S(phi)) + 1/2 (sum b^2 - sum a^2)] / sig^2", "SQ_E_STATE", "thermalise",
                 "Philox4x32-10", "guard trip"):
        assert word in h, word


def test_accept_stream_is_the_fourth():
    with open(os.path.join(ROOT, "stochquant_amd", "csrc", "sq_noise_consts.h")) as fh:
        h = fh.read()
    got = dict(re.findall(r"constexpr uint32_t (kStream\w+) = (\d+);", h))
    assert got == {"kStreamField": "0", "kStreamOmega": "1", "kStreamInit": "2", "kStreamAccept": "3"}


def test_null_handle_is_an_argument_error(sqlib):
    out = (ctypes.c_longlong * 3)()
    for nsteps, every, measure in ((4, 0, 0), (0, 0, 0), (4, 2, 1), (4, 2, 2)):
        assert sqlib.sq_phi4_ens_step_mala(None, nsteps, every, None, measure, None) == -1
        assert sqlib.sq_last_error().decode() != ""
    assert sqlib.sq_phi4_ens_mala_stats(None, 0, 1, out) == -1
    assert sqlib.sq_phi4_ens_mala_reset(None, 0, 1) == -1


def test_mala_errors_are_raised_before_any_library_call(sqlib):
    E = _bare()                                  # no handle: a library call would raise StochQuantError
    for bad in (lambda: E.step(4, every=2, momenta=True, scheme="mala"),
                lambda: E.step(4, every=2, flow=True, scheme="mala"),
                lambda: E.step(4, every=0, correlate=True, scheme="mala"),
                lambda: E.step_mala(4, every=-1, correlate=True),
                lambda: E.step_flow(4, 2, scheme="mala"),
                lambda: E.run_frames(2, scheme="mala"),
                lambda: E.run_frames(2, flow=True, scheme="mala"),
                lambda: E.run_frames_flow(2, scheme="mala"),
                lambda: E.run_frame(scheme="mala"),
                lambda: E.step(4, scheme="MALA")):
        with pytest.raises(ValueError):
            bad()


def test_python_signatures(sqlib):
    from stochquant_amd import Phi4Ensemble
    sig = inspect.signature(Phi4Ensemble.step).parameters
    assert list(sig) == ["self", "n", "every", "correlate", "momenta", "scheme"] and sig["scheme"].default == "euler"
    sig = inspect.signature(Phi4Ensemble.step_mala).parameters
    assert list(sig) == ["self", "n", "every", "correlate", "record"]
    assert [sig[k].default for k in ("n", "every", "correlate", "record")] == [1, 0, False, False]
    assert callable(Phi4Ensemble.mala_stats) and callable(Phi4Ensemble.mala_reset)


def test_shape_queries_keep_the_parents_values(sqlib):
    """Values of the parent, written out: the step and correlator launches' shapes, which the MALA launch uses."""
    from stochquant_amd import Phi4Ensemble
    LDS = 160 * 1024
    assert tuple(Phi4Ensemble.shape_info((8, 2, 2048)).values()) == (8, 1024, 1, 131648, 1, 131696, 131648, LDS)
    assert tuple(Phi4Ensemble.shape_info((8, 8, 8)).values()) == (1, 128, 2, 4672, 2, 4720, 2624, LDS)
    assert tuple(Phi4Ensemble.shape_info((8, 50, 51)).values()) == (8, 640, 2, 163776, 2, 163824, 82176, LDS)
    assert tuple(Phi4Ensemble.shape_info((64, 11, 29)).values()) == (8, 640, 1, 82240, 1, 82288, 82240, LDS)
    assert tuple(Phi4Ensemble.corr_shape_info((16, 4, 31)).values()) == (2, 16696, 2, 16744, 8760, 16)
    assert tuple(Phi4Ensemble.corr_shape_info((8, 50, 51)).values())[:2] == (1, 82176 + 8 * 51)


def test_mala_kernels_use_no_private_memory(sqlib):
    from stochquant_amd import isa_check
    md = isa_check.kernel_metadata(os.path.join(ROOT, "stochquant_amd", "lib", "libstochquant.so"))
    mala = {k: v for k, v in md.items() if "phi4_ens_mala_kernel" in k}
    assert len(mala) >= 8, sorted(k for k in md if "phi4_ens" in k)     # K = 1, 2, 4, 8 x plain, correlator
    for K in (1, 2, 4, 8):
        assert sum(f"phi4_ens_mala_kernelILi{K}E" in k for k in mala) >= 2, (K, sorted(mala))
    bad = {k: v for k, v in mala.items() if v.get("private", 0) != 0 or v.get("vgpr_spill", 0) != 0}
    assert bad == {}, bad
