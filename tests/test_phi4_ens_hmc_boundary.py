"""The phi^4 ensemble's hybrid Monte Carlo trajectories without a GPU: the
library exports the three calls and _lib.SIGNATURES binds them, the ABI version
stays 6, the header carries the definition, SQ_SCHEME_HMC and the words about
`randomize` and fixed lengths, arguments are checked before any device work,
Phi4Ensemble refuses scheme="hmc" wherever a scheme is taken before any library
call, the existing shape queries give what they gave (the HMC launch takes its
work-group shape and LDS layout from them, unchanged), and no instance of the
resident HMC kernel uses private memory."""
import ctypes
import inspect
import os
import re

import pytest

from test_phi4_ens_heun_boundary import _bare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"sq_phi4_ens_step_hmc": 8, "sq_phi4_ens_hmc_stats": 4, "sq_phi4_ens_hmc_reset": 3}


def test_library_exports_the_hmc_calls(sqlib):
    from stochquant_amd import _lib
    for name, nargs in CALLS.items():
        assert hasattr(sqlib, name), name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs, name
    a = _lib.SIGNATURES["sq_phi4_ens_step_hmc"][1]
    assert a[1:5] == [ctypes.c_int] * 4 and a[6] is ctypes.c_int
    assert a[5] is a[7] and a[5]._type_ is ctypes.c_double
    assert _lib.SIGNATURES["sq_phi4_ens_hmc_stats"][1][3]._type_ is ctypes.c_longlong


def test_abi_version_is_still_6(sqlib):
    from stochquant_amd import _lib
    assert sqlib.sq_abi_version() == _lib.ABI_VERSION == 6


def test_header_carries_the_definition():
    with open(os.path.join(ROOT, "include", "stochquant.h")) as fh:
        h = fh.read()
    assert re.search(r"#define\s+SQ_SCHEME_HMC\s+3\b", h) and re.search(r"#define\s+SQ_SCHEME_MALA\s+2\b", h)
    assert re.search(r"#define\s+SQ_PHI4_ENS_MAX_LEAP\s+4096\b", h)
    for name in CALLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*sq_phi4_ens\s*\*", h), name
        assert h.count(name) >= 2, name          # the prototype and the text
    for word in ("L = 1 + ((uint64) o.y * nleap >> 32)", "phi_1 = E_s(phi_0)",
                 "g = guard(fma(2h, d(phi_k), phi_k))", "t = phi_k - phi_{k-1}", "phi_{k+1} = guard(g + t)",
                 "dH = [2 h (S(phi_L) - S(phi_0)) + 1/2 (sum b^2 - sum a^2)] / sig^2",
                 "a = phi_1 - phi_0 - h d(phi_0)", "b = phi_{L-1} - phi_L - h d(phi_L)",
                 "one per trajectory", "randomize", "non-ergodic", "multiple of pi", "production", "SQ_E_STATE",
                 "guard trip"):
        assert word in h, word


def test_null_handle_and_bad_nleap_are_argument_errors(sqlib):
    out = (ctypes.c_longlong * 4)()
    for ntraj, nleap, rnd, every, measure in ((4, 3, 0, 0, 0), (0, 1, 1, 0, 0), (4, 3, 1, 2, 1), (4, 0, 0, 0, 0),
                                              (4, -1, 0, 0, 0), (4, 4097, 1, 0, 0)):
        assert sqlib.sq_phi4_ens_step_hmc(None, ntraj, nleap, rnd, every, None, measure, None) == -1
        assert sqlib.sq_last_error().decode() != ""
    assert sqlib.sq_phi4_ens_hmc_stats(None, 0, 1, out) == -1
    assert sqlib.sq_phi4_ens_hmc_reset(None, 0, 1) == -1


def test_hmc_errors_are_raised_before_any_library_call(sqlib):
    E = _bare()                                  # no handle: a library call would raise StochQuantError
    for bad in (lambda: E.step(4, scheme="hmc"),
                lambda: E.step(4, every=2, correlate=True, scheme="hmc"),
                lambda: E.step(4, every=2, flow=True, scheme="hmc"),
                lambda: E.step_flow(4, 2, scheme="hmc"),
                lambda: E.run_frames(2, scheme="hmc"),
                lambda: E.run_frames(2, flow=True, scheme="hmc"),
                lambda: E.run_frames_flow(2, scheme="hmc"),
                lambda: E.run_frame(scheme="hmc")):
        with pytest.raises(ValueError, match="step_hmc"):
            bad()
    for bad in (lambda: E.step_hmc(4, nleap=0),
                lambda: E.step_hmc(4, nleap=4097, randomize=True),
                lambda: E.step_hmc(4, nleap=3, every=0, correlate=True),
                lambda: E.step_hmc(4, nleap=3, every=-1, correlate=True)):
        with pytest.raises(ValueError, match="step_hmc"):
            bad()


def test_python_signatures(sqlib):
    from stochquant_amd import Phi4Ensemble
    sig = inspect.signature(Phi4Ensemble.step).parameters
    assert list(sig) == ["self", "n", "every", "correlate", "momenta", "scheme"] and sig["scheme"].default == "euler"
    sig = inspect.signature(Phi4Ensemble.step_hmc).parameters
    assert list(sig) == ["self", "n", "nleap", "randomize", "every", "correlate", "record"]
    assert [sig[k].default for k in list(sig)[1:]] == [1, 1, False, 0, False, False]
    sig = inspect.signature(Phi4Ensemble.step_mala).parameters
    assert list(sig) == ["self", "n", "every", "correlate", "record"]
    for name in ("hmc_stats", "hmc_reset"):
        sig = inspect.signature(getattr(Phi4Ensemble, name)).parameters
        assert list(sig) == ["self", "first", "count"] and sig["first"].default == 0 and sig["count"].default is None


def test_shape_queries_keep_the_parents_values(sqlib):
    """Values of the parent, written out: the step and correlator launches' shapes, which the HMC launch uses."""
    from stochquant_amd import Phi4Ensemble
    LDS = 160 * 1024
    assert tuple(Phi4Ensemble.shape_info((8, 2, 2048)).values()) == (8, 1024, 1, 131648, 1, 131696, 131648, LDS)
    assert tuple(Phi4Ensemble.shape_info((8, 8, 8)).values()) == (1, 128, 2, 4672, 2, 4720, 2624, LDS)
    assert tuple(Phi4Ensemble.shape_info((8, 50, 51)).values()) == (8, 640, 2, 163776, 2, 163824, 82176, LDS)
    assert tuple(Phi4Ensemble.shape_info((64, 11, 29)).values()) == (8, 640, 1, 82240, 1, 82288, 82240, LDS)
    assert tuple(Phi4Ensemble.corr_shape_info((16, 4, 31)).values()) == (2, 16696, 2, 16744, 8760, 16)
    assert tuple(Phi4Ensemble.corr_shape_info((8, 50, 51)).values())[:2] == (1, 82176 + 8 * 51)


def test_hmc_kernels_use_no_private_memory(sqlib):
    from stochquant_amd import isa_check
    md = isa_check.kernel_metadata(os.path.join(ROOT, "stochquant_amd", "lib", "libstochquant.so"))
    hmc = {k: v for k, v in md.items() if "phi4_ens_hmc_kernel" in k}
    assert len(hmc) >= 8, sorted(k for k in md if "phi4_ens" in k)      # K = 1, 2, 4, 8 x plain, correlator
    for K in (1, 2, 4, 8):
        assert sum(f"phi4_ens_hmc_kernelILi{K}E" in k for k in hmc) >= 2, (K, sorted(hmc))
    bad = {k: v for k, v in hmc.items() if v.get("private", 0) != 0 or v.get("vgpr_spill", 0) != 0}
    assert bad == {}, bad
