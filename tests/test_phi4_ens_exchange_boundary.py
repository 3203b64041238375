"""The phi^4 ensemble's replica exchange without a GPU: the library exports the
calls and _lib.SIGNATURES binds them, the ABI version stays 6, the header
carries the definition and its limits, a null handle is an argument error,
Phi4Ensemble raises its argument errors before any library call, the exchange
launch reports the moments launch's work-group shape, the existing shape
queries give what they gave, and no instance of the exchange kernel uses
private memory."""
import ctypes
import inspect
import os
import re

import pytest

from test_phi4_ens_heun_boundary import _bare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"sq_phi4_ens_set_ladder": 2, "sq_phi4_ens_get_ladder": 2, "sq_phi4_ens_exchange_round": 2,
         "sq_phi4_ens_set_exchange_round": 2, "sq_phi4_ens_exchange": 3, "sq_phi4_ens_step_hmc_exchange": 10,
         "sq_phi4_ens_exchange_stats": 4, "sq_phi4_ens_walkers": 4, "sq_phi4_ens_exchange_reset": 4,
         "sq_phi4_ens_exchange_shape_info": 2}


def test_library_exports_the_exchange_calls(sqlib):
    from stochquant_amd import _lib
    for name, nargs in CALLS.items():
        assert hasattr(sqlib, name), name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs, name
    S = _lib.SIGNATURES
    assert S["sq_phi4_ens_set_ladder"][1][1] is ctypes.c_int
    assert S["sq_phi4_ens_get_ladder"][1][1]._type_ is ctypes.c_int
    assert S["sq_phi4_ens_exchange_round"][1][1]._type_ is ctypes.c_ulonglong
    assert S["sq_phi4_ens_set_exchange_round"][1][1] is ctypes.c_ulonglong
    a = S["sq_phi4_ens_exchange"][1]
    assert a[1] is ctypes.c_int and a[2]._type_ is ctypes.c_double
    a = S["sq_phi4_ens_step_hmc_exchange"][1]
    assert a[1:6] == [ctypes.c_int] * 5 and a[7] is ctypes.c_int
    assert a[6] is a[8] is a[9] and a[6]._type_ is ctypes.c_double
    assert S["sq_phi4_ens_exchange_stats"][1][3]._type_ is ctypes.c_longlong
    assert S["sq_phi4_ens_walkers"][1][3]._type_ is ctypes.c_int
    assert S["sq_phi4_ens_exchange_reset"][1][1:] == [ctypes.c_int] * 3
    assert [t._type_ for t in S["sq_phi4_ens_exchange_shape_info"][1]] == [ctypes.c_int] * 2


def test_abi_version_is_still_6(sqlib):
    from stochquant_amd import _lib
    assert sqlib.sq_abi_version() == _lib.ABI_VERSION == 6


def test_header_carries_the_definition():
    with open(os.path.join(ROOT, "include", "stochquant.h")) as fh:
        h = fh.read()
    for name in CALLS:
        first = r"const\s+int\s+dims\[3\]" if name.endswith("shape_info") else r"sq_phi4_ens\s*\*"
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*" + first, h), name
        assert len(re.findall(r"\b" + name + r"\b", h)) >= 2, name          # the prototype and the text
    for word in ("Delta = (p_a - p_b)(S2_b - S2_a) - (beta_a - beta_b)(NN_b - NN_a) + (q_a - q_b)(S4_b - S4_a)",
                 "beta_r = 2 h_r / (sig_r sig_r)", "p_r = beta_r (3 + m2_r / 2)", "q_r = beta_r (lam6_r / 4)",
                 "{0, 4 << 24, x lo, x hi}", "o = x & 1", "u < exp(-Delta)", "NaN Delta", "SQ_E_STATE",
                 "equilibrium fields", "walker", "ntraj % every == 0"):
        assert word in h, word


def test_the_exchange_stream_is_declared_beside_the_exchange_code():
    with open(os.path.join(ROOT, "stochquant_amd", "csrc", "sq_phi4_ens.h")) as fh:
        assert re.search(r"constexpr uint32_t kPhi4EnsStreamExchange = 4;", fh.read())
    with open(os.path.join(ROOT, "stochquant_amd", "csrc", "sq_phi4_ens_exchange.hip")) as fh:
        assert "kPhi4EnsStreamExchange << 24" in fh.read()


def test_null_handle_is_an_argument_error(sqlib):
    n, x = ctypes.c_int(0), ctypes.c_ulonglong(0)
    st, wk = (ctypes.c_longlong * 2)(), (ctypes.c_int * 1)()
    for call in (lambda: sqlib.sq_phi4_ens_set_ladder(None, 4),
                 lambda: sqlib.sq_phi4_ens_set_ladder(None, 0),
                 lambda: sqlib.sq_phi4_ens_get_ladder(None, ctypes.byref(n)),
                 lambda: sqlib.sq_phi4_ens_exchange_round(None, ctypes.byref(x)),
                 lambda: sqlib.sq_phi4_ens_set_exchange_round(None, 7),
                 lambda: sqlib.sq_phi4_ens_exchange(None, 1, None),
                 lambda: sqlib.sq_phi4_ens_exchange(None, 0, None),
                 lambda: sqlib.sq_phi4_ens_step_hmc_exchange(None, 2, 2, 3, 1, 1, None, 1, None, None),
                 lambda: sqlib.sq_phi4_ens_step_hmc_exchange(None, 0, 0, 1, 0, 0, None, 0, None, None),
                 lambda: sqlib.sq_phi4_ens_exchange_stats(None, 0, 1, st),
                 lambda: sqlib.sq_phi4_ens_walkers(None, 0, 1, wk),
                 lambda: sqlib.sq_phi4_ens_exchange_reset(None, 0, 1, 1)):
        assert call() == -1
        assert sqlib.sq_last_error().decode() != ""
    assert sqlib.sq_phi4_ens_exchange_shape_info(None, None) == -1
    assert sqlib.sq_last_error().decode() != ""


def test_python_errors_are_raised_before_any_library_call(sqlib):
    E = _bare()                                  # no handle: a library call would raise StochQuantError
    for bad in (lambda: E.step_hmc_exchange(4, nleap=0),
                lambda: E.step_hmc_exchange(4, ntraj=2, nleap=4097, randomize=True),
                lambda: E.step_hmc_exchange(4, ntraj=2, nleap=3, every=0, correlate=True),
                lambda: E.step_hmc_exchange(4, ntraj=2, nleap=3, every=-1, correlate=True),
                lambda: E.step_hmc_exchange(4, ntraj=3, nleap=3, every=2),
                lambda: E.step_hmc_exchange(4, ntraj=1, nleap=1, every=2, correlate=True)):
        with pytest.raises(ValueError, match="step_hmc_exchange"):
            bad()


def test_python_signatures(sqlib):
    from stochquant_amd import Phi4Ensemble
    sig = inspect.signature(Phi4Ensemble.step_hmc_exchange).parameters
    assert list(sig) == ["self", "rounds", "ntraj", "nleap", "randomize", "every", "correlate", "record"]
    assert [sig[k].default for k in list(sig)[2:]] == [1, 1, False, 0, False, False]
    sig = inspect.signature(Phi4Ensemble.exchange).parameters
    assert list(sig) == ["self", "rounds", "record"] and [sig[k].default for k in list(sig)[1:]] == [1, False]
    for name in ("exchange_stats", "walkers"):
        sig = inspect.signature(getattr(Phi4Ensemble, name)).parameters
        assert list(sig) == ["self", "first", "count"] and sig["first"].default == 0 and sig["count"].default is None
    sig = inspect.signature(Phi4Ensemble.exchange_reset).parameters
    assert list(sig) == ["self", "first", "count", "walkers"] and sig["walkers"].default is False
    assert list(inspect.signature(Phi4Ensemble.set_ladder).parameters) == ["self", "n"]
    assert isinstance(Phi4Ensemble.ladder, property) and Phi4Ensemble.ladder.fset is None
    assert isinstance(Phi4Ensemble.exchange_round, property) and Phi4Ensemble.exchange_round.fset is not None
    assert isinstance(inspect.getattr_static(Phi4Ensemble, "exchange_shape_info"), staticmethod)


@pytest.mark.parametrize("shape", [(8, 8, 8), (8, 2, 2048), (8, 50, 51), (64, 11, 29)])
def test_exchange_shape_is_the_moments_launch_s(sqlib, shape):
    from stochquant_amd import Phi4Ensemble
    got = Phi4Ensemble.exchange_shape_info(shape)
    ref = Phi4Ensemble.shape_info(shape)
    assert list(got) == ["K", "T", "lds_bytes", "lds_limit"]
    assert tuple(got.values()) == (ref["K"], ref["T"], ref["moments_lds_bytes"], 160 * 1024)
    sites = shape[0] * shape[1] * shape[2]
    assert got["lds_bytes"] == 4 * sites + 16 * 4 * 8 + 16 * 4 <= got["lds_limit"]      # one image and the scratch


def test_exchange_shape_info_refuses_what_create_refuses(sqlib):
    from stochquant_amd import Phi4Ensemble, StochQuantError
    for shape in ((12, 8, 8), (8, 1, 8), (8, 8, 1), (64, 32, 32), (8, 2, 2049), (4, 8, 8)):
        with pytest.raises(StochQuantError):
            Phi4Ensemble.exchange_shape_info(shape)
        with pytest.raises(StochQuantError):
            Phi4Ensemble.shape_info(shape)


def test_shape_queries_keep_the_parents_values(sqlib):
    """Two rows of the parent's values, written out (test_phi4_ens_hmc_boundary.py has the rest)."""
    from stochquant_amd import Phi4Ensemble
    LDS = 160 * 1024
    assert tuple(Phi4Ensemble.shape_info((8, 2, 2048)).values()) == (8, 1024, 1, 131648, 1, 131696, 131648, LDS)
    assert tuple(Phi4Ensemble.shape_info((8, 50, 51)).values()) == (8, 640, 2, 163776, 2, 163824, 82176, LDS)


def test_exchange_kernels_use_no_private_memory(sqlib):
    from stochquant_amd import isa_check
    md = isa_check.kernel_metadata(os.path.join(ROOT, "stochquant_amd", "lib", "libstochquant.so"))
    xk = {k: v for k, v in md.items() if "phi4_ens_exchange_kernel" in k}
    assert len(xk) >= 4, sorted(k for k in md if "phi4_ens" in k)
    for K in (1, 2, 4, 8):
        assert sum(f"phi4_ens_exchange_kernelILi{K}E" in k for k in xk) >= 1, (K, sorted(xk))
    bad = {k: v for k, v in xk.items() if v.get("private", 0) != 0 or v.get("vgpr_spill", 0) != 0}
    assert bad == {}, bad
