"""The phi^4 ensemble's cluster sweep without a GPU: the library exports the calls and _lib.SIGNATURES binds them,
the ABI version stays 6, the header carries the definition and its limits, the stream constant is declared and
used, a null handle is an argument error, Phi4Ensemble raises its argument errors before any library call, the
sweep's launch reports the moments launch's work-group shape, the existing shape queries give what they gave, and
no instance of the cluster kernel uses private memory."""
import ctypes
import inspect
import os
import re

import pytest

from test_phi4_ens_heun_boundary import _bare

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"sq_phi4_ens_cluster": 4, "sq_phi4_ens_cluster_sweep": 2, "sq_phi4_ens_set_cluster_sweep": 2,
         "sq_phi4_ens_cluster_stats": 4, "sq_phi4_ens_cluster_reset": 3, "sq_phi4_ens_cluster_shape_info": 2,
         "sq_phi4_ens_step_hmc_cluster": 11}


def test_library_exports_the_cluster_calls(sqlib):
    from stochquant_amd import _lib
    for name, nargs in CALLS.items():
        assert hasattr(sqlib, name), name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs, name
    S = _lib.SIGNATURES
    a = S["sq_phi4_ens_cluster"][1]
    assert a[1] is ctypes.c_int and a[2]._type_ is ctypes.c_ubyte and a[3]._type_ is ctypes.c_int
    assert S["sq_phi4_ens_cluster_sweep"][1][1]._type_ is ctypes.c_ulonglong
    assert S["sq_phi4_ens_set_cluster_sweep"][1][1] is ctypes.c_ulonglong
    assert S["sq_phi4_ens_cluster_stats"][1][1:3] == [ctypes.c_int] * 2
    assert S["sq_phi4_ens_cluster_stats"][1][3]._type_ is ctypes.c_longlong
    assert S["sq_phi4_ens_cluster_reset"][1][1:] == [ctypes.c_int] * 2
    assert [t._type_ for t in S["sq_phi4_ens_cluster_shape_info"][1]] == [ctypes.c_int] * 2
    a = S["sq_phi4_ens_step_hmc_cluster"][1]
    assert a[1:6] == [ctypes.c_int] * 5 and a[7] is ctypes.c_int
    assert a[6] is a[8] and a[6]._type_ is ctypes.c_double
    assert a[9]._type_ is ctypes.c_ubyte and a[10]._type_ is ctypes.c_int


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
    for word in ("Swendsen-Wang", "Brower and Tamayo", "beta = 2 h / (sig sig)", "i = (z Ly + y) Lx + x",
                 "{i, 5 << 24, c lo, c hi}", "three forward bonds", "separate bonds with", "separate uniforms",
                 "u_mu = (word mu of o_i + 0.5) 2^-32", "u_mu >= exp(-(2 beta) t)", "t > 0", "A NaN t",
                 "smallest site index", "word 3 of o_l is odd", "sign bit toggled", "NaN payloads",
                 "c advances by one per sweep", "unconverged sweeps", "sites + 1", "SQ_E_STATE",
                 "exact only as one of the moves of an", "not ergodic", "|phi| is frozen", "ntraj % every == 0",
                 "before the\n * round's sweep"):
        assert word in h, word


def test_the_cluster_stream_is_declared_beside_the_exchange_stream():
    with open(os.path.join(ROOT, "stochquant_amd", "csrc", "sq_phi4_ens.h")) as fh:
        h = fh.read()
    assert re.search(r"constexpr uint32_t kPhi4EnsStreamCluster = 5;", h)
    assert h.index("kPhi4EnsStreamExchange = 4") < h.index("kPhi4EnsStreamCluster = 5")
    with open(os.path.join(ROOT, "stochquant_amd", "csrc", "sq_phi4_ens_cluster_dev.h")) as fh:
        k = fh.read()
    assert "kPhi4EnsStreamCluster << 24" in k and '#include "sq_phi4_ens_dev.h"' in k
    with open(os.path.join(ROOT, "stochquant_amd", "csrc", "sq_phi4_ens_cluster.hip")) as fh:
        assert '#include "sq_phi4_ens_cluster_dev.h"' in fh.read()
    import phi4_cluster_model as cm
    assert cm.STREAM_CLUSTER == 5


def test_the_source_is_in_the_build_list():
    from stochquant_amd import build
    assert "sq_phi4_ens_cluster.hip" in build.DEVICE_SOURCES
    # the kernel's own file, then exactly what the exchange unit depends on
    assert build.INCLUDES["sq_phi4_ens_cluster.hip"] == \
        ["sq_phi4_ens_cluster_dev.h"] + build.INCLUDES["sq_phi4_ens_exchange.hip"]
    assert "sq_phi4_ens_cluster_dev.h" not in build.INCLUDES["sq_phi4_ens_exchange.hip"]


def test_null_handle_is_an_argument_error(sqlib):
    c = ctypes.c_ulonglong(0)
    st = (ctypes.c_longlong * 5)()
    for call in (lambda: sqlib.sq_phi4_ens_cluster(None, 1, None, None),
                 lambda: sqlib.sq_phi4_ens_cluster(None, 0, None, None),
                 lambda: sqlib.sq_phi4_ens_cluster_sweep(None, ctypes.byref(c)),
                 lambda: sqlib.sq_phi4_ens_set_cluster_sweep(None, 7),
                 lambda: sqlib.sq_phi4_ens_cluster_stats(None, 0, 1, st),
                 lambda: sqlib.sq_phi4_ens_cluster_reset(None, 0, 1),
                 lambda: sqlib.sq_phi4_ens_step_hmc_cluster(None, 2, 2, 3, 1, 1, None, 1, None, None, None),
                 lambda: sqlib.sq_phi4_ens_step_hmc_cluster(None, 0, 0, 1, 0, 0, None, 0, None, None, None)):
        assert call() == -1
        assert sqlib.sq_last_error().decode() != ""
    assert sqlib.sq_phi4_ens_cluster_shape_info(None, None) == -1
    assert sqlib.sq_last_error().decode() != ""


def test_python_errors_are_raised_before_any_library_call(sqlib):
    E = _bare()                                  # no handle: a library call would raise StochQuantError
    for bad in (lambda: E.step_hmc_cluster(4, nleap=0),
                lambda: E.step_hmc_cluster(4, ntraj=2, nleap=4097, randomize=True),
                lambda: E.step_hmc_cluster(4, ntraj=2, nleap=3, every=0, correlate=True),
                lambda: E.step_hmc_cluster(4, ntraj=2, nleap=3, every=-1, correlate=True),
                lambda: E.step_hmc_cluster(4, ntraj=3, nleap=3, every=2),
                lambda: E.step_hmc_cluster(4, ntraj=1, nleap=1, every=2, correlate=True)):
        with pytest.raises(ValueError, match="step_hmc_cluster"):
            bad()


def test_python_signatures(sqlib):
    from stochquant_amd import Phi4Ensemble
    sig = inspect.signature(Phi4Ensemble.step_hmc_cluster).parameters
    assert list(sig) == ["self", "rounds", "ntraj", "nleap", "randomize", "every", "correlate", "record"]
    assert [sig[k].default for k in list(sig)[2:]] == [1, 1, False, 0, False, False]
    sig = inspect.signature(Phi4Ensemble.cluster).parameters
    assert list(sig) == ["self", "sweeps", "record"] and [sig[k].default for k in list(sig)[1:]] == [1, False]
    for name in ("cluster_stats", "cluster_reset"):
        sig = inspect.signature(getattr(Phi4Ensemble, name)).parameters
        assert list(sig) == ["self", "first", "count"] and sig["first"].default == 0 and sig["count"].default is None
    assert isinstance(Phi4Ensemble.cluster_sweep, property) and Phi4Ensemble.cluster_sweep.fset is not None
    assert isinstance(inspect.getattr_static(Phi4Ensemble, "cluster_shape_info"), staticmethod)


@pytest.mark.parametrize("shape", [(8, 2, 2), (8, 8, 8), (8, 2, 2048), (8, 50, 51), (64, 11, 29), (32, 32, 32)])
def test_cluster_shape_is_the_moments_launch_s(sqlib, shape):
    from stochquant_amd import Phi4Ensemble
    got = Phi4Ensemble.cluster_shape_info(shape)
    ref = Phi4Ensemble.shape_info(shape)
    assert list(got) == ["K", "T", "lds_bytes", "lds_limit"]
    assert tuple(got.values()) == (ref["K"], ref["T"], ref["moments_lds_bytes"], 160 * 1024)
    sites = shape[0] * shape[1] * shape[2]
    assert got["lds_bytes"] == 4 * sites + 16 * 4 * 8 + 16 * 4 <= got["lds_limit"]      # one image and the scratch


def test_cluster_shape_info_refuses_what_create_refuses(sqlib):
    from stochquant_amd import Phi4Ensemble, StochQuantError
    for shape in ((12, 8, 8), (8, 1, 8), (8, 8, 1), (64, 32, 32), (8, 2, 2049), (4, 8, 8)):
        with pytest.raises(StochQuantError):
            Phi4Ensemble.cluster_shape_info(shape)
        with pytest.raises(StochQuantError):
            Phi4Ensemble.shape_info(shape)


def test_shape_queries_keep_the_parents_values(sqlib):
    """Two rows of the parent's values, written out (test_phi4_ens_hmc_boundary.py has the rest)."""
    from stochquant_amd import Phi4Ensemble
    LDS = 160 * 1024
    assert tuple(Phi4Ensemble.shape_info((8, 2, 2048)).values()) == (8, 1024, 1, 131648, 1, 131696, 131648, LDS)
    assert tuple(Phi4Ensemble.shape_info((8, 50, 51)).values()) == (8, 640, 2, 163776, 2, 163824, 82176, LDS)
    assert tuple(Phi4Ensemble.exchange_shape_info((8, 50, 51)).values()) == (8, 640, 82176, LDS)


def test_cluster_kernels_use_no_private_memory(sqlib):
    from stochquant_amd import isa_check
    md = isa_check.kernel_metadata(os.path.join(ROOT, "stochquant_amd", "lib", "libstochquant.so"))
    ck = {k: v for k, v in md.items() if "phi4_ens_cluster_kernel" in k}
    assert len(ck) >= 4, sorted(k for k in md if "phi4_ens" in k)
    for K in (1, 2, 4, 8):
        assert sum(f"phi4_ens_cluster_kernelILi{K}E" in k for k in ck) >= 1, (K, sorted(ck))
    bad = {k: v for k, v in ck.items() if v.get("private", 0) != 0 or v.get("vgpr_spill", 0) != 0}
    assert bad == {}, bad
