"""The cluster sums of the phi^4 ensemble's sweep without a GPU: the library exports the calls and _lib.SIGNATURES
binds them, the ABI version stays 6, the header carries the definition, a null handle is an argument error before any
device work, Phi4Ensemble raises its argument errors before any library call, `cluster` and `step_hmc_cluster` keep
their signatures and return shapes, the shape query works for every legal shape and refuses the illegal ones, the new
source is in the build list, and no instance of the kernel uses private memory."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from test_phi4_ens_heun_boundary import _bare
from test_phi4_ens_shapes import LDS_LIMIT, SCRATCH, legal_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {"sq_phi4_ensemble_cluster_improved": 6, "sq_phi4_ensemble_step_hmc_cluster_improved": 13,
         "sq_phi4_ensemble_cluster_improved_shape_info": 2}


def test_library_exports_the_calls(sqlib):
    from stochquant_amd import _lib
    for name, nargs in CALLS.items():
        assert hasattr(sqlib, name), name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs, name
    S = _lib.SIGNATURES
    a = S["sq_phi4_ensemble_cluster_improved"][1]
    assert a[1] is ctypes.c_int and a[2]._type_ is ctypes.c_double and a[3]._type_ is ctypes.c_ubyte
    assert a[4]._type_ is ctypes.c_int and a[5]._type_ is ctypes.c_longlong
    a, plain = S["sq_phi4_ensemble_step_hmc_cluster_improved"][1], S["sq_phi4_ens_step_hmc_cluster"][1]
    assert a[:11] == plain and a[11]._type_ is ctypes.c_double and a[12]._type_ is ctypes.c_longlong
    assert [t._type_ for t in S["sq_phi4_ensemble_cluster_improved_shape_info"][1]] == [ctypes.c_int] * 2


def test_abi_version_is_still_6(sqlib):
    from stochquant_amd import _lib
    assert sqlib.sq_abi_version() == _lib.ABI_VERSION == 6


def test_header_carries_the_definition():
    with open(os.path.join(ROOT, "include", "stochquant.h")) as fh:
        h = fh.read()
    for name in CALLS:
        first = r"const\s+int\s+dims\[3\]" if name.endswith("shape_info") else r"sq_phi4_ens\s*\*"
        assert re.search(r"\bint\s+" + name + r"\s*\(\s*" + first, h), name
        assert len(re.findall(r"\b" + name + r"\b", h)) >= 2, name
    for word in ("<(sum phi)^2> = <sum_C M_C^2>", "3 (sum_C M_C^2)^2 - 2 sum_C M_C^4", "q_i = floor(a 2^32)",
                 "rint((a c[k]) 2^32), ties to even", "sq_phi4_ens_momentum_table(L_mu, 1)", ">= 2^15", "saturated",
                 "|sum| < 2^62", "I2 = sum_C m_C^2", "Mmax = max_C m_C", "nsat = -1", "n_clusters 2^-52",
                 "bit for bit those of the plain call", "M, A_x, B_x, A_y, B_y, A_z,", "SQ_E_STATE"):
        assert word in h, word
    assert h.index("int sq_phi4_ens_step_hmc_cluster(") < h.index("int sq_phi4_ensemble_cluster_improved(")


def test_the_source_is_in_the_build_list():
    from stochquant_amd import build
    assert "sq_phi4_ens_cluster_improved.hip" in build.DEVICE_SOURCES
    # the cluster kernel's file and everything the cluster unit depends on: the two units' lists are one
    assert build.INCLUDES["sq_phi4_ens_cluster_improved.hip"] == build.INCLUDES["sq_phi4_ens_cluster.hip"]
    assert build.INCLUDES["sq_phi4_ens_cluster_improved.hip"][0] == "sq_phi4_ens_cluster_dev.h"
    with open(os.path.join(ROOT, "stochquant_amd", "csrc", "sq_phi4_ens_cluster_improved.hip")) as fh:
        k = fh.read()
    assert '#include "sq_phi4_ens_cluster_dev.h"' in k and "KERNEL_ONLY" not in k
    with open(os.path.join(ROOT, "stochquant_amd", "csrc", "sq_phi4_ens_cluster_dev.h")) as fh:
        assert "phi4_ens_cluster_kernel(" in fh.read()


def test_null_handle_and_arguments_come_before_any_device_work(sqlib):
    ser = (ctypes.c_double * 8)()
    for call in (lambda: sqlib.sq_phi4_ensemble_cluster_improved(None, 1, ser, None, None, None),
                 lambda: sqlib.sq_phi4_ensemble_cluster_improved(None, 0, None, None, None, None),
                 lambda: sqlib.sq_phi4_ensemble_step_hmc_cluster_improved(None, 2, 2, 3, 1, 1, None, 1, None, None, None,
                                                                     ser, None),
                 lambda: sqlib.sq_phi4_ensemble_step_hmc_cluster_improved(None, 0, 0, 1, 0, 0, None, 0, None, None, None,
                                                                     None, None)):
        assert call() == -1
        assert sqlib.sq_last_error().decode() != ""
    out = (ctypes.c_int * 5)()
    assert sqlib.sq_phi4_ensemble_cluster_improved_shape_info(None, None) == -1
    assert sqlib.sq_phi4_ensemble_cluster_improved_shape_info((ctypes.c_int * 3)(8, 8, 8), None) == -1
    assert sqlib.sq_phi4_ensemble_cluster_improved_shape_info(None, out) == -1
    assert sqlib.sq_last_error().decode() != ""


def test_python_errors_are_raised_before_any_library_call(sqlib):
    E = _bare()                                  # no handle: a library call would raise StochQuantError
    for bad in (lambda: E.step_hmc_cluster_improved(4, nleap=0),
                lambda: E.step_hmc_cluster_improved(4, ntraj=2, nleap=4097, randomize=True),
                lambda: E.step_hmc_cluster_improved(4, ntraj=2, nleap=3, every=0, correlate=True),
                lambda: E.step_hmc_cluster_improved(4, ntraj=3, nleap=3, every=2)):
        with pytest.raises(ValueError, match="step_hmc_cluster_improved"):
            bad()


def test_python_signatures(sqlib):
    """The plain calls keep their signatures, so their defaults return what they returned; the calls with the sums
    repeat them."""
    from stochquant_amd import Phi4Ensemble
    sig = inspect.signature(Phi4Ensemble.cluster).parameters
    assert list(sig) == ["self", "sweeps", "record"] and [sig[k].default for k in list(sig)[1:]] == [1, False]
    assert list(inspect.signature(Phi4Ensemble.cluster_improved).parameters) == list(sig)
    sig = inspect.signature(Phi4Ensemble.step_hmc_cluster).parameters
    assert list(sig) == ["self", "rounds", "ntraj", "nleap", "randomize", "every", "correlate", "record"]
    imp = inspect.signature(Phi4Ensemble.step_hmc_cluster_improved).parameters
    assert list(imp) == list(sig) and [imp[k].default for k in imp] == [sig[k].default for k in sig]
    for name in ("cluster_improved_shape_info", "cluster_observables"):
        assert isinstance(inspect.getattr_static(Phi4Ensemble, name), staticmethod)


def test_every_legal_shape(sqlib):
    from stochquant_amd import Phi4Ensemble
    n = 0
    for shape in legal_shapes():
        if shape[1] > 6 and shape[1] % 7 and shape[2] % 5:      # a third of the 45,843: every Lx, every K, the edges
            continue
        n += 1
        got = Phi4Ensemble.cluster_improved_shape_info(shape)
        ref = Phi4Ensemble.cluster_shape_info(shape)
        sites = shape[0] * shape[1] * shape[2]
        assert list(got) == ["K", "T", "lds_bytes", "lds_limit", "park"]
        assert (got["K"], got["T"], got["lds_limit"]) == (ref["K"], ref["T"], LDS_LIMIT), shape
        assert got["lds_bytes"] == ref["lds_bytes"] + 32 == 4 * sites + SCRATCH + 32 <= LDS_LIMIT, shape
        assert got["park"] == (1 if got["K"] == 8 else 0), shape
    assert n > 10000
    for shape in ((8, 2, 2), (8, 2, 2048), (64, 256, 2), (32, 32, 32), (16, 32, 32), (64, 11, 29)):
        assert Phi4Ensemble.cluster_improved_shape_info(shape)["park"] == (shape[0] * shape[1] * shape[2] > 16384)


def test_shape_info_refuses_what_create_refuses(sqlib):
    from stochquant_amd import Phi4Ensemble, StochQuantError
    for shape in ((12, 8, 8), (8, 1, 8), (8, 8, 1), (64, 32, 32), (8, 2, 2049), (4, 8, 8)):
        with pytest.raises(StochQuantError) as ei:
            Phi4Ensemble.cluster_improved_shape_info(shape)
        assert ei.value.code == -1


def test_cluster_observables():
    """chi, the Binder cumulant and xi from a made-up series with known means."""
    from stochquant_amd import Phi4Ensemble
    shape, R, n = (8, 4, 4), 6, 5
    rng = np.random.default_rng(3)
    s = np.zeros((n, R, 8))
    s[:, :, 0] = 100.0 + rng.normal(size=(n, R))
    s[:, :, 1] = 50.0
    s[:, :, 2:5] = np.asarray([40.0, 20.0, 20.0]) + 0.1 * rng.normal(size=(n, R, 3))
    o = Phi4Ensemble.cluster_observables(s, shape)
    per = s[:, :, 0].mean(axis=0)
    assert o["chi"][0] == pytest.approx(per.mean() / 128.0) and \
        o["chi"][1] == pytest.approx(per.std(ddof=1) / np.sqrt(R) / 128.0)
    m4 = (3.0 * s[:, :, 0] ** 2 - 2.0 * s[:, :, 1]).mean()
    assert o["binder"][0] == pytest.approx(1.0 - m4 / (3.0 * s[:, :, 0].mean() ** 2)) and o["binder"][1] > 0
    want = [np.sqrt((s[:, :, 0].mean() / s[:, :, 2 + mu].mean() - 1.0) / (4.0 * np.sin(np.pi / L) ** 2))
            for mu, L in enumerate(shape)]
    assert [x[0] for x in o["xi"]] == pytest.approx(want) and all(x[1] > 0 for x in o["xi"])
    assert [x[0] for x in Phi4Ensemble.cluster_observables(s, shape, axis_mask=(0, 0, 1))["xi"]] == \
        pytest.approx(want[2:])
    s[0, 0, 7] = -1.0                      # an unconverged sweep is left out
    s[0, 0, :7] = 0.0
    assert Phi4Ensemble.cluster_observables(s, shape)["chi"][0] == pytest.approx(o["chi"][0], rel=0.01)
    for bad in (s[:, :1], s[:, :, :7], s[:0]):
        with pytest.raises(ValueError, match="cluster_observables"):
            Phi4Ensemble.cluster_observables(bad, shape)


def test_kernels_use_no_private_memory(sqlib):
    from stochquant_amd import isa_check
    md = isa_check.kernel_metadata(os.path.join(ROOT, "stochquant_amd", "lib", "libstochquant.so"))
    ck = {k: v for k, v in md.items() if "phi4_ens_cluster_kernel" in k}
    imp = {k: v for k, v in ck.items() if "Phi4EnsClusterSumArgs" in k}
    assert len(ck) >= 8 and len(imp) == 4, sorted(ck)
    for K in (1, 2, 4, 8):
        assert sum(f"phi4_ens_cluster_kernelILi{K}E" in k for k in imp) == 1, (K, sorted(imp))
    bad = {k: v for k, v in ck.items() if v.get("private", 0) != 0 or v.get("vgpr_spill", 0) != 0}
    assert bad == {}, bad
