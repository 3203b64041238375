"""The phi^4 ensemble's boundary without a GPU: libstochquant.so exports every
sq_phi4_ens_* symbol, sq_phi4_ens_create checks its arguments before it looks
for a device (SQ_E_ARG with a message), valid arguments without a device give
SQ_E_NODEV (no CPU fallback), and the ABI version stays 6."""
import ctypes

import pytest

ENS_SYMBOLS = ["sq_phi4_ens_create", "sq_phi4_ens_destroy", "sq_phi4_ens_upload", "sq_phi4_ens_download",
               "sq_phi4_ens_init_field", "sq_phi4_ens_set_params", "sq_phi4_ens_get_params", "sq_phi4_ens_get_step",
               "sq_phi4_ens_set_step", "sq_phi4_ens_step", "sq_phi4_ens_moments", "sq_phi4_ens_flags",
               "sq_phi4_ens_perf", "sq_phi4_ens_shape_info"]


def _create(sqlib, nrep=4, shape=(8, 8, 8), **kw):
    from stochquant_amd import _lib
    p = _lib.default_params()
    p.model = _lib.SQ_MODEL_PHI4
    for i in range(3):
        p.dims[i] = shape[i]
    p.deltatau = 0.01
    p.m2 = 0.5
    p.lambda_ = 1.0
    for k, v in kw.items():
        setattr(p, k, v)
    h = ctypes.c_void_p()
    rc = sqlib.sq_phi4_ens_create(ctypes.byref(p), nrep, None, ctypes.byref(h))
    msg = sqlib.sq_last_error().decode()
    if rc == 0:
        assert sqlib.sq_phi4_ens_destroy(h) == 0
    return rc, msg


def test_library_exports_every_phi4_ensemble_symbol(sqlib):
    from stochquant_amd import _lib
    assert [s for s in ENS_SYMBOLS if not hasattr(sqlib, s)] == []
    assert [s for s in ENS_SYMBOLS if s not in _lib.SIGNATURES] == []


@pytest.mark.parametrize("kw", [dict(shape=(12, 8, 8)), dict(shape=(128, 8, 8)), dict(shape=(8, 1, 8)),
                                dict(shape=(8, 8, 1)), dict(shape=(64, 32, 32)), dict(model=0), dict(comm=1),
                                dict(comm=2), dict(nrep=0), dict(nrep=-3), dict(clamp=1e30), dict(struct_size=8)],
                         ids=lambda kw: "-".join(f"{k}{v}" for k, v in kw.items()))
def test_argument_errors_come_before_device_discovery(sqlib, kw):
    kw = dict(kw)
    nrep = kw.pop("nrep", 4)
    rc, msg = _create(sqlib, nrep=nrep, **kw)
    assert rc == -1       # SQ_E_ARG, with or without a device
    assert msg != ""


def test_null_arguments(sqlib):
    from stochquant_amd import _lib
    p = _lib.default_params()
    h = ctypes.c_void_p()
    assert sqlib.sq_phi4_ens_create(None, 2, None, ctypes.byref(h)) == -1
    assert sqlib.sq_phi4_ens_create(ctypes.byref(p), 2, None, None) == -1
    assert sqlib.sq_phi4_ens_destroy(None) == 0
    assert sqlib.sq_phi4_ens_step(None, 1, 0, None) == -1
    assert sqlib.sq_phi4_ens_flags(None, 0, 1, None, 0) == -1


def test_python_class_checks_per_replica_sequences(sqlib):
    from stochquant_amd import Phi4Ensemble
    with pytest.raises(ValueError):
        Phi4Ensemble((8, 8, 8), 4, dtau=[0.01, 0.02])
    with pytest.raises(ValueError):
        Phi4Ensemble((8, 8, 8), 4, seeds=[1, 2, 3])


def test_no_device_no_fallback(sqlib):
    """Valid arguments: SQ_E_NODEV without a device, and the Python class raises."""
    from stochquant_amd import Phi4Ensemble, StochQuantError, _lib
    if _lib.device_count() > 0:
        with Phi4Ensemble((8, 8, 8), 4, dtau=0.01, m2=0.5, lam=1.0, C=1.0):   # a device: the same arguments create
            pass
        return
    rc, msg = _create(sqlib)
    assert rc == -5 and msg != ""
    with pytest.raises(StochQuantError) as ei:
        Phi4Ensemble((8, 8, 8), 4, dtau=0.01, m2=0.5, lam=1.0, C=1.0)
    assert ei.value.code == -5


def test_abi_version_unchanged(sqlib):
    from stochquant_amd import _lib
    assert sqlib.sq_abi_version() == _lib.ABI_VERSION == 6
