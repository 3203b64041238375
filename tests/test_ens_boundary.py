"""The replica ensemble's boundary without a GPU: libstochquant.so exports every
sq_ens_* symbol, sq_ens_create checks its arguments before it looks for a
device (SQ_E_ARG with a message), valid arguments without a device give
SQ_E_NODEV (no CPU fallback), and the ABI version stays 6."""
import ctypes

import pytest

ENS_SYMBOLS = ["sq_ens_create", "sq_ens_destroy", "sq_ens_upload", "sq_ens_download", "sq_ens_get_scan",
               "sq_ens_set_scan", "sq_ens_get_dtau", "sq_ens_set_dtau", "sq_ens_run_frames", "sq_ens_correlator",
               "sq_ens_perf"]


def _create(sqlib, nrep=4, **kw):
    from stochquant_amd import _lib
    p = _lib.default_params()
    p.dims[0] = 100
    p.deltat = 0.1
    p.loops = 10
    for k, v in kw.items():
        if k == "N":
            p.dims[0] = v
        else:
            setattr(p, k, v)
    h = ctypes.c_void_p()
    rc = sqlib.sq_ens_create(ctypes.byref(p), nrep, None, ctypes.byref(h))
    msg = sqlib.sq_last_error().decode()
    if rc == 0:
        assert sqlib.sq_ens_destroy(h) == 0
    return rc, msg


def test_library_exports_every_ensemble_symbol(sqlib):
    from stochquant_amd import _lib
    assert [s for s in ENS_SYMBOLS if not hasattr(sqlib, s)] == []
    assert [s for s in ENS_SYMBOLS if s not in _lib.SIGNATURES] == []


@pytest.mark.parametrize("kw", [dict(model=1), dict(N=1), dict(N=4097), dict(pot=1), dict(pot=2), dict(nrep=0),
                                dict(nrep=-3), dict(loops=0), dict(struct_size=8)],
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
    assert sqlib.sq_ens_create(None, 2, None, ctypes.byref(h)) == -1
    assert sqlib.sq_ens_create(ctypes.byref(p), 2, None, None) == -1
    assert sqlib.sq_ens_destroy(None) == 0
    assert sqlib.sq_ens_run_frames(None, 1, None) == -1


def test_no_device_no_fallback(sqlib):
    """Valid arguments: SQ_E_NODEV without a device, and the Python class raises."""
    from stochquant_amd import Qm1dEnsemble, StochQuantError, _lib
    if _lib.device_count() > 0:
        with Qm1dEnsemble(100, 0.1, 0.002, 4, loops=10):   # a device: the same arguments create
            pass
        return
    rc, msg = _create(sqlib)
    assert rc == -5 and msg != ""
    with pytest.raises(StochQuantError) as ei:
        Qm1dEnsemble(100, 0.1, 0.002, 4, loops=10)
    assert ei.value.code == -5


def test_abi_version_unchanged(sqlib):
    from stochquant_amd import _lib
    assert sqlib.sq_abi_version() == _lib.ABI_VERSION == 6
