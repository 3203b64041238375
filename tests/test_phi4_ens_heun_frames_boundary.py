"""The phi^4 ensemble's Heun frames without a GPU: the library exports
sq_phi4_ens_run_frames_heun and sq_phi4_ens_heun_frames_shape_info and
_lib.SIGNATURES binds them, the ABI version stays 6, arguments are checked
before any device work, Phi4Ensemble.run_frames / run_frame carry `scheme` and
refuse an unknown one before any library call, the shape report gives every
legal shape the frames launch's image count and bytes and refuses exactly what
sq_phi4_ens_shape_info refuses, and every instance of the resident Heun frames
kernel exists and uses neither private memory nor a spilled register."""
import ctypes
import inspect
import os

import pytest

from test_phi4_ens_shapes import FRAME_SCRATCH, LDS_LIMIT, legal_shapes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_heun_frames(sqlib):
    from stochquant_amd import _lib
    for name, nargs in (("sq_phi4_ens_run_frames_heun", 6), ("sq_phi4_ens_heun_frames_shape_info", 2)):
        assert hasattr(sqlib, name)
        assert name in _lib.SIGNATURES
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs
    assert _lib.SIGNATURES["sq_phi4_ens_run_frames_heun"][1] == \
        _lib.SIGNATURES["sq_phi4_ens_run_frames_pcorr"][1]            # the same argument list, `measure` last


def test_abi_version_is_still_6(sqlib):
    from stochquant_amd import _lib
    assert sqlib.sq_abi_version() == _lib.ABI_VERSION == 6


def test_null_handle_and_bad_measure_bits_are_argument_errors(sqlib):
    st = (ctypes.c_int * 4)()
    dt = (ctypes.c_double * 4)()
    for nframes, measure in ((1, 0), (0, 0), (2, 1), (2, 3), (1, 4), (1, -1), (0, 8)):
        assert sqlib.sq_phi4_ens_run_frames_heun(None, nframes, st, dt, None, measure) == -1
        assert sqlib.sq_last_error().decode() != ""


def _bare():
    from stochquant_amd import Phi4Ensemble
    E = Phi4Ensemble.__new__(Phi4Ensemble)      # no handle: a library call would fail differently
    E._h = ctypes.c_void_p()
    E.R = 2
    return E


def test_unknown_scheme_raises_before_any_library_call(sqlib):
    E = _bare()
    for scheme in ("rk4", "", None, "Heun", 1):
        with pytest.raises(ValueError):
            E.run_frames(2, scheme=scheme)
        with pytest.raises(ValueError):
            E.run_frame(scheme=scheme)


def test_run_frames_signature_has_scheme(sqlib):
    from stochquant_amd import Phi4Ensemble
    sig = inspect.signature(Phi4Ensemble.run_frames).parameters
    assert list(sig) == ["self", "n", "measure", "correlate", "momenta", "scheme"]
    assert sig["scheme"].default == "euler"
    assert (sig["measure"].default, sig["correlate"].default, sig["momenta"].default) == (False, False, False)
    one = inspect.signature(Phi4Ensemble.run_frame).parameters
    assert list(one) == ["self", "scheme"] and one["scheme"].default == "euler"


def test_shape_report_over_every_legal_shape(sqlib):
    """{images, LDS bytes} are the frames launch's (two images exactly when they fit beside the frame scratch);
    every `measure` value runs unless the shape cannot hold momenta, which then lacks values 2 and 3."""
    from stochquant_amd import Phi4Ensemble
    dims = (ctypes.c_int * 3)()
    o4, o8, o6 = (ctypes.c_int * 4)(), (ctypes.c_int * 8)(), (ctypes.c_int * 6)()
    n = masks = 0
    for Lx, Ly, Lz in legal_shapes():
        sites = Lx * Ly * Lz
        dims[0], dims[1], dims[2] = Lx, Ly, Lz
        assert sqlib.sq_phi4_ens_heun_frames_shape_info(dims, o4) == 0
        assert sqlib.sq_phi4_ens_shape_info(dims, o8) == 0
        two = 2 * 4 * sites + FRAME_SCRATCH <= LDS_LIMIT
        assert (o4[0], o4[1]) == (o8[4], o8[5]) == ((2 if two else 1), (2 if two else 1) * 4 * sites + FRAME_SCRATCH), \
            (Lx, Ly, Lz)
        momenta = sqlib.sq_phi4_ens_pcorr_shape_info(dims, o6) == 0
        assert o4[2] == (0xf if momenta else 0x3) and o4[3] == 0, (Lx, Ly, Lz, tuple(o4))
        masks += 0 if momenta else 1
        n += 1
    assert n == 45843 and masks > 0
    assert Phi4Ensemble.heun_frames_shape_info((8, 8, 8)) == {"images": 2, "lds_bytes": 4720, "measure_mask": 15}
    assert Phi4Ensemble.heun_frames_shape_info((8, 2, 2048)) == {"images": 1, "lds_bytes": 131696, "measure_mask": 3}


@pytest.mark.parametrize("shape", [(4, 8, 8), (12, 8, 8), (128, 8, 8), (0, 8, 8), (-8, 8, 8), (8, 1, 8), (8, 8, 1),
                                   (8, 0, 8), (8, 8, -2), (8, 17, 241), (8, 2, 2049), (16, 2, 1025), (32, 32, 33),
                                   (64, 2, 257), (8, 65536, 65536), (64, 32768, 32768)])
def test_shape_report_refuses_what_shape_info_refuses(sqlib, shape):
    from stochquant_amd import Phi4Ensemble, StochQuantError
    dims = (ctypes.c_int * 3)(*shape)
    assert sqlib.sq_phi4_ens_shape_info(dims, (ctypes.c_int * 8)()) == -1
    assert sqlib.sq_phi4_ens_heun_frames_shape_info(dims, (ctypes.c_int * 4)()) == -1
    assert sqlib.sq_last_error().decode() != ""
    with pytest.raises(StochQuantError) as ei:
        Phi4Ensemble.heun_frames_shape_info(shape)
    assert ei.value.code == -1
    assert sqlib.sq_phi4_ens_heun_frames_shape_info(None, (ctypes.c_int * 4)()) == -1
    assert sqlib.sq_phi4_ens_heun_frames_shape_info((ctypes.c_int * 3)(8, 8, 8), None) == -1


def test_heun_frames_kernels_exist_and_use_no_private_memory(sqlib):
    """K = 1, 2, 4, 8 x plain, correlator, momenta x one and two images: 24 instances, no combination refused for
    want of registers."""
    from stochquant_amd import isa_check
    md = isa_check.kernel_metadata(os.path.join(ROOT, "stochquant_amd", "lib", "libstochquant.so"))
    fr = {k: v for k, v in md.items() if "phi4_ens_heun_frames_kernel" in k}
    assert len(fr) >= 24, sorted(k for k in md if "phi4_ens" in k)
    assert not any("phi4_ens_frames_kernel" in k or "phi4_ens_heun_kernel" in k for k in fr)
    bad = {k: v for k, v in fr.items() if v.get("private", 0) != 0 or v.get("vgpr_spill", 0) != 0}
    assert bad == {}, bad
