"""The phi^4 ensemble correlator's boundary without a GPU: libstochquant.so
exports the new sq_phi4_ens_* symbols and _lib.SIGNATURES binds them, the ABI
version stays 6, a null handle is SQ_E_ARG in every call, the Python class
refuses correlate=True with every < 1 before it calls the library, and the
correlator launches' LDS requests (sq_phi4_ens_corr_shape_info, host only) stay
inside the 160 KiB limit over every legal shape."""
import ctypes

import pytest

CORR_SYMBOLS = ["sq_phi4_ens_step_corr", "sq_phi4_ens_run_frames_corr", "sq_phi4_ens_corr_sums",
                "sq_phi4_ens_corr_reset", "sq_phi4_ens_slices", "sq_phi4_ens_correlator"]
SCRATCH, FRAME_SCRATCH, LIMIT = 576, 624, 160 * 1024


def test_library_exports_the_correlator_symbols(sqlib):
    from stochquant_amd import _lib
    syms = CORR_SYMBOLS + ["sq_phi4_ens_corr_shape_info"]
    assert [s for s in syms if not hasattr(sqlib, s)] == []
    assert [s for s in syms if s not in _lib.SIGNATURES] == []


def test_abi_version_unchanged(sqlib):
    from stochquant_amd import _lib
    assert sqlib.sq_abi_version() == _lib.ABI_VERSION == 6


def test_null_handle_is_an_argument_error(sqlib):
    d = (ctypes.c_double * 4)()
    i = (ctypes.c_int * 4)()
    n = (ctypes.c_longlong * 4)()
    assert sqlib.sq_phi4_ens_step_corr(None, 4, 2, None) == -1
    assert sqlib.sq_phi4_ens_run_frames_corr(None, 1, i, d, None) == -1
    assert sqlib.sq_phi4_ens_corr_sums(None, 0, 1, d, d, n) == -1
    assert sqlib.sq_phi4_ens_corr_reset(None, 0, 1) == -1
    assert sqlib.sq_phi4_ens_slices(None, 0, 1, d, d) == -1
    assert sqlib.sq_phi4_ens_correlator(None, 1, d, d, 1, i) == -1
    assert sqlib.sq_last_error().decode() != ""
    assert sqlib.sq_phi4_ens_corr_shape_info(None, i) == -1


def test_correlate_needs_every_before_any_device_call(sqlib):
    from stochquant_amd import Phi4Ensemble
    E = Phi4Ensemble.__new__(Phi4Ensemble)      # no handle: a library call would fail differently
    E._h = ctypes.c_void_p()
    E.R = 2
    for every in (0, -1):
        with pytest.raises(ValueError):
            E.step(4, every=every, correlate=True)


def _legal_shapes():
    """Every Lx, with Ly and Lz at both ends and at each side of every site-count threshold of the shape rule."""
    out = set()
    for Lx in (8, 16, 32, 64):
        for Ly in (2, 3, 8, 16, 32, 50):
            top = 32768 // (Lx * Ly)
            if top < 2:
                continue
            cands = {2, 3, top, top - 1, max(2, top // 2), max(2, top // 2 + 1)}
            for sites in (4096, 8192, 16384, 20408, 20336):   # K thresholds, the two-image limits
                z = sites // (Lx * Ly)
                cands |= {z - 1, z, z + 1}
            out |= {(Lx, Ly, z) for z in cands if 2 <= z <= top}
    out.add((8, 2, 2048))
    return sorted(out)


def test_corr_shape_info_over_legal_shapes(sqlib):
    from stochquant_amd import Phi4Ensemble, StochQuantError
    seen_one_image_where_plain_has_two = False
    for shape in _legal_shapes():
        Lx, Ly, Lz = shape
        sites = Lx * Ly * Lz
        base = Phi4Ensemble.shape_info(shape)
        co = Phi4Ensemble.corr_shape_info(shape)
        assert co["nt"] == Lz // 2 + 1
        for images, lds, scratch in ((co["images"], co["lds_bytes"], SCRATCH),
                                     (co["frames_images"], co["frames_lds_bytes"], FRAME_SCRATCH)):
            assert images in (1, 2)
            assert lds == images * 4 * sites + scratch + 8 * Lz, shape
            assert lds <= LIMIT == base["lds_limit"], shape
            # two images exactly when they fit
            assert (images == 2) == (2 * 4 * sites + scratch + 8 * Lz <= LIMIT), shape
        assert co["slices_lds_bytes"] == 4 * sites + SCRATCH + 8 * Lz <= LIMIT
        # the slice sums sit behind the plain launch's layout and are 8-byte aligned
        assert co["lds_bytes"] - 8 * Lz == (co["images"] * 4 * sites + SCRATCH) and (co["lds_bytes"] - 8 * Lz) % 8 == 0
        assert co["images"] <= base["images"] and co["frames_images"] <= base["frames_images"]
        seen_one_image_where_plain_has_two |= co["images"] < base["images"]
    assert seen_one_image_where_plain_has_two
    assert Phi4Ensemble.corr_shape_info((8, 2, 2048))["lds_bytes"] == 128 * 1024 + 576 + 16 * 1024
    for bad in ((12, 8, 8), (8, 1, 8), (64, 32, 32)):
        with pytest.raises(StochQuantError) as ei:
            Phi4Ensemble.corr_shape_info(bad)
        assert ei.value.code == -1
