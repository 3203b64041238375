"""The single lattice's in-stream measurement entry points at the library boundary (CPU only): exported,
prototyped, refusing a null context before anything touches a device, and sq_phi4_measure_shape_info for the
shapes test_gpu_phi4_measure.py runs."""
import ctypes

import pytest

from stochquant_amd import Phi4Lattice, StochQuantError, _lib

NAMES = ("sq_phi4_set_momenta", "sq_phi4_get_momenta", "sq_phi4_measure", "sq_phi4_step_hmc_meas",
         "sq_phi4_step_hmc_cluster_meas", "sq_phi4_corr_sums", "sq_phi4_corr_reset", "sq_phi4_measure_shape_info")
SHAPES = [(8, 2, 2), (16, 4, 1), (64, 11, 29), (256, 4, 6), (512, 2, 5), (768, 3, 4), (256, 16, 16)]


def test_the_symbols_are_exported_and_prototyped(sqlib):
    for name in NAMES:
        assert name in _lib.SIGNATURES and not name.startswith("sq_phi4_ens_"), name
        fn = getattr(sqlib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(_lib.SIGNATURES[name][1])
    assert sqlib.sq_abi_version() == 6


def test_a_null_context_is_an_argument_error(sqlib):
    m = ctypes.c_int()
    for rc in (sqlib.sq_phi4_set_momenta(None, 0, None), sqlib.sq_phi4_get_momenta(None, ctypes.byref(m), None),
               sqlib.sq_phi4_measure(None, None, None, None, None, None),
               sqlib.sq_phi4_step_hmc_meas(None, 1, 1, 0, 1, None, 0, None),
               sqlib.sq_phi4_step_hmc_cluster_meas(None, 1, 1, 1, 0, 1, None, 0, None, None, None),
               sqlib.sq_phi4_corr_sums(None, None, None, None, None, None), sqlib.sq_phi4_corr_reset(None),
               sqlib.sq_phi4_measure_shape_info(None, 0, None)):
        assert rc == -1
        assert sqlib.sq_last_error().decode() != ""


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("M", [0, 4, 8])
def test_shape_info(sqlib, shape, M):
    info = Phi4Lattice.measure_shape_info(shape, M)
    Lx, Ly, Lz = shape
    # a wave's unit holds at most 64 lanes x 4 rows x 2 quads of 4 sites: the units of a plane cover it
    assert info["units_per_plane"] >= 1 and info["units_per_plane"] * 2048 >= Lx * Ly
    assert info["partial_bytes"] == Lz * info["units_per_plane"] * (1 + 2 * M) * 8
    assert info["lds"] == (16 if M else 8) * Lz <= 64 * 1024
    assert info["nt"] == Lz // 2 + 1


@pytest.mark.parametrize("shape,M", [((12, 4, 4), 0), ((0, 4, 4), 0), ((8, 4, 0), 0), ((8, 2, 2), 9), ((8, 2, 2), -1)])
def test_an_illegal_shape_or_count_is_refused(sqlib, shape, M):
    with pytest.raises(StochQuantError) as ei:
        Phi4Lattice.measure_shape_info(shape, M)
    assert ei.value.code == -1
