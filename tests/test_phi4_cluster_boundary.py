"""The single lattice's cluster-sweep entry points at the library boundary (CPU only): exported, prototyped,
refusing a null context before anything touches a device, and sq_phi4_cluster_shape_info's bricks for the shapes
test_gpu_phi4_cluster.py runs: they tile the lattice, the LDS request is inside the limit the ensemble's launch
path uses, and SQ_CLUSTER_TILE is taken or ignored as the header says."""
import ctypes

import pytest

from stochquant_amd import Phi4Lattice, StochQuantError, _lib

NAMES = ("sq_phi4_cluster", "sq_phi4_step_hmc_cluster", "sq_phi4_cluster_stats", "sq_phi4_cluster_reset",
         "sq_phi4_cluster_sweep", "sq_phi4_set_cluster_sweep", "sq_phi4_cluster_shape_info")
# (shape, SQ_CLUSTER_TILE or None): the cases of test_gpu_phi4_cluster.py's model test
CASES = [((8, 2, 2), None), ((16, 4, 1), None), ((64, 11, 29), None), ((256, 4, 6), None), ((512, 2, 5), None),
         ((768, 3, 4), None), ((16, 6, 5), "8,4,2"), ((64, 32, 17), None)]


def test_the_symbols_are_exported_and_prototyped(sqlib):
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        fn = getattr(sqlib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(_lib.SIGNATURES[name][1])
    assert sqlib.sq_abi_version() == 6


def test_a_null_context_is_an_argument_error(sqlib):
    out, c = (ctypes.c_longlong * 5)(), ctypes.c_ulonglong()
    for rc in (sqlib.sq_phi4_cluster(None, 1, None, None), sqlib.sq_phi4_step_hmc_cluster(None, 1, 1, 1, 0, None, None, None),
               sqlib.sq_phi4_cluster_stats(None, out), sqlib.sq_phi4_cluster_reset(None),
               sqlib.sq_phi4_cluster_sweep(None, ctypes.byref(c)), sqlib.sq_phi4_set_cluster_sweep(None, 1),
               sqlib.sq_phi4_cluster_shape_info(None, None)):
        assert rc == -1
        assert sqlib.sq_last_error().decode() != ""


@pytest.mark.parametrize("shape,tile", CASES)
def test_bricks_tile_the_lattice_inside_the_lds_limit(sqlib, monkeypatch, shape, tile):
    if tile:
        monkeypatch.setenv("SQ_CLUSTER_TILE", tile)
    info = Phi4Lattice.cluster_shape_info(shape)
    t, n = info["tile"], info["tiles"]
    if tile:
        assert t == tuple(int(v) for v in tile.split(","))
    assert t[0] in (8, 16, 32, 64, 128, 256) and shape[0] % t[0] == 0 and n[0] * t[0] == shape[0]
    for ax in (1, 2):
        assert 1 <= t[ax] <= shape[ax] and (n[ax] - 1) * t[ax] < shape[ax] <= n[ax] * t[ax]
    ens = (ctypes.c_int * 4)()
    assert sqlib.sq_phi4_ens_cluster_shape_info((ctypes.c_int * 3)(8, 8, 8), ens) == 0
    assert 5 * t[0] * t[1] * t[2] <= info["lds"] <= ens[3]
    assert info["bytes_per_site"] == 5


def test_a_default_case_has_seams_in_y_and_z_and_a_partial_brick(sqlib, monkeypatch):
    monkeypatch.delenv("SQ_CLUSTER_TILE", raising=False)
    hit = []
    for shape, tile in CASES:
        info = Phi4Lattice.cluster_shape_info(shape)
        t, n = info["tile"], info["tiles"]
        if tile is None and n[1] >= 2 and n[2] >= 2 and (shape[1] % t[1] or shape[2] % t[2]):
            hit.append(shape)
    assert hit, "no default-tiled case crosses a seam in y and in z with a partial brick"


@pytest.mark.parametrize("tile", ["4,4,4", "12,2,2", "32,2,2", "8,0,2", "8,2,-1", "8,2", "8,2,2,2", "8,2,2x", "256,8,8",
                                  "16,64,64", ""])
def test_an_illegal_override_is_ignored(sqlib, monkeypatch, tile):
    shape = (16, 64, 64)    # 32 does not divide Lx; 16 x 64 x 64 is more than a brick holds
    monkeypatch.delenv("SQ_CLUSTER_TILE", raising=False)
    default = Phi4Lattice.cluster_shape_info(shape)
    monkeypatch.setenv("SQ_CLUSTER_TILE", tile)
    assert Phi4Lattice.cluster_shape_info(shape) == default
    monkeypatch.setenv("SQ_CLUSTER_TILE", "8,100,3")       # ty is cut to Ly
    assert Phi4Lattice.cluster_shape_info(shape)["tile"] == (8, 64, 3)


@pytest.mark.parametrize("shape", [(12, 4, 4), (0, 4, 4), (8, 4, 0), (8, -1, 4), (1024, 1024, 2048)])
def test_an_illegal_shape_is_refused(sqlib, shape):
    with pytest.raises(StochQuantError) as ei:
        Phi4Lattice.cluster_shape_info(shape)
    assert ei.value.code == -1
