"""Swendsen-Wang cluster sweeps of the single phi^4 lattice on the GPU (sq_phi4_cluster.hip, Phi4Lattice.cluster,
step_hmc_cluster) against the NumPy statement of the header's definition (phi4_cluster_model.py, whose fields and
seeds these are) and against a Phi4Ensemble of one replica.

Tolerances.  Bond bytes, labels, field bits, statistics and counters: exact.  A bond with |exp(-2 beta t) - u| <
1e-12 could not be decided across two exp implementations: the tests assert margin >= 1e-12 and fail if they meet
one (the smallest margin of these inputs is 1.7e-7)."""
import functools

import numpy as np
import pytest

import phi4_cluster_model as cm
from test_oracle import same_bits
from test_phi4_cluster_boundary import CASES

pytestmark = pytest.mark.gpu

M2, LAM = 0.5, 1.0
FORCED = ((16, 6, 5), "8,4,2")      # 2 x 2 x 3 bricks, partial in y and z


def _lat(shape, k=0, **kw):
    from stochquant_amd import Phi4Lattice
    kw.setdefault("C", cm.ORACLE_C[k])
    kw.setdefault("dtau", cm.ORACLE_DTAU)
    return Phi4Lattice(shape, m2=M2, lam=LAM, seed=cm.oracle_seeds(4)[k], **kw)


def _grid(shape, flat):
    return np.ascontiguousarray(flat).reshape(tuple(reversed(shape)))


@functools.lru_cache(maxsize=None)
def _model(shape):
    return cm.oracle_run(shape)


def _sweeps(phi, c0, n, seed, beta, shape):
    """The model's n sweeps of one lattice from counter c0: [(bits, labels, phi, stats, margin)]."""
    out = []
    for j in range(n):
        res = cm.sweep(phi[None], [beta], [seed], c0 + j, shape)
        phi = res["phi"][0]
        out.append((res["bits"][0], res["labels"][0], phi, res["stats"][0], res["margin"]))
    return out


def _check(A, c0, want, stats):
    """cluster(len(want), record=True) of lattice A from counter c0 against the model's sweeps `want`; adds to stats."""
    n, sites = len(want), want[0][2].size
    A.cluster_sweep = c0
    bonds, labels = A.cluster(n, record=True)
    assert bonds.shape == labels.shape == (n, sites) and bonds.dtype == np.uint8 and labels.dtype == np.int32
    for j, (bits, lab, _, inc, margin) in enumerate(want):
        assert margin >= 1e-12, ("a bond within 1e-12 of a tie: another input, not another bound", margin)
        assert np.array_equal(bonds[j], bits), (A.shape, c0 + j, np.argwhere(bonds[j] != bits)[:8])
        assert np.array_equal(labels[j], lab), (A.shape, c0 + j, np.argwhere(labels[j] != lab)[:8])
        stats[0] += 1
        stats[1:4] += inc
    assert same_bits(A.download(), _grid(A.shape, want[-1][2])), "sign bits toggled exactly on the odd-rooted clusters"
    assert A.cluster_sweep == c0 + n and list(A.cluster_stats()) == list(stats), (A.cluster_stats(), stats)


@pytest.mark.parametrize("shape,tile", CASES)
def test_against_the_model(gpu, monkeypatch, shape, tile):
    if tile:
        monkeypatch.setenv("SQ_CLUSTER_TILE", tile)
    run = _model(shape)
    assert [c for c, _ in run] == [7, 8, 2 ** 40 + 5, 2 ** 40 + 6] and min(r["margin"] for _, r in run) >= 1e-12
    big = int(np.argmax(np.bincount(run[0][1]["labels"][1])))
    assert any(r["flip"][1][big] for _, r in run), "the percolating cluster flips in none of the checked sweeps"
    fields = cm.oracle_fields(shape)
    for k in range(4):
        with _lat(shape, k) as A:
            A.upload(_grid(shape, fields[k]))
            assert A.cluster_sweep == 0 and not A.cluster_stats().any()
            stats = np.zeros(5, dtype=np.int64)
            for i, c0 in enumerate(cm.ORACLE_SWEEPS):
                _check(A, c0, [(r["bits"][k], r["labels"][k], r["phi"][k], r["stats"][k], r["margin"])
                               for _, r in run[2 * i:2 * i + 2]], stats)
            assert A.step_counter == 0 and A.dtau == cm.ORACLE_DTAU and not A.hmc_stats().any()
    path = cm.serpentine(shape)
    assert (run[0][1]["labels"][3][path] == 0).all() and np.bincount(run[0][1]["labels"][1]).max() > len(fields[1]) // 2


def _thermal(shape, seed):
    """A thermalised field from a one-replica ensemble, which is left at sweep counter 3."""
    from stochquant_amd import Phi4Ensemble
    E = Phi4Ensemble(shape, 1, dtau=cm.ORACLE_DTAU, m2=M2, lam=LAM, C=[cm.ORACLE_C[0]], seeds=[seed])
    E.init_field(0.5)
    E.step(50)
    E.cluster_sweep = 3
    return E


@pytest.mark.parametrize("shape", [(8, 8, 8), (64, 11, 29), (32, 32, 32)])
def test_is_the_ensemble_replica(gpu, shape):
    seed = cm.oracle_seeds(4)[0]
    with _thermal(shape, seed) as E, _lat(shape) as A:
        A.upload(E.download()[0])
        A.cluster_sweep = 3
        be, le = E.cluster(3, record=True)
        ba, la = A.cluster(3, record=True)
        assert np.array_equal(ba, be[:, 0]) and np.array_equal(la, le[:, 0])
        assert same_bits(A.download(), E.download()[0])
        assert list(A.cluster_stats()[:4]) == list(E.cluster_stats()[0, :4]) and not A.cluster_stats()[4]
        assert A.cluster_stats()[3] > 0 and A.cluster_sweep == E.cluster_sweep == 6


def test_fused_call_is_the_loop(gpu, dev_oracle):
    from stochquant_amd import Phi4Lattice
    shape, seed = (64, 32, 17), cm.oracle_seeds(4)[0]
    dtau = round(0.4 / (64 * 32 * 17) ** 0.5, 5)        # test_gpu_phi4_hmc.py's rule
    assert min(Phi4Lattice.cluster_shape_info(shape)["tiles"]) >= 2
    with _lat(shape, dtau=dtau) as A, _lat(shape, dtau=dtau) as B:
        for X in (A, B):
            X.init_field(0.5)
            X.step(20)
        rh, bo, la = A.step_hmc_cluster(3, ntraj=2, nleap=3, record=True)
        assert rh.shape == (6, 4) and bo.shape == la.shape == (3, 64 * 32 * 17)
        parts = []
        for _ in range(3):
            r = B.step_hmc(2, nleap=3, record=True)
            parts.append((r,) + B.cluster(1, record=True))
        assert np.array_equal(rh.view(np.uint64), np.concatenate([p[0] for p in parts]).view(np.uint64))
        assert np.array_equal(bo, np.concatenate([p[1] for p in parts]))
        assert np.array_equal(la, np.concatenate([p[2] for p in parts]))
        with _lat(shape, dtau=dtau) as C:               # without records: the same field
            C.init_field(0.5)
            C.step(20)
            assert C.step_hmc_cluster(3, ntraj=2, nleap=3) is None
            assert same_bits(C.download(), A.download())
        for X in (A, B):
            assert list(X.hmc_stats()) == list(A.hmc_stats()) and list(X.cluster_stats()) == list(A.cluster_stats())
            assert X.step_counter == 26 and X.cluster_sweep == 3
        assert A.hmc_stats()[1] > 0 and A.cluster_stats()[3] > 0 and list(A.cluster_stats()[[0, 4]]) == [3, 0]
        phi = A.download()
        assert same_bits(phi, B.download())
        for X in (A, B):                                # what the step kernels cache about the field still holds
            X.step(4)
        assert same_bits(A.download(), B.download()) and A.step_counter == 30
        p = dev_oracle.phi4_params(shape, dtau, M2, LAM, seed, C=cm.ORACLE_C[0])
        for s in range(26, 30):
            phi = dev_oracle.phi4_step(p, phi, s)
        assert same_bits(A.download(), phi)


def test_special_sites_on_both_sides_of_a_seam(gpu, monkeypatch):
    shape, tile = FORCED
    monkeypatch.setenv("SQ_CLUSTER_TILE", tile)
    Lx, Ly, Lz = shape
    at = lambda x, y, z: (z * Ly + y) * Lx + x          # noqa: E731
    f = cm.oracle_fields(shape)[1].copy()               # all positive: every special site has live neighbours
    u = f.view(np.uint32)
    # the seams of 8 x 4 x 2 bricks lie behind x = 7, y = 3 and z = 1, 3: pairs of sites across each of them
    u[at(7, 1, 0)], u[at(8, 1, 0)] = 0x7FC12345, 0xFFA00001                   # NaNs with payloads across the x seam
    f[at(3, 3, 1)] = f[at(3, 4, 1)] = f[at(3, 4, 2)] = np.inf                 # +inf across the y seam and a z seam
    f[at(12, 5, 4)] = f[at(12, 5, 0)] = f[at(12, 0, 0)] = -np.inf             # -inf across the z wrap and the y wrap
    f[at(15, 2, 3)], f[at(0, 2, 3)] = 0.0, -0.0                               # zeros across the x wrap
    f[at(5, 3, 3)], f[at(5, 4, 4)] = -0.0, 0.0
    seed, beta = cm.oracle_seeds(4)[1], cm.oracle_betas()[1]
    with _lat(shape, 1) as A:
        assert A.cluster_shape_info(shape)["tiles"] == (2, 2, 3)
        A.upload(_grid(shape, f))
        want = _sweeps(f, 11, 2, seed, beta, shape)
        _check(A, 11, want, np.zeros(5, dtype=np.int64))
    assert not ((want[-1][2].view(np.uint32) ^ u) & ~np.uint32(0x80000000)).any(), "only sign bits"
    bits, lab = want[0][:2]
    assert lab[at(3, 3, 1)] == lab[at(3, 4, 1)] == lab[at(3, 4, 2)] and bits[at(3, 3, 1)] & 2 and bits[at(3, 4, 1)] & 4
    assert lab[at(12, 5, 4)] == lab[at(12, 5, 0)] == lab[at(12, 0, 0)] == at(12, 0, 0)
    for i in (at(7, 1, 0), at(8, 1, 0), at(15, 2, 3), at(0, 2, 3)):
        assert bits[i] == 0 and (lab == i).sum() == 1


def test_refusals_leave_the_context_running(gpu, sqlib):
    from stochquant_amd import Phi4Lattice, StochQuantError
    shape = (16, 6, 5)
    f = _grid(shape, cm.oracle_fields(shape)[0])
    with _lat(shape) as A, _lat(shape) as B:
        for X in (A, B):
            X.upload(f)
        A.set_noise(0.0)
        for call in (lambda: A.cluster(1), lambda: A.cluster(0), lambda: A.step_hmc_cluster(1, nleap=2)):
            with pytest.raises(StochQuantError) as ei:
                call()
            assert ei.value.code == -4                      # SQ_E_STATE
        A.set_noise(cm.ORACLE_C[0])
        with pytest.raises(StochQuantError) as ei:
            A.cluster(-1)
        assert ei.value.code == -1 and sqlib.sq_phi4_step_hmc_cluster(A._h, -1, 1, 1, 0, None, None, None) == -1
        assert same_bits(A.download(), f) and A.cluster_sweep == 0 and not A.cluster_stats().any()
        ra, rb = A.cluster(2, record=True), B.cluster(2, record=True)
        assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and same_bits(A.download(), B.download())
        A.cluster_reset()
        assert not A.cluster_stats().any() and A.cluster_sweep == 2
    with Phi4Lattice((16, 4, 4), comm="loopback", nslabs=2) as S:
        S.upload(_grid((16, 4, 4), cm.oracle_fields((16, 4, 4))[0]))
        with pytest.raises(StochQuantError) as ei:
            S.cluster(1)
        assert ei.value.code == -4 and same_bits(S.download(), _grid((16, 4, 4), cm.oracle_fields((16, 4, 4))[0]))
        S.step(2)
