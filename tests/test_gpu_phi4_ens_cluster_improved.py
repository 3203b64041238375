"""The cluster sums of the phi^4 ensemble's Swendsen-Wang sweep on the GPU (sq_phi4_ensemble_cluster_improved,
sq_phi4_ensemble_step_hmc_cluster_improved) against the NumPy statement of the header's definition
(phi4_cluster_improved_model.py), and the sweep itself against a twin handle that runs the plain call.

Tolerances.  The weights (int64 sums per cluster), Mmax, Mtot, nsat, fields, bonds, labels, counters and
statistics: exact.  I2, I4 and each F are sums of n_clusters non-negative doubles whose terms are the model's bit for
bit and whose order is the kernel's: within n_clusters 2^-52 relative of the model's value, the bound on reordering
such a sum.  The physics check takes its bound (5 standard errors of the replica scatter, the error capped at 3 %)
from the exact free-field value."""
import numpy as np
import pytest

import phi4_cluster_improved_model as im
import phi4_cluster_model as cm
from test_gpu_phi4_ens_cluster import _bits, _betas, _ens, _flat, _lat, _same, _state, _thermal
from test_gpu_phi4_ens_hmc import CLASS_SHAPES
from test_oracle import same_bits
from test_phi4_ens_shapes import GPU_SHAPES, assert_shape

pytestmark = pytest.mark.gpu

SIGN = np.uint32(0x80000000)
K_SHAPES = [(8, 8, 8), (64, 16, 8), (16, 24, 24), (32, 32, 32)]        # K = 1, 2, 4, 8; the last holds 32,768 sites


def check_records(shape, phi, ser, labels, weights):
    """One sweep's series (R, 8) and weights (R, sites, 7) against the model's sums of the field `phi` (R, sites)
    the sweep started from, over the sweep's own labels.  Returns the model's record."""
    w, sat = im.weights(phi, shape)
    W = im.cluster_sums(w, labels)
    assert np.array_equal(weights, W), (shape, np.argwhere(weights != W)[:8])
    rec, ncl = im.record(W, sat, labels)
    for k in (5, 6, 7):
        assert np.array_equal(_bits(ser[:, k]), _bits(rec[:, k])), (shape, im.REC[k], ser[:, k], rec[:, k])
    for k in range(5):
        err = np.abs(ser[:, k] - rec[:, k])
        assert (err <= ncl * 2.0 ** -52 * np.abs(rec[:, k])).all(), (shape, im.REC[k], ser[:, k], rec[:, k], ncl)
    return rec


def run_pair(A, B, nsweeps):
    """cluster_improved(nsweeps, record=True) on A and cluster(nsweeps, record=True) on its twin B: the plain
    call's records and state bit for bit, and every sweep's sums against the model."""
    shape = A.shape
    phi = _flat(A, A.download())
    ser, bonds, labels, weights = A.cluster_improved(nsweeps, record=True)
    pb, pl = B.cluster(nsweeps, record=True)
    sites = shape[0] * shape[1] * shape[2]
    assert ser.shape == (nsweeps, A.R, 8) and weights.shape == (nsweeps, A.R, sites, 7) and weights.dtype == np.int64
    assert np.array_equal(bonds, pb) and np.array_equal(labels, pl)
    _same(_state(A), _state(B))
    recs = []
    for i in range(nsweeps):
        recs.append(check_records(shape, phi, ser[i], labels[i], weights[i]))
        odd = (cm.blocks(cm.oracle_seeds(A.R), A.cluster_sweep - nsweeps + i, sites)[:, :, 3] & 1).astype(bool)
        flip = np.take_along_axis(odd, labels[i].astype(np.int64), axis=1)
        phi = (phi.view(np.uint32) ^ (flip.astype(np.uint32) << np.uint32(31))).view(np.float32)
    assert same_bits(A.download(), _lat(A, phi))
    return ser, labels, weights, recs


@pytest.mark.parametrize("shape", list(GPU_SHAPES))
def test_against_the_model(gpu, shape):
    assert_shape(shape)
    with _ens(shape) as A, _ens(shape) as B:
        for E in (A, B):
            E.upload(_lat(E, cm.oracle_fields(shape)))
        first = None
        for c in cm.ORACLE_SWEEPS:
            A.cluster_sweep = B.cluster_sweep = c
            ser, labels, weights, recs = run_pair(A, B, 2)
            first = (ser[0], labels[0]) if first is None else first
        assert A.cluster_stats()[:, 0].tolist() == [4] * 4 and not A.cluster_stats()[:, 4].any()
    # the fields are there for something: many clusters, one percolating cluster, the path
    assert (first[0][:, 7] == 0).all() and (first[0][:, 5] > 0).all() and (first[0][:, 5] <= first[0][:, 6]).all()
    assert (first[1][3][cm.serpentine(shape)] == 0).all()
    print(f"cluster sums {shape} I2 {first[0][:, 0].tolist()}", flush=True)


@pytest.mark.parametrize("shape", K_SHAPES)
def test_limb_extremes(gpu, shape):
    """Every site at the largest unsaturated float: one cluster of all sites, every limb sum near its maximum; then
    the same magnitudes with alternating-sign z-planes: one cluster per plane and signed top limbs in A and B."""
    info = assert_shape(shape)
    assert info["K"] == {(8, 8, 8): 1, (64, 16, 8): 2, (16, 24, 24): 4, (32, 32, 32): 8}[shape]
    sites = shape[0] * shape[1] * shape[2]
    z = np.arange(sites) // (shape[0] * shape[1])
    one = np.full((4, sites), im.LARGEST, dtype=np.float32)
    planes = np.where(z % 2 == 0, one, -one).astype(np.float32)
    for f, ncl in ((one, 1), (planes, shape[2])):
        with _ens(shape) as A, _ens(shape) as B:
            for E in (A, B):
                E.upload(_lat(E, f))
                E.cluster_sweep = 5
            ser, labels, weights, recs = run_pair(A, B, 1)
            assert (A.cluster_stats()[:, 1] == ncl).all()
        assert np.array_equal(_bits(ser[0]), _bits(recs[0])) or ncl > 1       # one term: no order to differ in
        assert np.array_equal(weights[0], im.limb_sums(im.weights(f, shape)[0], labels[0]))
        assert weights[0][:, 0, 0].tolist() == [(sites // ncl) * ((2 ** 24 - 1) << 23)] * 4
        assert (ser[0][:, 7] == 0).all() and (ncl == 1 or (weights[0][:, :, 5] < -2 ** 32).any())
        if ncl == 1:
            assert (ser[0][:, 5] == ser[0][:, 6]).all() and ser[0][0, 6] == sites * float(im.LARGEST)


@pytest.mark.parametrize("shape", [(8, 2, 2), (32, 24, 24)])
def test_saturated_sites(gpu, shape):
    """NaN, +-inf and exactly 32768.0 weigh nothing and are counted; +-0 and 1e-30 weigh their q = 0; the sweep
    itself is the plain one's, so every other bit of the field stays."""
    assert assert_shape(shape)["K"] == {(8, 2, 2): 1, (32, 24, 24): 8}[shape]
    sites = shape[0] * shape[1] * shape[2]
    f = cm.oracle_fields(shape)
    u = f.view(np.uint32)
    at = {"nan": 5, "-nan": sites // 2 + 3, "inf": 9, "-inf": sites - 1, "edge": 12, "-edge": sites - 7, "zero": 17,
          "-zero": 20, "tiny": 23, "largest": 26}
    u[0, at["nan"]], u[0, at["-nan"]] = 0x7FC12345, 0xFFA00001
    f[0, at["inf"]], f[0, at["-inf"]] = np.inf, -np.inf
    f[0, at["edge"]], f[0, at["-edge"]] = 32768.0, -32768.0
    f[0, at["zero"]], f[0, at["-zero"]], f[0, at["tiny"]], f[0, at["largest"]] = 0.0, -0.0, 1e-30, im.LARGEST
    f[1, 7] = np.nan
    f[2, :] = np.inf                                    # every site saturated: all sums 0
    with _ens(shape) as A, _ens(shape) as B:
        for E in (A, B):
            E.upload(_lat(E, f))
            E.cluster_sweep = 11
        ser, labels, weights, recs = run_pair(A, B, 2)
        after = _flat(A, A.download()).view(np.uint32)
    assert not ((after ^ u) & ~SIGN).any(), "only sign bits"
    w, sat = im.weights(f, shape)
    assert sat[0].sum() == 6 and sat[1].sum() == 1 and sat[2].all() and not sat[3].any()
    for i in range(2):
        assert ser[i][:, 7].tolist() == [6.0, 1.0, float(sites), 0.0]
        assert not ser[i][2, :7].any() and not weights[i][2].any()
        for k in ("nan", "-nan", "inf", "-inf", "edge", "-edge"):
            assert not w[0, at[k]].any()
        lab = labels[i][0]
        for k in ("nan", "-nan", "zero", "-zero"):       # a cluster of its own with the sums of nothing
            assert lab[at[k]] == at[k] and not weights[i][0, at[k]].any()
    assert w[0, at["largest"], 0] == (2 ** 24 - 1) << 23 and w[0, at["tiny"], 0] == 0


def test_sweeps_split_over_calls(gpu):
    shape = (8, 17, 31)
    with _thermal(shape) as A, _thermal(shape) as B:
        for E in (A, B):
            E.cluster_sweep = 2 ** 32 - 2
        sa, ba, la, wa = A.cluster_improved(4, record=True)
        parts = [B.cluster_improved(1, record=True) for _ in range(4)]
        for k, got in enumerate((sa, ba, la, wa)):
            assert np.array_equal(got, np.concatenate([p[k] for p in parts])), k
        assert np.array_equal(_bits(sa), _bits(np.concatenate([p[0] for p in parts])))
        _same(_state(A), _state(B))
        assert A.cluster_sweep == 2 ** 32 + 2 and (sa[:, :, 0] > 0).all()
        # without records: the same series; no sweep: empty arrays
        with _thermal(shape) as C:
            C.cluster_sweep = 2 ** 32 - 2
            assert np.array_equal(_bits(C.cluster_improved(4)), _bits(sa))
            _same(_state(A), _state(C))
        assert A.cluster_improved(0).shape == (0, 4, 8) and A.cluster_improved(0, record=True)[3].shape == \
            (0, 4, 8 * 17 * 31, 7)


def test_a_replica_does_not_depend_on_the_others(gpu):
    shape = (16, 4, 31)
    seeds = cm.oracle_seeds(5)
    C = list(np.resize(cm.ORACLE_C[:3], 5))
    with _thermal(shape, R=5, C=C, seeds=seeds) as A:
        sa, ba, la, wa = A.cluster_improved(2, record=True)
        for r in (0, 3, 4):
            with _thermal(shape, R=1, C=[C[r]], seeds=[seeds[r]]) as B:
                sb, bb, lb, wb = B.cluster_improved(2, record=True)
                assert np.array_equal(_bits(sa[:, r]), _bits(sb[:, 0])) and np.array_equal(wa[:, r], wb[:, 0])
                assert np.array_equal(la[:, r], lb[:, 0]) and same_bits(A.download(r, 1), B.download())


@pytest.mark.parametrize("shape", CLASS_SHAPES)
def test_fused_call_is_the_loop(gpu, shape):
    assert_shape(shape)
    with _thermal(shape) as A, _thermal(shape) as B, _thermal(shape) as P:
        ser, rh, bo, la, cs, we = A.step_hmc_cluster_improved(3, ntraj=2, nleap=3, every=1, correlate=True,
                                                              record=True)
        sites = shape[0] * shape[1] * shape[2]
        assert ser.shape == rh.shape == (6, 4, 4) and cs.shape == (3, 4, 8) and we.shape == (3, 4, sites, 7)
        parts = []
        for _ in range(3):
            s, r = B.step_hmc(2, nleap=3, every=1, correlate=True, record=True)
            parts.append((s, r) + tuple(B.cluster_improved(1, record=True)))
        # parts: series, rec_hmc, cseries, bonds, labels, weights
        for got, k in ((ser, 0), (rh, 1), (cs, 2)):
            assert np.array_equal(_bits(got), _bits(np.concatenate([p[k] for p in parts]))), k
        for got, k in ((bo, 3), (la, 4), (we, 5)):
            assert np.array_equal(got, np.concatenate([p[k] for p in parts])), k
        _same(_state(A), _state(B))
        # the plain fused call: the same chain
        ps, pr, pb, pl = P.step_hmc_cluster(3, ntraj=2, nleap=3, every=1, correlate=True, record=True)
        assert np.array_equal(_bits(ps), _bits(ser)) and np.array_equal(pb, bo) and np.array_equal(pl, la)
        _same(_state(A), _state(P))
        with _thermal(shape) as C:                          # without records
            s2, c2 = C.step_hmc_cluster_improved(3, ntraj=2, nleap=3)
            assert s2 is None and np.array_equal(_bits(c2), _bits(cs)) and same_bits(C.download(), A.download())


def test_free_field_susceptibility(gpu):
    """8 x 4 x 4, R = 1024, lam = 0, m2 = 1, C = 1 from the exact free-field samples of the CPU test: 20 rounds of
    one trajectory (nleap = 4, dtau = 0.02) and one sweep; the mean of I2 over the last 10 rounds against V / (beta
    m2), within 5 standard errors of the replica means' scatter, the error at most 3 %."""
    from stochquant_amd import Phi4Ensemble
    shape, R, dtau = im.FREE_SHAPE, 1024, 0.02
    beta = cm.beta(cm.record(dtau, im.FREE_M2, 0.0, im.FREE_C))
    with _ens(shape, R=R, C=[im.FREE_C] * R, seeds=cm.oracle_seeds(R), dtau=dtau, m2=im.FREE_M2, lam=0.0) as E:
        E.upload(_lat(E, im.free_fields(R)))
        ser, cs = E.step_hmc_cluster_improved(20, ntraj=1, nleap=4)
        assert ser is None and cs.shape == (20, R, 8) and not E.flags().any() and not E.cluster_stats()[:, 4].any()
        acc = E.hmc_stats()[:, 1].sum() / E.hmc_stats()[:, 0].sum()
    assert (cs[:, :, 7] == 0).all()
    per = cs[10:, :, 0].mean(axis=0)
    mean, se = per.mean(), per.std(ddof=1) / np.sqrt(R)
    exact = im.free_exact(shape, im.FREE_M2, beta)[0]
    obs = Phi4Ensemble.cluster_observables(cs[10:], shape)
    print(f"free field I2 {mean:.3f} +- {se:.3f} exact {exact:.3f}: {(mean - exact) / se:+.2f} sigma, relative s.e. "
          f"{se / exact:.4f}, acceptance {acc:.3f}, observables {obs}", flush=True)
    assert se / exact <= 0.03, se / exact
    assert abs(mean - exact) <= 5.0 * se, (mean, se, exact)
    V = shape[0] * shape[1] * shape[2]
    assert obs["chi"][0] == pytest.approx(mean / V, rel=1e-12) and obs["chi"][1] == pytest.approx(se / V, rel=1e-9)
    assert len(obs["xi"]) == 3 and abs(obs["binder"][0]) < 5.0 * obs["binder"][1] + 0.05
