"""The NumPy model of the cluster sweep (phi4_cluster_model.py) without a GPU: its Philox is the oracle's, its
sweep samples exp(β Σ φ_i φ_j) exactly (by enumeration of all 256 sign configurations of eight sites, with a test
of power: the same model at two wrong couplings fails), and the fields the GPU oracle test uploads have the
properties they are there for, with no bond too close to a tie to be decided across two exp implementations."""
import numpy as np
import pytest

import phi4_cluster_model as cm
from test_phi4_ens_shapes import GPU_SHAPES


def test_model_philox_is_the_oracles(oracle_mod):
    seeds = [0x123456789ABCDEF0, 5, 2 ** 64 - 1]
    for c in (0, 7, 2 ** 40 + 5, 2 ** 64 - 1):
        o = cm.blocks(seeds, c, 40)
        for n, seed in enumerate(seeds):
            for i in (0, 1, 17, 39):
                want = oracle_mod.philox([i, cm.STREAM_CLUSTER << 24, c & 0xFFFFFFFF, c >> 32],
                                         [seed & 0xFFFFFFFF, seed >> 32])
                assert list(o[n, i]) == want, (c, n, i)


def _chains(shape, N, nsweeps, beta, factor, seed0=1234):
    """N independent chains of nsweeps sweeps from db_start: the configuration numbers at the end."""
    phi = cm.db_start(shape, N)
    seeds = cm.oracle_seeds(N, seed0)
    for c in range(nsweeps):
        phi = cm.sweep(phi, [beta] * N, seeds, c, shape, factor)["phi"]
    return cm.sign_code(phi, cm.db_live(shape)), phi


def test_exactness_by_enumeration():
    """2 x 2 x 2: every bond is doubled.  32,768 chains of 12 sweeps from random signs against the exact weights;
    χ² <= 255 + 6 sqrt(510).  The model with 2β replaced by β and by 2.2β must exceed the bound."""
    shape, N = (2, 2, 2), 32768
    beta = cm.beta(cm.record(cm.ORACLE_DTAU, 0.0, 0.0, cm.DB_C))
    assert abs(beta - 0.390625) < 0.001
    p = cm.exact_weights(cm.db_magnitudes(), cm.db_live(shape), beta, shape)
    got = {}
    for factor in (2.0, 1.0, 2.2):
        codes, phi = _chains(shape, N, 12, beta, factor)
        assert np.array_equal(np.abs(phi), np.abs(cm.db_start(shape, N))), "only signs move"
        got[factor], emin = cm.chi2(codes, p)
        assert emin >= cm.DB_MIN_EXPECTED, emin
    print("chi2 2x2x2", got, "bound", cm.DB_CHI2_BOUND, flush=True)
    assert got[2.0] <= cm.DB_CHI2_BOUND, got
    assert got[1.0] > cm.DB_CHI2_BOUND and got[2.2] > cm.DB_CHI2_BOUND, got


def test_the_device_graph_by_enumeration():
    """The graph of the GPU's detailed-balance test (8 x 2 x 2, live sites x in {0, 1}: a single x-bond, doubled y-
    and z-bonds), run in the model at the GPU test's sample size: the definition passes, the two wrong couplings
    fail."""
    shape, R = cm.DB_SHAPE, cm.DB_R
    beta = cm.beta(cm.record(cm.ORACLE_DTAU, 0.0, 0.0, cm.DB_C))
    live = cm.db_live(shape)
    p = cm.exact_weights(cm.db_magnitudes(), live, beta, shape)
    # the exact weights see 4 single x-bonds and 16 doubled-bond terms
    fwd = cm.forward(shape)
    assert sum(int(fwd[mu][i]) in live for mu in range(3) for i in live) == 4 + 8 + 8
    seeds = cm.oracle_seeds(R, 4321)
    got = {}
    for factor in (2.0, 1.0, 2.2):
        phi = cm.db_start(shape, R)
        codes, c = [], 0
        for _ in range(cm.DB_SNAPSHOTS):
            for _ in range(cm.DB_GAP):
                res = cm.sweep(phi, [beta] * R, seeds, c, shape, factor)
                phi = res["phi"]
                c += 1
            codes.append(cm.sign_code(phi, live))
        dead = np.setdiff1d(np.arange(32), live)
        assert not (res["bits"][:, dead] != 0).any() and (res["labels"][:, dead] == dead[None, :]).all(), \
            "a 1e-30 site bonds with nothing"
        got[factor], emin = cm.chi2(np.concatenate(codes), p)
        assert emin >= cm.DB_MIN_EXPECTED, emin
    print("chi2 8x2x2", got, "bound", cm.DB_CHI2_BOUND, flush=True)
    assert got[2.0] <= cm.DB_CHI2_BOUND, got
    assert got[1.0] > cm.DB_CHI2_BOUND and got[2.2] > cm.DB_CHI2_BOUND, got


def test_the_serpentine_is_an_induced_path():
    for shape in GPU_SHAPES:
        path = cm.serpentine(shape)
        assert path[0] == 0 and len(set(path)) == len(path)
        where = {s: k for k, s in enumerate(path)}
        for nb in cm.forward(shape):
            for s, k in where.items():
                j = int(nb[s])
                assert j not in where or abs(where[j] - k) == 1, (shape, s, j)


@pytest.mark.parametrize("shape", list(GPU_SHAPES))
def test_oracle_inputs(shape):
    """No undecidable bond in any of the four sweeps of any replica, and each field has what it is there for."""
    sites = shape[0] * shape[1] * shape[2]
    betas = cm.oracle_betas()
    assert abs(betas[3] - 16.0) < 0.01 and len(set(cm.oracle_seeds(4))) == 4
    runs = cm.oracle_run(shape)
    assert [c for c, _ in runs] == [7, 8, 2 ** 40 + 5, 2 ** 40 + 6]
    for c, res in runs:
        assert res["margin"] >= 1e-12, (shape, c, res["margin"])
    first = runs[0][1]
    f = cm.oracle_fields(shape)
    # (0) both signs, both bond states, many clusters, both flip verdicts
    assert (f[0] > 0).any() and (f[0] < 0).any()
    assert 1 < first["stats"][0, 0] < sites and 0 < first["stats"][0, 1] < first["stats"][0, 0]
    # (1) one cluster holds more than half of the sites
    assert (f[1] > 0).all() and np.bincount(first["labels"][1]).max() > sites // 2
    # (2) two domains: no bond across the walls, at most a few clusters
    assert first["stats"][2, 0] >= 2 and set(np.unique(f[2])) == {np.float32(-1.2), np.float32(1.2)}
    # (3) the path is one cluster with site 0 at one end, and nothing else bonds
    path = cm.serpentine(shape)
    lab = first["labels"][3]
    assert (lab[path] == 0).all() and (lab == 0).sum() == len(path)
    rest = np.setdiff1d(np.arange(sites), path)
    assert (lab[rest] == rest).all()
    d = cm.diameter(first["bits"][3], shape, lab, 0)
    assert d == len(path) - 1
    need = sites / 8 if min(shape[1], shape[2]) >= 4 else max(shape) - 1
    assert d >= need, (shape, d, need)
    # every sweep keeps the path whole: its sites flip together
    for c, res in runs:
        assert (res["labels"][3][path] == 0).all() and len(set(res["flip"][3][path])) == 1
