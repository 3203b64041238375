"""The NumPy model of the cluster sums (phi4_cluster_improved_model.py) without a GPU, on 8192 exact free-field
samples of 8 x 4 x 4 (m2 = 1, lam = 0, C = 1, dtau = 0.01; one sweep at counter 3): the improved estimators have the
exact means V / (beta m2), 3 (V / (beta m2))^2 and V / (beta (m2 + 4 sin^2(pi / L_mu))) within 5 standard errors, with
caps on the standard errors so that a wide error bar cannot hide a wrong mean, the variance of I2 is well below the
naive (sum phi)^2's, and the same model with the bond coupling 2.2 beta fails.  Mtot is the exact sum of the q_i, and
the limb decomposition recombines to the int64 sums at the largest unsaturated field."""
import numpy as np
import pytest

import phi4_cluster_model as cm
import phi4_cluster_improved_model as im

N = 8192
COUNTER = 3
NAMES = ("I2", "fourth moment", "F_x", "F_y", "F_z")
CAPS = (0.0125, 0.035, 0.0075, 0.0075, 0.0075)      # relative standard errors
SIGMAS = 5.0


@pytest.fixture(scope="module")
def samples(sqlib):
    phi = im.free_fields(N)
    return phi, cm.oracle_seeds(N), [im.free_beta()] * N


@pytest.fixture(scope="module")
def swept(samples):
    phi, seeds, betas = samples
    return im.sweep(phi, betas, seeds, COUNTER, im.FREE_SHAPE)


def _deviations(rec):
    q = im.free_quantities(rec)
    mean, se = q.mean(axis=0), q.std(axis=0, ddof=1) / np.sqrt(q.shape[0])
    exact = np.asarray(im.free_exact())
    return (mean - exact) / se, se / exact


def test_improved_estimators_have_the_exact_means(samples, swept):
    dev, rel = _deviations(swept["rec"])
    for name, d, r in zip(NAMES, dev, rel):
        print(f"improved model {name}: {d:+.2f} sigma, relative s.e. {r:.4f}", flush=True)
    for name, d, r, cap in zip(NAMES, dev, rel, CAPS):
        assert abs(d) <= SIGMAS, (name, d)
        assert r <= cap, (name, r, cap)
    assert not swept["sat"].any() and (swept["rec"][:, 7] == 0).all()


def test_variance_gain(samples, swept):
    phi = samples[0]
    naive = phi.astype(np.float64).sum(axis=1) ** 2
    ratio = naive.var(ddof=1) / swept["rec"][:, 0].var(ddof=1)
    print(f"improved model var[(sum phi)^2] / var[I2] = {ratio:.2f}", flush=True)
    assert ratio >= 1.5, ratio
    # the naive estimator has the same mean: both are within 5 of its standard errors of the exact value
    assert abs(naive.mean() - im.free_exact()[0]) <= SIGMAS * naive.std(ddof=1) / np.sqrt(N)


def test_the_wrong_coupling_fails(samples):
    phi, seeds, betas = samples
    dev, _ = _deviations(im.sweep(phi, betas, seeds, COUNTER, im.FREE_SHAPE, factor=2.2)["rec"])
    print(f"improved model at 2.2 beta: I2 {dev[0]:+.2f} sigma, F_x {dev[2]:+.2f} sigma", flush=True)
    assert abs(dev[0]) > SIGMAS and abs(dev[2]) > SIGMAS, dev


def test_mtot_is_the_sum_of_q(samples, swept):
    w = swept["site_weights"]
    tot = w[:, :, 0].sum(axis=1)
    assert np.array_equal(swept["weights"][:, :, 0].sum(axis=1), tot)
    assert np.array_equal(swept["rec"][:, 6], tot.astype(np.float64) * 2.0 ** -32)
    a = np.abs(samples[0].astype(np.float64))
    assert np.array_equal(w[:, :, 0], np.floor(a * 2.0 ** 32).astype(np.int64))
    # every cluster's sums sit at its root, and the labels are the plain model's
    plain = cm.sweep(samples[0], samples[2], samples[1], COUNTER, im.FREE_SHAPE)
    assert np.array_equal(plain["labels"], swept["labels"]) and np.array_equal(plain["phi"], swept["phi"])
    root = swept["labels"] == np.arange(w.shape[1])[None, :]
    assert not swept["weights"][~root].any()
    assert np.array_equal(swept["nclusters"], plain["stats"][:, 0])


@pytest.mark.parametrize("shape", [(8, 2, 2), (8, 4, 4), (32, 32, 32)])
def test_limbs_recombine_at_the_largest_field(sqlib, shape):
    """Every site at nextafter(32768, 0) in one cluster: every limb sum near its maximum; then alternating-sign
    z-planes in two clusters and a random labelling."""
    sites = shape[0] * shape[1] * shape[2]
    assert float(im.LARGEST) < im.SAT and float(np.nextafter(im.LARGEST, np.float32(np.inf))) == im.SAT
    phi = np.full((1, sites), im.LARGEST, dtype=np.float32)
    w, sat = im.weights(phi, shape)
    assert not sat.any() and w[0, 0, 0] == (2 ** 24 - 1) << 23
    z = np.arange(sites) // (shape[0] * shape[1])
    rng = np.random.default_rng(5)
    for lab in (np.zeros((1, sites), dtype=np.int32), (z % 2 * shape[0] * shape[1])[None, :].astype(np.int32),
                np.minimum(np.arange(sites), rng.integers(0, sites, sites))[None, :].astype(np.int32)):
        want = im.cluster_sums(w, lab)
        assert np.array_equal(im.limb_sums(w, lab), want)
        assert (np.abs(want) < 2 ** 62).all()
    l0, l1, l2 = im.limbs(w)
    assert np.array_equal(l0 + (l1 << 16) + (l2 << 32), w) and l2.min() < 0 < l2.max()
    assert im.cluster_sums(w, np.zeros((1, sites), dtype=np.int32))[0, 0, 0] == sites * w[0, 0, 0]


def test_saturated_sites_weigh_nothing(sqlib):
    shape = (8, 2, 2)
    phi = np.full((1, 32), 0.5, dtype=np.float32)
    phi[0, :6] = [np.nan, np.inf, -np.inf, 32768.0, -0.0, 1e-30]
    phi[0, 6] = -im.LARGEST
    w, sat = im.weights(phi, shape)
    assert sat[0, :8].tolist() == [True] * 4 + [False] * 4 and not w[0, :4].any()
    assert w[0, 4, 0] == 0 and w[0, 5, 0] == 0 and w[0, 6, 0] == (2 ** 24 - 1) << 23 and w[0, 7, 0] == 2 ** 31
    rec, ncl = im.record(im.cluster_sums(w, np.arange(32)[None, :]), sat, np.arange(32)[None, :])
    assert rec[0, 7] == 4 and ncl[0] == 32 and rec[0, 5] == float(im.LARGEST)
