"""The NumPy statement of the cluster sums of include/stochquant.h (sq_phi4_ensemble_cluster_improved): on top of the
sweep of phi4_cluster_model.py the per-site fixed-point weights, their sums per cluster in int64 (np.add.at), the
record of eight doubles per lattice, and the kernel's way to the sums through 16-bit limbs.  The oracle of
test_gpu_phi4_ens_cluster_improved.py; checked without a GPU by test_phi4_cluster_improved_model.py.

As in phi4_cluster_model.py everything works on a batch of N lattices, phi of shape (N, sites)."""
import numpy as np

import phi4_cluster_model as cm

SAT = 32768.0                   # |phi| >= 2^15, inf and NaN: a saturated site, weight 0
ONE = 2.0 ** 32                 # the fixed point
NW = 7                          # M, A_x, B_x, A_y, B_y, A_z, B_z
REC = ("I2", "I4", "Fx", "Fy", "Fz", "Mmax", "Mtot", "nsat")
LARGEST = np.nextafter(np.float32(SAT), np.float32(0.0))       # the largest unsaturated float


def tables(shape):
    """[(c, s)] per axis x, y, z: the unit momentum's table of the momentum kernels (sq_phi4_ens_momentum_table)."""
    from stochquant_amd import Phi4Ensemble
    return [Phi4Ensemble.momentum_table(L, 1) for L in shape]


def coordinates(shape):
    """k[mu][i]: the coordinate of site i = (z Ly + y) Lx + x on axis mu = x, y, z."""
    Lx, Ly, Lz = shape
    i = np.arange(Lx * Ly * Lz)
    return [i % Lx, (i // Lx) % Ly, i // (Lx * Ly)]


def weights(phi, shape):
    """(w, sat): w[n, i, 0 .. 6] = q, a_x, b_x, a_y, b_y, a_z, b_z of site i as int64, sat[n, i] the saturated sites
    (all seven weights 0)."""
    phi = np.ascontiguousarray(phi, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        a = np.abs(phi.astype(np.float64))
        sat = ~(a < SAT)
    a = np.where(sat, 0.0, a)
    w = np.zeros(phi.shape + (NW,), dtype=np.int64)
    w[:, :, 0] = np.floor(a * ONE).astype(np.int64)
    for mu, ((c, s), k) in enumerate(zip(tables(shape), coordinates(shape))):
        w[:, :, 1 + 2 * mu] = np.rint((a * c[k][None, :]) * ONE).astype(np.int64)
        w[:, :, 2 + 2 * mu] = np.rint((a * s[k][None, :]) * ONE).astype(np.int64)
    return w, sat


def cluster_sums(w, labels):
    """W[n, l, 0 .. 6]: the sums of w over the cluster with label l, at the root's index, 0 elsewhere."""
    N, sites, _ = w.shape
    W = np.zeros_like(w)
    n = np.repeat(np.arange(N), sites)
    np.add.at(W, (n, np.asarray(labels, dtype=np.int64).reshape(-1)), w.reshape(N * sites, NW))
    return W


def limbs(w):
    """The three 16-bit limbs of the 48-bit signed weights, the top one signed: w = l0 + 2^16 l1 + 2^32 l2."""
    assert (np.abs(w) < 2 ** 47).all()
    return w & 0xFFFF, (w >> 16) & 0xFFFF, w >> 32


def limb_sums(w, labels):
    """cluster_sums the kernel's way: per limb a 32-bit sum per cluster (asserted to fit), the sum's upper half
    carried into the next limb's word, the three recombined at the root."""
    out = np.zeros_like(w)
    carry = np.zeros_like(w)
    for k, l in enumerate(limbs(w)):
        s = cluster_sums(l, labels) + carry
        assert (s < 2 ** 31).all() and (s >= -2 ** 31).all(), "a limb sum leaves 32 bits"
        if k < 2:
            assert (s >= 0).all()
            out += (s & 0xFFFF) << (16 * k)
            carry = s >> 16
        else:
            out += s << 32
    return out


def record(W, sat, labels):
    """(rec, nclusters): rec[n] = I2, I4, Fx, Fy, Fz, Mmax, Mtot, nsat of lattice n from its cluster sums."""
    N, sites, _ = W.shape
    root = np.asarray(labels) == np.arange(sites)[None, :]
    assert not W[~root].any()
    v = W.astype(np.float64) * 2.0 ** -32       # m, alpha_x, beta_x, ..: int64 to double rounds to nearest even
    m2 = v[:, :, 0] * v[:, :, 0]
    rec = np.zeros((N, 8))
    rec[:, 0] = m2.sum(axis=1)
    rec[:, 1] = (m2 * m2).sum(axis=1)
    for mu in range(3):
        al, be = v[:, :, 1 + 2 * mu], v[:, :, 2 + 2 * mu]
        rec[:, 2 + mu] = (al * al).sum(axis=1) + (be * be).sum(axis=1)
    rec[:, 5] = v[:, :, 0].max(axis=1)
    rec[:, 6] = W[:, :, 0].sum(axis=1).astype(np.float64) * 2.0 ** -32
    rec[:, 7] = sat.sum(axis=1)
    return rec, root.sum(axis=1)


def sweep(phi, betas, seeds, c, shape, factor=2.0):
    """phi4_cluster_model.sweep with the cluster sums of the field it started from: "weights" (N, sites, 7) int64,
    "rec" (N, 8), "sat" and "nclusters" beside that model's entries."""
    res = cm.sweep(phi, betas, seeds, c, shape, factor)
    w, sat = weights(phi, shape)
    W = cluster_sums(w, res["labels"])
    rec, ncl = record(W, sat, res["labels"])
    res.update(site_weights=w, weights=W, sat=sat, rec=rec, nclusters=ncl)
    return res


# ---- exact free-field samples: the inputs of the statistical tests ----
FREE_SHAPE, FREE_M2, FREE_C, FREE_DTAU, FREE_RNG = (8, 4, 4), 1.0, 1.0, 0.01, 2025


def free_beta():
    return cm.beta(cm.record(FREE_DTAU, FREE_M2, 0.0, FREE_C))


def khat2(shape):
    """The lattice momenta squared, shape (Lz, Ly, Lx)."""
    Lx, Ly, Lz = shape
    k = [4.0 * np.sin(np.pi * np.arange(L) / L) ** 2 for L in (Lz, Ly, Lx)]
    return k[0][:, None, None] + k[1][None, :, None] + k[2][None, None, :]


def free_fields(N, shape=FREE_SHAPE, m2=FREE_M2, beta=None, seed=FREE_RNG):
    """(N, sites) float32: N exact samples of exp(-beta S) of the free field, phi = ifftn(fftn(eta) / sqrt(beta (m2 +
    khat^2))) with eta white noise from default_rng(seed)."""
    Lx, Ly, Lz = shape
    beta = free_beta() if beta is None else beta
    eta = np.random.default_rng(seed).normal(size=(N, Lz, Ly, Lx))
    f = np.fft.ifftn(np.fft.fftn(eta, axes=(1, 2, 3)) / np.sqrt(beta * (m2 + khat2(shape)))[None], axes=(1, 2, 3))
    assert np.abs(f.imag).max() < 1e-12
    return np.ascontiguousarray(f.real.reshape(N, -1), dtype=np.float32)


def free_exact(shape=FREE_SHAPE, m2=FREE_M2, beta=None):
    """The exact means of I2, 3 I2^2 - 2 I4 and F_x, F_y, F_z."""
    beta = free_beta() if beta is None else beta
    V = shape[0] * shape[1] * shape[2]
    chi = V / (beta * m2)
    return [chi, 3.0 * chi * chi] + [V / (beta * (m2 + 4.0 * np.sin(np.pi / L) ** 2)) for L in shape]


def free_quantities(rec):
    """(..., 5): I2, 3 I2^2 - 2 I4, F_x, F_y, F_z of records (..., 8)."""
    rec = np.asarray(rec)
    return np.stack([rec[..., 0], 3.0 * rec[..., 0] ** 2 - 2.0 * rec[..., 1], rec[..., 2], rec[..., 3], rec[..., 4]],
                    axis=-1)
