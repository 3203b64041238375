"""The NumPy statement of the replica-exchange test of include/stochquant.h: the
pairing of a round, a slot's coefficients from its float record, and Δ from the
two fields' sums.  The oracle of test_gpu_phi4_ens_exchange.py; checked without
a GPU by test_phi4_exchange_model.py."""
import numpy as np

STREAM_EXCHANGE = 4     # kPhi4EnsStreamExchange (sq_phi4_ens.h)


def pairs(R, nlad, x):
    """The pairs (a, a + 1) of round x, ascending."""
    o = x & 1
    return [(l * nlad + o + 2 * j, l * nlad + o + 2 * j + 1)
            for l in range(R // nlad) for j in range((nlad - o) // 2)]


def partners(R, nlad, x):
    """partner[r] of every slot in round x, -1 without one."""
    p = [-1] * R
    for a, b in pairs(R, nlad, x):
        p[a], p[b] = b, a
    return p


def coef(rec):
    """(β, p, q) of a slot from its record (h, m2, lam6, sig), floats held in double."""
    h, m2, lam6, sig = (float(v) for v in rec)
    beta = 2.0 * h / (sig * sig)
    return beta, beta * (3.0 + m2 / 2.0), beta * (lam6 / 4.0)


def delta(rec_a, rec_b, sums_a, sums_b):
    """(Δ, A): the header's Δ of a pair from the slots' records and the rows (S1, S2, S4, NN, ..) of `moments()` of
    the fields they hold, and A, the sum of the magnitudes of its three products."""
    ba, pa, qa = coef(rec_a)
    bb, pb, qb = coef(rec_b)
    with np.errstate(invalid="ignore", over="ignore"):
        t2 = np.float64(pa - pb) * (np.float64(sums_b[1]) - np.float64(sums_a[1]))
        tn = np.float64(ba - bb) * (np.float64(sums_b[3]) - np.float64(sums_a[3]))
        t4 = np.float64(qa - qb) * (np.float64(sums_b[2]) - np.float64(sums_a[2]))
        return float((t2 - tn) + t4), float(abs(t2) + abs(tn) + abs(t4))


def uniform(o, seed, x):
    """u of the pair whose lower slot has `seed`, in round x (o: the oracle module, for Philox)."""
    w = o.philox([0, STREAM_EXCHANGE << 24, x & 0xFFFFFFFF, x >> 32], [seed & 0xFFFFFFFF, seed >> 32])[0]
    return (w + 0.5) * 2.0 ** -32


def verdict(d, u):
    """1 if Δ <= 0 or u < exp(-Δ), else 0 (a NaN Δ included)."""
    if d <= 0.0:
        return 1
    with np.errstate(over="ignore", invalid="ignore"):
        return int(u < float(np.exp(-np.float64(d))))
