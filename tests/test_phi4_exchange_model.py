"""The exchange model (phi4_exchange_model.py) without a GPU: Δ vanishes for
equal parameters, changes sign when the two fields change places, is the
difference of the four energies β_r S_r(φ) evaluated site by site, and the
pairing table of (nlad, x) is the header's."""
import math

import numpy as np
import pytest

import phi4_exchange_model as xm
from test_gpu_phi4_ens_mala import _record


def _sums(phi):
    f = phi.astype(np.float64)
    nn = sum(float(np.sum(f * np.roll(f, -1, axis=a))) for a in (2, 1, 0))
    return [float(f.sum()), float((f * f).sum()), float((f ** 4).sum()), nn, float(np.abs(f).max())]


def _fields():
    rng = np.random.default_rng(11)
    return (rng.normal(0.0, 0.6, (6, 4, 8)).astype(np.float32), rng.normal(0.2, 0.8, (6, 4, 8)).astype(np.float32))


def test_equal_parameters_give_zero():
    fa, fb = _fields()
    rec = _record(0.02, 0.5, 1.0, 1.07)
    d, A = xm.delta(rec, rec, _sums(fa), _sums(fb))
    assert d == 0.0 and A == 0.0
    assert xm.verdict(d, 0.999999) == 1


def test_swapping_the_fields_flips_the_sign():
    fa, fb = _fields()
    ra, rb = _record(0.02, 0.5, 1.0, 1.0), _record(0.02, 0.3, 1.4, 1.145)
    d, A = xm.delta(ra, rb, _sums(fa), _sums(fb))
    d2, A2 = xm.delta(ra, rb, _sums(fb), _sums(fa))
    assert d != 0.0 and d2 == -d and A2 == A
    # and exchanging the slots' roles as well gives Δ back: the pair is unordered
    d3, _ = xm.delta(rb, ra, _sums(fb), _sums(fa))
    assert d3 == d


def test_delta_is_the_difference_of_the_four_energies():
    fa, fb = _fields()
    ra, rb = _record(0.02, 0.5, 1.0, 1.0), _record(0.01, -0.3, 1.4, 1.225)

    def energy(rec, phi):
        h, m2, lam6, sig = rec
        f = phi.astype(np.float64)
        terms = [(3.0 + 0.5 * m2) * f * f, 0.25 * lam6 * f ** 4] + [-f * np.roll(f, -1, axis=a) for a in (2, 1, 0)]
        flat = np.concatenate([t.ravel() for t in terms])
        return 2.0 * h / (sig * sig) * math.fsum(flat), 2.0 * h / (sig * sig) * math.fsum(np.abs(flat))

    (eab, m1), (eba, m2_), (eaa, m3), (ebb, m4) = energy(ra, fb), energy(rb, fa), energy(ra, fa), energy(rb, fb)
    d, _ = xm.delta(ra, rb, _sums(fa), _sums(fb))
    assert abs(d - (eab + eba - eaa - ebb)) <= 1e-12 * (m1 + m2_ + m3 + m4)


def test_verdict_rule():
    assert xm.verdict(-1.0, 0.99) == 1 and xm.verdict(0.0, 0.99) == 1
    assert xm.verdict(1.0, 0.3) == 1 and xm.verdict(1.0, 0.4) == 0      # exp(-1) = 0.3679
    assert xm.verdict(float("nan"), 0.0) == 0 and xm.verdict(float("inf"), 0.0) == 0


TABLE = {
    (2, 0): [(0, 1)], (2, 1): [],
    (3, 0): [(0, 1)], (3, 1): [(1, 2)],
    (4, 0): [(0, 1), (2, 3)], (4, 1): [(1, 2)],
    (5, 0): [(0, 1), (2, 3)], (5, 1): [(1, 2), (3, 4)],
}


@pytest.mark.parametrize("nlad", [2, 3, 4, 5])
def test_pairing_table(nlad):
    for x in (0, 1, 6, 7, 2 ** 40 + 4, 2 ** 40 + 5):
        want = TABLE[(nlad, x & 1)]
        assert xm.pairs(nlad, nlad, x) == want
        # three ladders: the same pairs shifted, none across a boundary
        got = xm.pairs(3 * nlad, nlad, x)
        assert got == [(a + l * nlad, b + l * nlad) for l in range(3) for a, b in want]
        assert all(a // nlad == b // nlad and b == a + 1 for a, b in got)
        p = xm.partners(3 * nlad, nlad, x)
        assert all((p[r] == -1) or p[p[r]] == r for r in range(3 * nlad))
        assert sum(v >= 0 for v in p) == 2 * len(got)
