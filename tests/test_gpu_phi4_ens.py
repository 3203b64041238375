"""The phi^4 lattice ensemble on the GPU (sq_phi4_ens_*, Phi4Ensemble): R small
lattices per launch, each on-chip in one work-group.

Replica r must be bit for bit the single context (Phi4Lattice, comm="none") of
the same shape, parameters, seed, step counter and start field, hence also the
oracle's.  The shapes are test_phi4_ens_shapes.GPU_SHAPES; that file's CPU
test asserts that they hold a lattice of every work-group shape the launchers
can pick (K, LDS images, owned quads that do not exist), and every test here
first asserts that its shape still gets the work-group shape listed there.

Tolerances: bitwise everywhere except (a) the mathematical oracle, whose bound
is the suite's per-step fp32 bound (conftest.PHI4_STEP_ATOL / RTOL), and (b)
the in-flight sums, which the kernel adds in double in its own order: any
order of n double additions of terms t_i differs from the exact sum by at most
(n - 1) u sum |t_i| (u = 2^-53), a phi^4 term adds one rounding, and the bound
asserted is 2 n u sum |t_i| against the exactly rounded sum (math.fsum).
"""
import math

import numpy as np
import pytest

from conftest import PHI4_STEP_ATOL, PHI4_STEP_RTOL, tol_report
from test_phi4_ens_shapes import GPU_SHAPES, assert_shape

pytestmark = pytest.mark.gpu

SHAPES = list(GPU_SHAPES)
# the shapes this file began with come first and keep their parametrised ids
assert SHAPES[:7] == [(8, 2, 2), (8, 8, 8), (16, 4, 31), (32, 8, 13), (64, 16, 8), (32, 32, 32), (64, 16, 32)]
# K = 4 with 240 owned quads that do not exist; the largest K = 4 lattice; the largest two-image lattice (20
# missing quads); K = 8 with one image, Ly = 2 and 496 missing quads
MEASURED = [(64, 3, 43), (16, 32, 32), (8, 50, 51), (32, 2, 321)]
DTAU, M2, LAM = 0.02, 0.5, 1.0
SEEDS = [1234, 99, 0xDEADBEEF12345]

_cache = {}


def _ens(shape, R, **kw):
    from stochquant_amd import Phi4Ensemble
    kw.setdefault("dtau", DTAU)
    kw.setdefault("m2", M2)
    kw.setdefault("lam", LAM)
    return Phi4Ensemble(shape, R, **kw)


def _lat(shape, **kw):
    from stochquant_amd import Phi4Lattice
    return Phi4Lattice(shape, **kw)


def _starts(oracle_mod, shape, amp=0.9, seeds=(77, 78, 79)):
    """Distinct start fields, one per replica (computed once per shape)."""
    key = ("start", shape, amp, tuple(seeds))
    if key not in _cache:
        _cache[key] = np.stack([oracle_mod.phi4_init(oracle_mod.phi4_params(shape, DTAU, M2, LAM, s), amp)
                                for s in seeds])
        _cache[key].setflags(write=False)
    return _cache[key]


def _oracle_run(oracle_mod, shape, phi, steps, seed, C, dtau=DTAU, m2=M2, lam=LAM, step0=0):
    p = oracle_mod.phi4_params(shape, dtau, m2, lam, seed, C=C)
    for s in range(steps):
        phi = oracle_mod.phi4_step(p, phi, step0 + s)
    return phi


def _noisy_run(oracle_mod, shape):
    """4 noisy steps of 3 replicas with distinct seeds (one GPU run per shape)."""
    key = ("noisy", shape)
    if key not in _cache:
        with _ens(shape, 3, C=1.0, seeds=SEEDS) as E:
            E.upload(_starts(oracle_mod, shape))
            E.step(4)
            _cache[key] = E.download()
    return _cache[key]


@pytest.mark.parametrize("shape", SHAPES)
def test_noiseless_bitwise_vs_oracle(gpu, oracle_mod, shape):
    assert_shape(shape)
    phi0 = _starts(oracle_mod, shape)
    with _ens(shape, 3, C=0.0, seeds=SEEDS) as E:
        E.upload(phi0)
        E.step(5)
        got = E.download()
        assert not E.flags().any()
        assert list(E.step_counter) == [5, 5, 5]
    for r in range(3):
        ref = _oracle_run(oracle_mod, shape, phi0[r], 5, SEEDS[r], 0.0)
        assert np.array_equal(got[r], ref), f"replica {r}: max diff {np.max(np.abs(got[r] - ref))}"


@pytest.mark.parametrize("shape", SHAPES)
def test_noisy_bitwise_vs_device_oracle(gpu, dev_oracle, shape):
    assert_shape(shape)
    phi0 = _starts(dev_oracle, shape)
    got = _noisy_run(dev_oracle, shape)
    for r in range(3):
        ref = _oracle_run(dev_oracle, shape, phi0[r], 4, SEEDS[r], 1.0)
        assert np.array_equal(got[r], ref), f"replica {r}: max diff {np.max(np.abs(got[r] - ref))}"


@pytest.mark.parametrize("shape", SHAPES)
def test_noisy_within_tolerance_of_mathematical_oracle(gpu, oracle_mod, shape):
    assert_shape(shape)
    phi0 = _starts(oracle_mod, shape)
    got = _noisy_run(oracle_mod, shape)
    k = 4
    for r in range(3):
        ref = _oracle_run(oracle_mod, shape, phi0[r], k, SEEDS[r], 1.0)
        err = np.abs(got[r].astype(np.float64) - ref)
        tol_report(f"phi4_ens{shape}r{r}", err, k, ref, PHI4_STEP_RTOL)
        assert np.all(err <= k * (PHI4_STEP_ATOL + PHI4_STEP_RTOL * np.abs(ref)))


@pytest.mark.parametrize("shape", [(8, 8, 8), (32, 8, 13), (32, 32, 32), (64, 3, 43), (8, 50, 51)])
def test_bitwise_vs_single_context(gpu, shape):
    assert_shape(shape)
    dt = [0.005, 0.01, 0.02, 0.03]
    m2 = [-0.5, 0.25, 0.5, 1.0]
    lam = [0.5, 1.0, 2.0, 4.0]
    C = [0.0, 0.5, 1.0, 1.0]
    seeds = [11, 12, 0x1_0000_0005, 14]
    s0 = [0, 0, 2 ** 32 - 3, 40]
    with _ens(shape, 4, dtau=dt, m2=m2, lam=lam, C=C, seeds=seeds) as E:
        E.init_field(0.7)
        E.step_counter = s0
        start = E.download()
        E.step(7)
        got = E.download()
        steps = E.step_counter
        par = E.get_params()
    assert list(par["dtau"]) == dt and list(par["m2"]) == m2 and list(par["lam"]) == lam and list(par["C"]) == C
    for r in range(4):
        with _lat(shape, dtau=dt[r], m2=m2[r], lam=lam[r], C=C[r], seed=seeds[r]) as L:
            L.init_field(0.7)
            assert np.array_equal(start[r], L.download()), f"replica {r}: init_field differs"
            L.step_counter = s0[r]
            L.step(7)
            assert np.array_equal(got[r], L.download()), f"replica {r}: field differs after 7 steps"
            assert int(steps[r]) == L.step_counter == s0[r] + 7


@pytest.mark.parametrize("shape", [(16, 4, 31), (32, 32, 32)])
def test_split_calls_are_additive(gpu, oracle_mod, shape):
    phi0 = _starts(oracle_mod, shape)[:2]
    with _ens(shape, 2, seeds=SEEDS[:2]) as A, _ens(shape, 2, seeds=SEEDS[:2]) as B:
        A.upload(phi0)
        B.upload(phi0)
        A.step(11)
        for n in (1, 4, 6):
            B.step(n)
        assert np.array_equal(A.download(), B.download())
        assert list(A.step_counter) == list(B.step_counter) == [11, 11]


def test_long_call_equals_single_context(gpu):
    shape = (8, 8, 8)
    with _ens(shape, 2, seeds=[5, 6]) as E:
        E.init_field(0.5)
        E.step(300)
        got = E.download()
        assert E.perf()["steps"] == 600 and E.perf()["kernel_launches"] == 1
    for r, seed in enumerate([5, 6]):
        with _lat(shape, dtau=DTAU, m2=M2, lam=LAM, seed=seed) as L:
            L.init_field(0.5)
            L.step(300)
            assert np.array_equal(got[r], L.download())


def test_independent_of_replica_count_and_position(gpu):
    shape = (16, 4, 31)
    s = [101, 202, 303, 404, 505]
    with _ens(shape, 5, seeds=s) as A, _ens(shape, 2, seeds=[s[3], s[1]]) as B:
        for E in (A, B):
            E.init_field(0.6)
            E.step(5)
        a, b = A.download(), B.download()
    assert np.array_equal(b[0], a[3]) and np.array_equal(b[1], a[1])


def test_more_work_groups_than_the_chip_holds(gpu, oracle_mod):
    shape, R = (8, 8, 8), 1500
    phi0 = _starts(oracle_mod, shape)[0]
    with _ens(shape, R, C=0.0) as E:
        E.upload(phi0)
        E.step(3)
        got = E.download()
    assert np.all(got == got[0]), "replicas that started equal differ"
    ref = _oracle_run(oracle_mod, shape, phi0, 3, 0, 0.0)
    for r in (0, 749, 1499):
        assert np.array_equal(got[r], ref)


def test_guard_on_uploaded_non_finite_values(gpu, oracle_mod):
    shape = (8, 8, 8)
    phi0 = np.array(_starts(oracle_mod, shape, amp=0.3))
    bad = phi0[1]
    bad[3, 4, 5] = np.float32(5e3)
    bad[6, 1, 2] = np.float32("nan")
    bad[0, 0, 0] = np.float32("inf")
    bad[7, 7, 7] = np.float32("-inf")
    with _ens(shape, 3, seeds=SEEDS) as E:
        E.upload(phi0)
        E.step(2)
        got = E.download()
        assert list(E.flags()) == [False, True, False]
        assert list(E.flags(clear=True)) == [False, True, False]
        assert not E.flags().any()
    assert np.all(np.abs(got) <= 1000)
    for r in range(3):
        with _lat(shape, dtau=DTAU, m2=M2, lam=LAM, seed=SEEDS[r]) as L:
            L.upload(phi0[r])
            L.step(2)
            assert np.array_equal(got[r], L.download()), f"replica {r}"


def test_guard_flag_of_a_diverging_replica(gpu, oracle_mod):
    shape = (8, 8, 8)
    quiet = _starts(oracle_mod, shape, amp=0.5)
    hot = oracle_mod.phi4_init(oracle_mod.phi4_params(shape, DTAU, M2, LAM, 5), 50.0)
    phi0 = np.stack([quiet[0], hot, quiet[2]])
    dt = [0.01, 0.5, 0.01]
    with _ens(shape, 3, dtau=dt, seeds=SEEDS) as E:
        E.upload(phi0)
        E.step(3)
        got = E.download()
        assert list(E.flags()) == [False, True, False]
    with _lat(shape, dtau=0.5, m2=M2, lam=LAM, seed=SEEDS[1]) as L:
        L.upload(hot)
        L.step(3)
        assert np.array_equal(got[1], L.download())
    assert np.abs(got[1]).max() == 1000.0


def _exact_sums(phi):
    """Exactly rounded S1, S2, S4, NN of one lattice, max |phi|, and per sum the bound 2 n u sum |terms|."""
    a = phi.astype(np.float64)
    a2 = a * a                                     # exact: 24-bit factors
    links = np.concatenate([(a * np.roll(a, -1, axis=ax)).ravel() for ax in (2, 1, 0)])   # exact
    terms = [a.ravel(), a2.ravel(), (a2 * a2).ravel(), links]
    u = 2.0 ** -53
    sums = [math.fsum(t) for t in terms]
    bounds = [2 * t.size * u * math.fsum(np.abs(t)) for t in terms]
    return np.array(sums), np.array(bounds), float(np.abs(phi).max())


@pytest.mark.parametrize("shape", [(16, 4, 31), (32, 32, 32)] + MEASURED)
def test_series_and_moments(gpu, oracle_mod, shape):
    assert_shape(shape)
    phi0 = _starts(oracle_mod, shape)
    with _ens(shape, 3, seeds=SEEDS) as E, _ens(shape, 3, seeds=SEEDS) as Ref:
        E.upload(phi0)
        Ref.upload(phi0)
        ser = E.step(12, every=4)
        assert ser.shape == (3, 3, 4)
        worst = 0.0
        for m in range(3):
            Ref.step(4)
            f = Ref.download()
            for r in range(3):
                s, b, _ = _exact_sums(f[r])
                err = np.abs(ser[m, r] - s)
                worst = max(worst, float(np.max(err / b)))
                assert np.all(err <= b), f"record {m} replica {r}: err {err} bound {b}"
        assert np.array_equal(E.download(), f)     # measuring changes nothing
        mom = E.moments()
        for r in range(3):
            s, b, mx = _exact_sums(f[r])
            got = np.array([mom[k][r] for k in ("S1", "S2", "S4", "NN")])
            assert np.all(np.abs(got - s) <= b)
            assert mom["maxabs"][r] == mx
        one = E.moments(first=1, count=1)
        assert one["S2"][0] == mom["S2"][1] and one["maxabs"][0] == mom["maxabs"][1]
        print(f"SUMS {shape} worst err/bound = {worst:.3e}", flush=True)


def _incomplete_tail(oracle_mod, shape):
    assert_shape(shape)
    phi0 = _starts(oracle_mod, shape)
    with _ens(shape, 3, seeds=SEEDS) as E, _ens(shape, 3, seeds=SEEDS) as Ref:
        E.upload(phi0)
        Ref.upload(phi0)
        ser = E.step(12, every=5)
        assert ser.shape == (2, 3, 4)
        for m in range(2):
            Ref.step(5)
            f = Ref.download()
            for r in range(3):
                s, b, _ = _exact_sums(f[r])
                assert np.all(np.abs(ser[m, r] - s) <= b)
        Ref.step(2)
        assert np.array_equal(E.download(), Ref.download())
        assert E.step(3, every=5).shape == (0, 3, 4)
        assert E.step(2) is None


def test_series_drops_the_incomplete_tail(gpu, oracle_mod):
    _incomplete_tail(oracle_mod, (16, 4, 31))


@pytest.mark.parametrize("shape", MEASURED)
def test_series_drops_the_incomplete_tail_at(gpu, oracle_mod, shape):
    _incomplete_tail(oracle_mod, shape)


def test_ranges_and_errors(gpu):
    from stochquant_amd import StochQuantError
    shape = (8, 8, 8)
    with _ens(shape, 3) as E:
        for first, count in ((-1, 1), (0, 4), (3, 1), (2, 2), (0, -1)):
            with pytest.raises(StochQuantError) as ei:
                E.download(first=first, count=count)
            assert ei.value.code == -1
            with pytest.raises(StochQuantError):
                E.moments(first=first, count=count)
            with pytest.raises(StochQuantError):
                E.flags(first=first, count=count)
            with pytest.raises(StochQuantError):
                E.set_params(dtau=0.01, first=first, count=count)
        with pytest.raises(StochQuantError):
            E.upload(np.zeros((2, 8, 8, 8), np.float32), first=2)
        assert E.download(first=3, count=0).shape == (0, 8, 8, 8)
        before = E.get_params()
        # replica 1's values break dtau * drift(clamp) < 1e30: nothing changes, replica 0's valid ones included
        with pytest.raises(StochQuantError) as ei:
            E.set_params(dtau=[0.05, 0.01, 0.01], lam=[1.0, 1e25, 1.0])
        assert ei.value.code == -1
        with pytest.raises(StochQuantError):
            E.set_params(dtau=[0.01, float("nan"), 0.01])
        with pytest.raises(StochQuantError):
            E.dtau = -1.0
        after = E.get_params()
        for k in before:
            assert np.array_equal(before[k], after[k])
        with pytest.raises(StochQuantError):
            E.step(-1)
        E.dtau = [0.01, 0.02, 0.03]
        assert list(E.dtau) == [0.01, 0.02, 0.03]
