"""Gradient-flow measurements of the phi^4 ensemble on the GPU
(sq_phi4_ens_set_flow / _step_flow / _flowed / _flow_field / _fcorr_sums /
_fcorr_reset / _fcorrelator; Phi4Ensemble.set_flow, step(flow=True), flowed,
flow_field, fcorr_sums, fcorr_reset, fcorrelator).

Definitions (include/stochquant.h): the flowed field at level n is the noise-off
site update applied n times to a copy of the replica's field with the flow
coefficients (h = eps, the flow's m2 and lambda, sig = 0); a measurement at a
level is the existing one of that field.  So every number is pinned bit for bit
by composing calls that exist: a second ensemble with C = 0 and dtau = eps,
moments(), slices(), and oracle.phi4_step with C = 0.

Tolerances: everything bit for bit, except
  * the plane wave: S2 after 8 heat-equation steps against the exact decay
    within 1e-4 relative -- eight steps of at most about eight fp32 roundings
    each on the amplitude stay under 2e-5 relative (8 * 8 * 2^-24 = 4e-6 by
    the count alone), doubled for the square: a margin of 2.5 to 5;
  * the free field: the replica mean of the time-averaged S2 / V within 4
    standard errors of the Euler scheme's exact stationary value at flow level
    n, (1/V) sum_k (1 - eps k^2)^(2n) / (w_k (1 - dtau w_k / 2)), w_k = k^2 + m2,
    k^2 = sum_mu (2 - 2 cos k_mu): the rule of the other stationary-law tests.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_phi4_ens_corr import SHAPES as CORR_SHAPES
from test_phi4_ens_shapes import GPU_SHAPES, assert_shape

pytestmark = pytest.mark.gpu

SEEDS = [1234, 99, 0xDEADBEEF12345]
DTAU = [0.02, 0.015, 0.01]
M2 = [0.5, -0.2, 1.0]
LAM = [1.0, 0.7, 2.0]
EPS = 0.05
LEVELS = (0, 1, 3, 6)

_cache = {}


def _ens(shape, R=3, **kw):
    from stochquant_amd import Phi4Ensemble
    kw.setdefault("dtau", DTAU[:R] if R <= 3 else DTAU[0])
    kw.setdefault("m2", M2[:R] if R <= 3 else M2[0])
    kw.setdefault("lam", LAM[:R] if R <= 3 else LAM[0])
    kw.setdefault("seeds", SEEDS[:R] if R <= 3 else None)
    return Phi4Ensemble(shape, R, **kw)


def _starts(oracle_mod, shape, amp=0.9, seeds=(77, 78, 79)):
    """Distinct start fields, one per replica (computed once per shape, read-only)."""
    key = ("start", shape)
    if key not in _cache:
        a = np.stack([oracle_mod.phi4_init(oracle_mod.phi4_params(shape, DTAU[0], M2[0], LAM[0], s), amp)
                      for s in seeds])
        a.setflags(write=False)
        _cache[key] = a
    return _cache[key]


def _s1_host(S):
    s = 0.0
    for v in S:
        s = s + float(v)
    return s


def _twin(shape, phi, m2, lam, steps):
    """The composition: a C = 0 ensemble with dtau = eps and the flow's m2, lambda, uploaded with phi and stepped
    steps[0], steps[1], ... in turn; moments()[:4] and slices() after each."""
    out = []
    with _ens(shape, 3, dtau=EPS, m2=m2, lam=lam, C=0.0) as T:
        T.upload(phi)
        for k in steps:
            T.step(k)
            m = T.moments()
            S, g = T.slices()
            out.append((np.stack([m["S1"], m["S2"], m["S4"], m["NN"]], axis=1), S, g))
        assert list(T.step_counter) == [sum(steps)] * 3
    return out


@pytest.mark.parametrize("own", [True, False], ids=["own", "shared"])
@pytest.mark.parametrize("shape", sorted(GPU_SHAPES))
def test_composition(gpu, oracle_mod, shape, own):
    assert_shape(shape)
    phi0 = _starts(oracle_mod, shape)
    with _ens(shape) as E:
        E.upload(phi0)
        E.step(2)                                    # a field the noise has touched, counters off zero
        phi, cnt, flg = E.download(), E.step_counter, E.flags()
        if own:
            E.set_flow(EPS, LEVELS)
            fm2, flam = M2, LAM
        else:
            E.set_flow(EPS, LEVELS, m2=0.3, lam=0.0)
            fm2, flam = 0.3, 0.0
        assert E.flow == {"eps": EPS, "levels": LEVELS, "m2": None if own else 0.3, "lam": None if own else 0.0}
        sums, S, g = E.flowed()
        assert sums.shape == (3, 4, 4) and S.shape == (3, 4, shape[2]) and g.shape == (3, 4, shape[2] // 2 + 1)
        ref = _twin(shape, phi, fm2, flam, [0, 1, 2, 3])
        for l, (rs, rS, rg) in enumerate(ref):
            assert np.array_equal(sums[:, l], rs), (l, np.max(np.abs(sums[:, l] - rs)))
            assert np.array_equal(S[:, l], rS), l
            assert np.array_equal(g[:, l], rg), l
        assert not np.array_equal(sums[:, 0], sums[:, 3])
        # a sub-range, and the simulation untouched
        s1, S1, g1 = E.flowed(first=1, count=2)
        assert np.array_equal(s1, sums[1:]) and np.array_equal(S1, S[1:]) and np.array_equal(g1, g[1:])
        assert np.array_equal(E.download(), phi)
        assert np.array_equal(E.step_counter, cnt) and np.array_equal(E.flags(), flg)


@pytest.mark.parametrize("shape", [(8, 2, 2), (16, 4, 31), (64, 16, 8), (32, 32, 32)])
def test_flow_field_against_the_oracle(gpu, oracle_mod, shape):
    phi0 = _starts(oracle_mod, shape)
    with _ens(shape) as E:
        E.upload(phi0)
        E.set_flow(EPS, (0,))
        got = E.flow_field(5)
        assert np.array_equal(E.flow_field(0), phi0)
        assert np.array_equal(E.flow_field(5, first=2, count=1), got[2:])
        assert np.array_equal(E.download(), phi0)
    for r in range(3):
        p = oracle_mod.phi4_params(shape, EPS, M2[r], LAM[r], SEEDS[r], C=0.0)
        ref = phi0[r]
        for k in range(5):
            ref = oracle_mod.phi4_step(p, ref, k)
        assert np.array_equal(got[r], ref), (r, np.max(np.abs(got[r] - ref)))


IN_FLIGHT_LEVELS = (0, 2, 5)     # an odd last level: the flow ends in the other image than it started in


@pytest.mark.parametrize("shape", CORR_SHAPES)
def test_in_flight_equals_stand_alone(gpu, oracle_mod, shape):
    phi0 = _starts(oracle_mod, shape)
    F = len(IN_FLIGHT_LEVELS)

    def fresh():
        E = _ens(shape)
        E.upload(phi0)
        E.set_flow(EPS, IN_FLIGHT_LEVELS)
        return E

    with fresh() as A, fresh() as B, fresh() as C:
        ser = A.step(6, every=3, flow=True, correlate=True)
        assert ser.shape == (2, F, 3, 4)
        G = np.zeros((3, F, A.nt))
        S1 = np.zeros((3, F))
        for k in range(2):
            B.step(3)
            sums, S, g = B.flowed()
            assert np.array_equal(ser[k], sums.transpose(1, 0, 2)), k
            G = G + g
            S1 = S1 + np.array([[_s1_host(S[r, l]) for l in range(F)] for r in range(3)])
        GA, SA, nA = A.fcorr_sums()
        assert list(nA) == [2, 2, 2]
        assert np.array_equal(GA, G), np.max(np.abs(GA - G))
        assert np.array_equal(SA, S1)
        C.step(6)
        ref = C.download()
        for E in (A, B):
            assert np.array_equal(E.download(), ref)
            assert list(E.step_counter) == [6, 6, 6]
            assert np.array_equal(E.flags(), C.flags())
        # the plain accumulators do not advance in a flow call
        Gp, Sp, nP = A.corr_sums()
        assert not nP.any() and not Gp.any() and not Sp.any()
        # the series alone (the instance without the correlator) gives the same sums and accumulates nothing
        ser2 = C.step(3, every=3, flow=True)
        B.step(3)
        assert np.array_equal(ser2[0], B.flowed()[0].transpose(1, 0, 2))
        assert not C.fcorr_sums()[2].any()
        assert np.array_equal(C.download(), B.download())
        # statistics: the plain correlator's rule per level
        mean, err, used = A.fcorrelator()
        assert mean.shape == err.shape == (F, A.nt) and used == 3


@pytest.mark.parametrize("shape", [(8, 2, 2), (16, 4, 31)])
def test_additivity_and_independence(gpu, oracle_mod, shape):
    phi0 = _starts(oracle_mod, shape)

    def fresh(levels=LEVELS):
        E = _ens(shape)
        E.upload(phi0)
        E.set_flow(EPS, levels)
        return E

    with fresh() as A, fresh() as B:
        sa = A.step(6, every=3, flow=True, correlate=True)
        sb = np.concatenate([B.step(3, every=3, flow=True, correlate=True) for _ in range(2)])
        assert np.array_equal(sa, sb)
        for x, y in zip(A.fcorr_sums(), B.fcorr_sums()):
            assert np.array_equal(x, y)
        assert list(A.fcorr_sums()[2]) == [2, 2, 2]
        assert A.step(2, every=3, flow=True, correlate=True).shape == (0, 4, 3, 4)   # an incomplete tail
        assert list(A.fcorr_sums()[2]) == [2, 2, 2] and list(A.step_counter) == [8, 8, 8]
        # fcorr_reset clears its range only; set_flow clears everything
        G0, S0, _ = B.fcorr_sums()
        B.fcorr_reset(first=1, count=1)
        G1, S1, n1 = B.fcorr_sums()
        assert list(n1) == [2, 0, 2] and not G1[1].any() and not S1[1].any()
        assert np.array_equal(G1[[0, 2]], G0[[0, 2]]) and np.array_equal(S1[[0, 2]], S0[[0, 2]])
        G2, S2, n2 = B.fcorr_sums(first=2, count=1)
        assert np.array_equal(G2, G0[2:]) and np.array_equal(S2, S0[2:]) and list(n2) == [2]
        B.set_flow(EPS, LEVELS)
        G3, S3, n3 = B.fcorr_sums()
        assert not G3.any() and not S3.any() and not n3.any()

    # replica r of an R = 5 handle is the R = 1 handle of its seed
    seeds5 = [500 + r for r in range(5)]
    with _ens(shape, 5, seeds=seeds5) as E, _ens(shape, 1, seeds=[seeds5[3]], dtau=DTAU[0], m2=M2[0],
                                                 lam=LAM[0]) as O:
        for X in (E, O):
            X.upload(phi0[0])
            X.set_flow(EPS, LEVELS, m2=0.3, lam=0.0)
        se = E.step(6, every=2, flow=True, correlate=True)
        so = O.step(6, every=2, flow=True, correlate=True)
        assert np.array_equal(se[:, :, 3], so[:, :, 0])
        for x, y in zip(E.fcorr_sums(first=3, count=1), O.fcorr_sums()):
            assert np.array_equal(x, y)
        assert np.array_equal(E.download(first=3, count=1), O.download())

    # levels = (0,): the plain call's series and the plain correlator's accumulator values
    with fresh((0,)) as A, fresh((0,)) as P:
        sa = A.step(6, every=3, flow=True, correlate=True)
        sp = P.step(6, every=3, correlate=True)
        assert np.array_equal(sa[:, 0], sp)
        GA, SA, nA = A.fcorr_sums()
        GP, SP, nP = P.corr_sums()
        assert np.array_equal(GA[:, 0], GP) and np.array_equal(SA[:, 0], SP) and np.array_equal(nA, nP)
        assert np.array_equal(A.download(), P.download())
        for conn in (True, False):
            ma, ea, ua = A.fcorrelator(connected=conn)
            mp, ep, up = P.correlator(connected=conn)
            assert np.array_equal(ma[0], mp) and np.array_equal(ea[0], ep) and ua == up == 3


def _state(E):
    return (E.flow, [a.copy() for a in E.fcorr_sums()], E.download(), list(E.step_counter), E.get_params())


def _same_state(a, b):
    assert a[0] == b[0] and a[3] == b[3]
    assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1])) and np.array_equal(a[2], b[2])
    assert all(np.array_equal(a[4][k], b[4][k]) for k in a[4])


def test_arguments(gpu, oracle_mod):
    from stochquant_amd import StochQuantError, _lib
    lib = _lib.load()
    shape = (8, 2, 2)
    phi0 = _starts(oracle_mod, shape)

    def ints(*v):
        return (ctypes.c_int * len(v))(*v)

    with _ens(shape) as E:
        E.upload(phi0)
        # no flow yet
        assert E.flow is None
        assert lib.sq_phi4_ens_step_flow(E._h, 4, 2, None, 1) == -4
        with pytest.raises(StochQuantError) as ei:
            E.step(4, every=2, flow=True)
        assert ei.value.code == -4
        for fn in (E.flowed, E.fcorr_sums, E.fcorrelator, lambda: E.flow_field(1)):
            with pytest.raises(StochQuantError) as ei:
                fn()
            assert ei.value.code == -4
        assert list(E.step_counter) == [0, 0, 0] and np.array_equal(E.download(), phi0)
        E.set_flow(EPS, (0, 2))
        E.step(4, every=2, flow=True, correlate=True)
        before = _state(E)
        assert list(before[1][2]) == [2, 2, 2]
        nan = float("nan")
        for eps, lev in ((EPS, (3, 3)), (EPS, (5, 2)), (EPS, (-1, 2)), (EPS, (0, 4097)), (EPS, (0, 1, 2, 3, 4)),
                         (0.0, (0, 2)), (-0.05, (0, 2)), (nan, (0, 2)), (float("inf"), (0, 2))):
            assert lib.sq_phi4_ens_set_flow(E._h, eps, len(lev), ints(*lev), None, None) == -1, (eps, lev)
            _same_state(before, _state(E))
        assert lib.sq_phi4_ens_set_flow(E._h, EPS, 2, None, None, None) == -1
        assert lib.sq_phi4_ens_set_flow(E._h, EPS, -1, ints(0), None, None) == -1
        bad = ctypes.c_double(nan)
        assert lib.sq_phi4_ens_set_flow(E._h, EPS, 2, ints(0, 2), ctypes.byref(bad), None) == -1
        assert lib.sq_phi4_ens_set_flow(E._h, EPS, 2, ints(0, 2), None, ctypes.byref(bad)) == -1
        assert lib.sq_phi4_ens_step_flow(E._h, -1, 2, None, 1) == -1
        assert lib.sq_phi4_ens_step_flow(E._h, 4, 0, None, 1) == -1
        assert lib.sq_phi4_ens_flow_field(E._h, 0, 3, 4097, None) == -1
        assert lib.sq_phi4_ens_flow_field(E._h, 0, 3, -1, None) == -1
        assert lib.sq_phi4_ens_flowed(E._h, 2, 2, None, None, None) == -1      # a range past the last replica
        with pytest.raises(StochQuantError):
            E.fcorrelator(n=E.nt + 1)
        _same_state(before, _state(E))
        for kw in (dict(every=0), dict(every=2, momenta=True, correlate=True), dict(every=2, scheme="heun")):
            with pytest.raises(ValueError):
                E.step(4, flow=True, **kw)
        _same_state(before, _state(E))
        # the largest level allowed runs
        E.set_flow(EPS, (4096,), m2=0.0, lam=0.0)
        assert E.flowed()[0].shape == (3, 1, 4)
        # a set_params that would make a replica's flow record illegal is refused: with clamp = 1000 and
        # lambda = 3e23 the replica's own step (dtau = 0.01) keeps dtau * drift(clamp) = 5e29 < 1e30 and the
        # flow step eps = 0.05 does not (2.5e30)
        E.set_flow(EPS, (0, 2))
        E.set_params(dtau=0.01)
        before = _state(E)
        with pytest.raises(StochQuantError) as ei:
            E.set_params(lam=[1.0, 3e23, 1.0])
        assert ei.value.code == -1
        _same_state(before, _state(E))
        E.set_flow(EPS, (0, 2), lam=0.5)             # the flow's own lambda: the replica's no longer matters
        E.set_params(lam=[1.0, 3e23, 1.0])
        with pytest.raises(StochQuantError) as ei:   # ... and cannot be handed back to the flow
            E.set_flow(EPS, (0, 2))
        assert ei.value.code == -1
        assert E.flow["lam"] == 0.5
        E.set_flow(None)
        assert E.flow is None
        assert lib.sq_phi4_ens_step_flow(E._h, 4, 2, None, 1) == -4


def test_plane_wave_decay(gpu):
    """m2 = lambda = 0: the flow is the lattice heat equation, and a plane wave of momentum k decays by
    1 - eps k^2 per step, k^2 = 2 - 2 cos(2 pi / 8) = 2 - sqrt 2."""
    shape, eps, n = (8, 4, 4), 0.1, 8
    x = np.arange(8)
    phi = np.broadcast_to(np.cos(2.0 * np.pi * x / 8.0).astype(np.float32), (4, 4, 8))
    with _ens(shape, 1, dtau=0.01, m2=1.0, lam=1.0, seeds=[5]) as E:
        E.upload(phi)
        E.set_flow(eps, (0, n), m2=0.0, lam=0.0)
        sums, _, _ = E.flowed()
    want = (1.0 - eps * (2.0 - np.sqrt(2.0))) ** (2 * n)
    got = sums[0, 1, 1] / sums[0, 0, 1]
    print(f"flow plane wave: S2 ratio {got:.9f}, exact {want:.9f}, relative error {abs(got / want - 1):.3g}")
    assert abs(sums[0, 0, 1] - 64.0) <= 64.0 * 1e-6          # sum cos^2 = V / 2
    assert abs(got / want - 1.0) <= 1e-4


def _free_exact(shape, dtau, m2, eps, n):
    Lx, Ly, Lz = shape
    k2 = sum(np.meshgrid(*[2.0 - 2.0 * np.cos(2.0 * np.pi * np.arange(L) / L) for L in (Lx, Ly, Lz)],
                         indexing="ij"))
    w = k2 + m2
    return float(np.sum((1.0 - eps * k2) ** (2 * n) / (w * (1.0 - dtau * w / 2.0))) / (Lx * Ly * Lz))


def test_free_field_flowed_law(gpu):
    """lambda = 0: the Euler scheme's stationary <phi^2> is known in closed form, and the heat-equation flow
    multiplies mode k by (1 - eps k^2)^n.  A flow that ran a step too many or too few, or with the wrong
    step, misses the level-4 value by many standard errors; the seeds are fixed."""
    shape, R, dtau, m2, eps = (8, 4, 4), 512, 0.05, 1.0, 0.05
    exact = [_free_exact(shape, dtau, m2, eps, n) for n in (0, 4)]
    assert np.allclose(exact, [0.2031735, 0.0411439], atol=1e-6), exact
    V = float(shape[0] * shape[1] * shape[2])
    with _ens(shape, R, dtau=dtau, m2=m2, lam=0.0, C=1.0, seeds=[3000 + r for r in range(R)]) as E:
        E.step(400)
        E.set_flow(eps, (0, 4), m2=0.0, lam=0.0)
        ser = E.step(2000, every=20, flow=True)
        assert ser.shape == (100, 2, R, 4) and not E.flags().any()
    per = ser[:, :, :, 1].mean(axis=0) / V               # (2, R): each replica's time average
    mean = per.mean(axis=1)
    err = per.std(axis=1, ddof=1) / np.sqrt(R)
    print("flow free field: level 0 / 4 mean", mean, "exact", exact, "(mean - exact) / err", (mean - exact) / err)
    assert np.all(np.abs(mean - exact) <= 4.0 * err), (mean, exact, err)
