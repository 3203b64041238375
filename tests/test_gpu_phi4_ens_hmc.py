"""The phi^4 ensemble's hybrid Monte Carlo trajectories on the GPU (phi4_ens_hmc_kernel, sq_phi4_ens_step_hmc,
Phi4Ensemble.step_hmc) against an oracle composed here from the header's definition: the first leapfrog step
from oracle.phi4_step (device normals: bit for bit), every interior step from oracle.phi4_step at step size 2h
with C = 0 and a float32 NumPy displacement add, the uniform and the length from oracle.philox, dH in NumPy
float64 with math.fsum.

Parameters: the seeds, m2 and lambda of test_gpu_phi4_ens_heun.py's three replicas at C = [0.7, 1.0, 0.5] (the
MALA test's), fields thermalised with 100 Euler steps, dtau = round(0.4 / sqrt(V), 5) at nleap = 3, where a
float32 NumPy model of the definition accepts 0.39 - 0.72 of the trajectories from V = 32 to 32,768.

Tolerances.  Fields, uniforms, verdicts, lengths, counters, flags and counts: exact.  dH against the float64
formula: 1e-10 A, A the sum of the absolute values of all summed terms over sig^2 (test_gpu_phi4_ens_mala.py
derives it: the kernel sums the same two fields' terms in the same way, whatever L).  The verdict is checked
against the kernel's own dH with NumPy's exp; a trajectory with |exp(-dH) - u| < 1e-12 could not be decided
across two exp implementations, and there must be none (on a hit: another seed, not another bound).  The
physics test's bounds are derived at the test.
"""
import math

import numpy as np
import pytest

from test_gpu_phi4_ens_heun import CLAMP, LAM, M2, SEEDS, _free_phi2
from test_gpu_phi4_ens_mala import COUNTERS, CS, STREAM_ACCEPT, THERM, _record
from test_oracle import same_bits
from test_phi4_ens_shapes import GPU_SHAPES, assert_shape

pytestmark = pytest.mark.gpu

SHAPES = list(GPU_SHAPES)
NLEAP = 3
# one shape per (K, images) class of the step launch, and a second one of the smallest and the largest
CLASS_SHAPES = [(8, 2, 2), (8, 8, 8), (64, 16, 8), (16, 24, 24), (32, 24, 24), (64, 11, 29), (32, 32, 32)]

_cache = {}


def _dtau(shape):
    return round(0.4 / math.sqrt(shape[0] * shape[1] * shape[2]), 5)


def _ens(shape, R=3, **kw):
    from stochquant_amd import Phi4Ensemble
    kw.setdefault("dtau", _dtau(shape))
    kw.setdefault("m2", M2[:R])
    kw.setdefault("lam", LAM[:R])
    kw.setdefault("C", CS[:R])
    kw.setdefault("seeds", SEEDS[:R])
    kw.setdefault("clamp", CLAMP)
    return Phi4Ensemble(shape, R, **kw)


def _params(shape, r):
    return (_dtau(shape), M2[r], LAM[r], CS[r], SEEDS[r])


def accept_block(o, seed, s):
    return o.philox([0, STREAM_ACCEPT << 24, s & 0xFFFFFFFF, s >> 32], [seed & 0xFFFFFFFF, seed >> 32])


def length(o, seed, s, nleap, randomize):
    """The definition's L: nleap, or 1 + ((uint64) o.y nleap >> 32)."""
    if not randomize:
        return nleap
    return 1 + ((int(accept_block(o, seed, s)[1]) * nleap) >> 32)


def guard(v, clamp):
    """The update's guard on a float32 array: NaN -> +clamp, else clipped (fminf / fmaxf drop the NaN)."""
    cl = np.float32(clamp)
    return np.fmax(np.fmin(v, cl), -cl).astype(np.float32)


def reaches(f, clamp):
    with np.errstate(invalid="ignore"):
        return not bool(np.max(np.abs(f)) < np.float32(clamp))


def trajectory(o, shape, par, phi0, s, L, clamp=CLAMP):
    """The definition's steps 2 and 3: (phi_1, phi_{L-1}, phi_L, some phi_1, g or phi_k reached the clamp)."""
    dtau, m2, lam, C, seed = par
    P = o.phi4_params(shape, dtau, m2, lam, seed, clamp=clamp, C=C)
    P2 = o.phi4_params(shape, 2.0 * float(np.float32(dtau)), m2, lam, seed, clamp=clamp, C=0.0)
    phi1 = o.phi4_step(P, phi0, s)
    hit = reaches(phi1, clamp)
    prev, cur = phi0, phi1
    for _ in range(1, L):
        g = o.phi4_step(P2, cur, s)
        t = (cur - prev).astype(np.float32)
        nxt = guard(g + t, clamp)
        hit = hit or reaches(g, clamp) or reaches(nxt, clamp)
        prev, cur = cur, nxt
    return phi1, prev, cur, hit


def dH_reference(phi0, phi1, phim, phiL, rec):
    """(dH, A) of the header's formula in float64, exactly rounded sums (math.fsum) of every term."""
    h, m2, lam6, sig = rec
    f, f1, gm, g = (x.astype(np.float64) for x in (phi0, phi1, phim, phiL))

    def fwd(x):
        return [np.roll(x, -1, axis=a) for a in (2, 1, 0)]

    def drift(x):
        nb = sum(np.roll(x, d, axis=a) for a in (0, 1, 2) for d in (1, -1))
        return nb - 6.0 * x - x * (m2 + lam6 * x * x)

    a = f1 - f - h * drift(f)
    b = gm - g - h * drift(g)
    km, l4 = 3.0 + 0.5 * m2, 0.25 * lam6
    terms = [2.0 * h * km * g * g, -2.0 * h * km * f * f, 2.0 * h * l4 * g ** 4, -2.0 * h * l4 * f ** 4,
             0.5 * b * b, -0.5 * a * a]
    terms += [-2.0 * h * g * n for n in fwd(g)] + [2.0 * h * f * n for n in fwd(f)]
    flat = np.concatenate([t.ravel() for t in terms])
    s2 = sig * sig
    return math.fsum(flat) / s2, math.fsum(np.abs(flat)) / s2


def check_trajectories(o, shape, par, phi, s0, rec, nleap, randomize, clamp=CLAMP):
    """Follow one replica through the records of a call from field phi at counter s0: every record against the
    oracle; returns (the field after each trajectory, the verdicts, the lengths)."""
    dtau, m2, lam, C, seed = par
    R = _record(dtau, m2, lam, C)
    fields, verdicts, lengths = [], [], []
    for k in range(rec.shape[0]):
        dH, u, v, Lk = (float(x) for x in rec[k])
        s = s0 + k
        L = length(o, seed, s, nleap, randomize)
        assert Lk == float(L), (shape, k, Lk, L)
        assert u == (int(accept_block(o, seed, s)[0]) + 0.5) * 2.0 ** -32, (shape, k, u)
        phi1, phim, phiL, hit = trajectory(o, shape, par, phi, s, L, clamp)
        assert (v == 2.0) == hit, (shape, k, v)
        if not hit:
            ref, A = dH_reference(phi, phi1, phim, phiL, R)
            assert abs(dH - ref) <= 1e-10 * A, (shape, k, dH, ref, A)
            with np.errstate(over="ignore"):
                e = float(np.exp(-dH))
            assert abs(e - u) >= 1e-12, ("undecidable across exp implementations: change the seed", shape, k, e, u)
            assert v == float(dH <= 0.0 or u < e), (shape, k, dH, u, v)
        if v == 1.0:
            phi = phiL
        fields.append(phi)
        verdicts.append(int(v))
        lengths.append(L)
    return fields, verdicts, lengths


def _run_calls(o, shape, calls, nleap, randomize):
    """Calls of `calls` trajectories with records from thermalised fields at COUNTERS, everything against the
    oracle; returns (verdicts, lengths) of all replicas."""
    assert_shape(shape)
    with _ens(shape) as E:
        E.init_field(0.5)
        E.step(THERM)
        E.step_counter = COUNTERS
        start = E.download()
        assert not E.flags().any()
        recs, after = [], []
        for n in calls:
            ser, rec = E.step_hmc(n, nleap=nleap, randomize=randomize, record=True)
            assert ser is None and rec.shape == (n, 3, 4)
            recs.append(rec)
            after.append(E.download())
        assert [int(s) for s in E.step_counter] == [c + sum(calls) for c in COUNTERS]
        flags = E.flags()
        stats = E.hmc_stats()
        assert not E.mala_stats().any()
    rec = np.concatenate(recs)
    out, lens = [], []
    for r in range(3):
        fields, verdicts, lengths = check_trajectories(o, shape, _params(shape, r), start[r], COUNTERS[r], rec[:, r],
                                                       nleap, randomize)
        done = 0
        for n, got in zip(calls, after):
            done += n
            assert same_bits(got[r], fields[done - 1]), f"replica {r} after trajectory {done}: " \
                f"{np.count_nonzero(got[r] != fields[done - 1])} sites differ"
        assert list(stats[r]) == [sum(calls), verdicts.count(1), verdicts.count(2), sum(lengths)], \
            (r, stats[r], verdicts, lengths)
        assert bool(flags[r]) == (2 in verdicts) and 2 not in verdicts, (r, flags, verdicts)
        out.append(verdicts)
        lens.append(lengths)
    print(f"HMC {shape} dtau {_dtau(shape)} nleap {nleap} randomize {randomize} verdicts {out} lengths {lens}",
          flush=True)
    return out, lens


def _run_shape(o, shape):
    """The oracle test of one shape, once: calls of 3, 1, 1, 1 trajectories of three steps."""
    if shape not in _cache:
        _cache[shape] = _run_calls(o, shape, (3, 1, 1, 1), NLEAP, False)[0]
    return _cache[shape]


@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_composed_oracle(gpu, dev_oracle, shape):
    _run_shape(dev_oracle, shape)


def test_both_verdicts_in_every_work_group_class(gpu, dev_oracle):
    """Over the shapes above, every (K, images) class has accepted and rejected trajectories."""
    seen = {}
    for shape in SHAPES:
        K, _, images, _ = GPU_SHAPES[shape]
        seen.setdefault((K, images), set()).update(v for vs in _run_shape(dev_oracle, shape) for v in vs)
    assert {k for k, _ in seen} == {1, 2, 4, 8} and (8, 1) in seen and (8, 2) in seen
    for cls, vs in seen.items():
        assert {0, 1} <= vs, (cls, vs)


@pytest.mark.parametrize("shape", CLASS_SHAPES)
def test_one_leapfrog_step_is_mala(gpu, shape):
    """step_hmc(6, nleap=1), with and without randomize, against a twin's step_mala(6): the same bits."""
    assert_shape(shape)
    assert {GPU_SHAPES[s][0::2] for s in CLASS_SHAPES} == {GPU_SHAPES[s][0::2] for s in GPU_SHAPES}
    with _ens(shape) as M, _ens(shape) as H, _ens(shape) as Hr:
        for E in (M, H, Hr):
            E.init_field(0.5)
            E.step(THERM)
            E.step_counter = COUNTERS
        _, rm = M.step_mala(6, record=True)
        want = M.download()
        assert (rm[:, :, 2] == 0.0).any() or (rm[:, :, 2] == 1.0).any()
        for E, rnd in ((H, False), (Hr, True)):
            _, rh = E.step_hmc(6, nleap=1, randomize=rnd, record=True)
            assert np.array_equal(rh[:, :, :3].view(np.uint64), rm.view(np.uint64)), rnd
            assert (rh[:, :, 3] == 1.0).all()
            assert same_bits(E.download(), want), rnd
            assert list(E.step_counter) == list(M.step_counter) and list(E.flags()) == list(M.flags())
            st = E.hmc_stats()
            assert np.array_equal(st[:, :3], M.mala_stats()) and st[:, 3].tolist() == [6, 6, 6]
            assert not E.mala_stats().any() and not M.hmc_stats().any()


@pytest.mark.parametrize("shape", [(8, 8, 8), (32, 24, 24), (64, 11, 29)])
def test_randomised_lengths(gpu, dev_oracle, shape):
    """nleap = 5 with randomize: every recorded L is the formula's, several lengths occur, the oracle is followed
    with those lengths (check_trajectories), and the fourth counter is their sum (_run_calls)."""
    _, lens = _run_calls(dev_oracle, shape, (8,), 5, True)
    assert len({L for ls in lens for L in ls}) >= 2, lens
    assert all(1 <= L <= 5 for ls in lens for L in ls)


@pytest.mark.parametrize("shape", [(8, 8, 8), (32, 32, 32)])
def test_invariances(gpu, shape):
    """A call of 6 trajectories is calls of 3 + 1 + 2; a replica of three is the same replica alone; calls of the
    four schemes alternate on one handle with every counter as expected; every=2 returns the moments() of the
    fields held at those points and correlate=True adds what slices() of those fields gives."""
    assert_shape(shape)
    with _ens(shape) as A, _ens(shape) as B, _ens(shape) as M, _ens(shape) as S:
        for E in (A, B, M, S):
            E.init_field(0.5)
            E.step(THERM)
            E.step_counter = COUNTERS
        _, ra = A.step_hmc(6, nleap=NLEAP, record=True)
        rb = [B.step_hmc(n, nleap=NLEAP, record=True)[1] for n in (3, 1, 2)]
        assert np.array_equal(ra.view(np.uint64), np.concatenate(rb).view(np.uint64))
        assert same_bits(A.download(), B.download())
        assert np.array_equal(A.hmc_stats(), B.hmc_stats()) and A.hmc_stats()[:, 0].tolist() == [6, 6, 6]
        assert A.hmc_stats()[:, 3].tolist() == [6 * NLEAP] * 3
        assert list(A.step_counter) == list(B.step_counter) == [c + 6 for c in COUNTERS]
        got = A.download()
        for r in range(3):
            with _ens(shape, 1, m2=M2[r:r + 1], lam=LAM[r:r + 1], C=CS[r:r + 1], seeds=SEEDS[r:r + 1]) as One:
                One.init_field(0.5)
                One.step(THERM)
                One.step_counter = COUNTERS[r:r + 1]
                _, r1 = One.step_hmc(6, nleap=NLEAP, record=True)
                assert same_bits(got[r], One.download()[0]), f"replica {r}"
                assert np.array_equal(ra[:, r].view(np.uint64), r1[:, 0].view(np.uint64)), f"replica {r}"
                assert np.array_equal(A.hmc_stats()[r], One.hmc_stats()[0])
        # the four schemes on one handle against twins that get the field and the counters by upload
        seq = [("hmc", 2), ("mala", 2), ("heun", 1), ("hmc", 1), ("euler", 2), ("hmc", 2)]
        field, cnt = M.download(), np.array(COUNTERS, dtype=np.uint64)
        steps = 0
        for scheme, n in seq:
            run = (lambda E: E.step_hmc(n, nleap=NLEAP)) if scheme == "hmc" else (lambda E: E.step(n, scheme=scheme))
            run(M)
            steps += n
            with _ens(shape) as T:
                T.upload(field)
                T.step_counter = cnt
                run(T)
                field, cnt = T.download(), T.step_counter
            assert same_bits(M.download(), field), (scheme, n)
            assert list(M.step_counter) == list(cnt) == [c + steps for c in COUNTERS]
        assert M.hmc_stats()[:, 0].tolist() == [5, 5, 5] and M.mala_stats()[:, 0].tolist() == [2, 2, 2]
        assert M.perf()["steps"] == 3 * (THERM + steps)
        M.hmc_reset(1, 1)
        assert M.hmc_stats()[:, 0].tolist() == [5, 0, 5] and M.mala_stats()[:, 0].tolist() == [2, 2, 2]
        # measurements in flight
        with _ens(shape) as Q:
            Q.upload(S.download())
            Q.step_counter = COUNTERS
            ser, rec = S.step_hmc(6, nleap=NLEAP, every=2, correlate=True, record=True)
            assert ser.shape == (3, 3, 4)
            G, S1 = np.zeros((3, S.nt)), np.zeros(3)
            for m in range(3):
                Q.step_hmc(2, nleap=NLEAP)
                mom = Q.moments()
                row = np.stack([mom[k] for k in ("S1", "S2", "S4", "NN")], axis=1)
                assert np.array_equal(ser[m].view(np.uint64), row.view(np.uint64)), f"record {m}"
                Sz, g = Q.slices()
                G = G + g
                s1 = np.zeros(3)
                for z in range(shape[2]):
                    s1 = s1 + Sz[:, z]
                S1 = S1 + s1
            aG, aS1, aN = S.corr_sums()
            assert np.array_equal(aG.view(np.uint64), G.view(np.uint64))
            assert np.array_equal(aS1.view(np.uint64), S1.view(np.uint64))
            assert list(aN) == [3, 3, 3]
            assert same_bits(S.download(), Q.download()) and same_bits(S.download(), A.download())
            assert np.array_equal(rec.view(np.uint64), ra.view(np.uint64))


@pytest.mark.parametrize("shape", [(8, 8, 8), (32, 32, 32)])
def test_guard_trip_rejects_and_flags(gpu, dev_oracle, shape):
    """Replica 0: a field at 9.9 everywhere under clamp 10 with noise of width 0.32: the first step reaches the
    clamp.  Verdict 2, the field unchanged bit for bit, the flag set, the counter advanced.  Replica 1, quiet, is
    what it is alone."""
    from stochquant_amd import Phi4Ensemble
    assert_shape(shape)
    kw = dict(dtau=0.05, m2=0.05, lam=0.0, C=1.0, clamp=10.0)
    with Phi4Ensemble(shape, 2, seeds=[1, 2], **kw) as E, Phi4Ensemble(shape, 1, seeds=[2], **kw) as One:
        E.init_field(0.5)
        start = E.download()
        start[0] = np.float32(9.9)
        E.upload(start)
        One.upload(start[1:])
        ser, rec = E.step_hmc(1, nleap=NLEAP, record=True)
        _, rec1 = One.step_hmc(1, nleap=NLEAP, record=True)
        got = E.download()
        assert list(E.flags()) == [True, False] and list(E.step_counter) == [1, 1]
        assert E.hmc_stats().tolist() == [[1, 0, 1, NLEAP], [1, int(rec[0, 1, 2]), 0, NLEAP]]
        assert same_bits(got[1], One.download()[0])
        assert np.array_equal(rec[0, 1].view(np.uint64), rec1[0, 0].view(np.uint64))
    P = dev_oracle.phi4_params(shape, 0.05, 0.05, 0.0, 1, clamp=10.0, C=1.0)
    assert np.max(np.abs(dev_oracle.phi4_step(P, start[0], 0))) == np.float32(10.0)
    assert rec[0, 0, 2] == 2.0 and rec[0, 0, 3] == NLEAP and same_bits(got[0], start[0])
    fields, verdicts, _ = check_trajectories(dev_oracle, shape, (0.05, 0.05, 0.0, 1.0, 2), start[1], 0, rec[:, 1],
                                             NLEAP, False, clamp=10.0)
    assert verdicts[0] in (0, 1) and same_bits(got[1], fields[0])


@pytest.mark.parametrize("shape", [(8, 8, 8), (32, 32, 32)])
def test_a_trip_inside_the_trajectory(gpu, dev_oracle, shape):
    """A trip that only an interior step makes.  m2 = -0.5 without a quartic term pushes a uniform field of 9.0
    outwards: phi_1 = 9.0 + 0.225 + noise of width 0.03 stays below the clamp of 10, the displacement grows by
    some 0.46 a step, and the second interior step's g = 9.9 + 0.5 is beyond it whatever the noise was.  Verdict
    2, the field unchanged bit for bit, the flag set, the counter advanced; with nleap = 1 the same start is an
    ordinary trajectory."""
    from stochquant_amd import Phi4Ensemble
    assert_shape(shape)
    par = (0.05, -0.5, 0.0, 0.1, 11)
    kw = dict(dtau=par[0], m2=par[1], lam=par[2], C=par[3], clamp=10.0)
    start = np.full((1,) + tuple(reversed(shape)), 9.0, dtype=np.float32)
    phi1, _, _, hit = trajectory(dev_oracle, shape, par, start[0], 0, NLEAP, clamp=10.0)
    assert float(np.max(np.abs(phi1))) < 9.5 and hit
    assert not trajectory(dev_oracle, shape, par, start[0], 0, 1, clamp=10.0)[3]
    with Phi4Ensemble(shape, 1, seeds=[par[4]], **kw) as E, Phi4Ensemble(shape, 1, seeds=[par[4]], **kw) as F:
        E.upload(start)
        F.upload(start)
        _, rec = E.step_hmc(1, nleap=NLEAP, record=True)
        assert rec[0, 0, 2] == 2.0 and rec[0, 0, 3] == NLEAP
        assert same_bits(E.download(), start)
        assert list(E.flags()) == [True] and list(E.step_counter) == [1]
        assert E.hmc_stats().tolist() == [[1, 0, 1, NLEAP]]
        _, rec1 = F.step_hmc(1, nleap=1, record=True)
        assert rec1[0, 0, 2] in (0.0, 1.0) and list(F.flags()) == [False]
        check_trajectories(dev_oracle, shape, par, start[0], 0, rec[:, 0], NLEAP, False, clamp=10.0)
        check_trajectories(dev_oracle, shape, par, start[0], 0, rec1[:, 0], 1, False, clamp=10.0)


def test_a_replica_without_noise_is_refused(gpu, sqlib):
    from stochquant_amd import StochQuantError
    with _ens((8, 8, 8)) as E:
        E.init_field(0.5)
        E.step(2)
        before = E.download()
        launches = E.perf()["kernel_launches"]
        E.set_params(C=0.0, first=1, count=1)
        call = lambda *a: sqlib.sq_phi4_ens_step_hmc(E._h, *a)      # noqa: E731
        assert call(4, 3, 0, 0, None, 0, None) == -4 and call(0, 3, 1, 0, None, 0, None) == -4
        assert sqlib.sq_last_error().decode() != ""
        assert call(4, 0, 0, 0, None, 0, None) == -1 and call(4, 4097, 0, 0, None, 0, None) == -1
        assert call(-1, 3, 0, 0, None, 0, None) == -1 and call(4, 3, 0, 2, None, 2, None) == -1
        assert call(4, 3, 0, 0, None, 1, None) == -1
        with pytest.raises(StochQuantError):
            E.step_hmc(4, nleap=3)
        assert E.perf()["kernel_launches"] == launches and list(E.step_counter) == [2, 2, 2]
        assert same_bits(E.download(), before) and not E.hmc_stats().any() and not E.flags().any()
        E.set_params(C=1.0, first=1, count=1)
        assert call(0, 3, 0, 0, None, 0, None) == 0 and E.perf()["kernel_launches"] == launches
        E.step_hmc(2, nleap=3)
        assert list(E.step_counter) == [4, 4, 4] and E.hmc_stats()[:, 0].tolist() == [2, 2, 2]
        assert E.perf()["kernel_launches"] == launches + 1


@pytest.mark.parametrize("nleap,randomize", [(4, False), (16, True)])
def test_no_step_size_bias_in_the_free_field(gpu, nleap, randomize):
    """Free 8 x 4 x 4 lattices, R = 256, m2 = 1, C = 1, dtau = 0.02: 300 Heun steps, then 1500 trajectories with a
    record each.  <phi^2> = S2 / 128 per replica over all records, the standard error from the spread of the 256
    replica means.

    Asserted: the mean within 4 standard errors of the exact lattice value 0.172701; <exp(-dH)> over all records
    within 4 standard errors of 1, the error from the replica means; the acceptance in [0.6, 0.9] (a float32
    NumPy model of the definition gave 0.76 for both); and the Euler step's own stationary value at this dtau
    (0.183461) more than 10 of those standard errors away, so that a missing Metropolis test would show."""
    shape, R, dt = (8, 4, 4), 256, 0.02
    want = _free_phi2(shape, 1.0, dt)
    exact = want["continuum"]
    assert abs(exact - 0.172701) < 1e-6 and abs(want["euler"] - 0.183461) < 1e-6
    with _ens(shape, R, dtau=dt, m2=1.0, lam=0.0, C=1.0, seeds=None, seed=4242) as E:
        E.step(300, scheme="heun")
        ser, rec = E.step_hmc(1500, nleap=nleap, randomize=randomize, every=1, record=True)
        assert not E.flags().any()
        stats = E.hmc_stats()
    assert ser.shape == (1500, R, 4) and rec.shape == (1500, R, 4)
    per = ser[:, :, 1].mean(axis=0) / 128.0
    mean, sem = float(per.mean()), float(per.std(ddof=1) / np.sqrt(R))
    acc = float(stats[:, 1].sum()) / float(stats[:, 0].sum())
    w = np.exp(-rec[:, :, 0]).mean(axis=0)
    wm, ws = float(w.mean()), float(w.std(ddof=1) / np.sqrt(R))
    print(f"HMC nleap {nleap} randomize {randomize} PHI2 {mean:.6f} +- {sem:.6f}  exact {exact:.6f}  "
          f"deviation {(mean - exact) / sem:+.2f} sigma  euler {want['euler']:.6f}  acceptance {acc:.4f}  "
          f"<exp(-dH)> {wm:.6f} +- {ws:.6f}  mean L {rec[:, :, 3].mean():.3f}", flush=True)
    assert stats[:, 0].tolist() == [1500] * R and not stats[:, 2].any()
    assert int(stats[:, 3].sum()) == int(rec[:, :, 3].sum())
    assert (rec[:, :, 3] == nleap).all() if not randomize else len(np.unique(rec[:, :, 3])) == nleap
    assert acc == float((rec[:, :, 2] == 1.0).mean())
    assert abs(mean - exact) < 4.0 * sem, (mean, sem, exact)
    assert abs(wm - 1.0) < 4.0 * ws, (wm, ws)
    assert 0.6 <= acc <= 0.9, acc
    assert abs(want["euler"] - mean) > 10.0 * sem, (mean, sem, want["euler"])
