"""The phi^4 ensemble's Metropolis-adjusted Langevin step on the GPU (phi4_ens_mala_kernel,
sq_phi4_ens_step_mala, Phi4Ensemble.step_mala / step(scheme="mala")) against an oracle composed here
from the header's definition: the proposal from oracle.phi4_step (device normals: bit for bit), the
uniform from oracle.philox, dH in NumPy float64 with math.fsum.

Parameters: the seeds, m2 and lambda of test_gpu_phi4_ens_heun.py's three replicas.  Their C is [0, 1, 0.5]
and a MALA step refuses C = 0, so replica 0 runs at C = 0.7 here; and dtau is chosen per shape, 0.2 / V^(1/3),
where the acceptance is near one half (it falls with the volume at fixed dtau), so that both verdicts occur.

Tolerances.  Fields, uniforms, verdicts, counters, flags and counts: exact.  dH against the float64
formula: 1e-10 A, A the sum of the absolute values of all summed terms over sig^2 (the worst-case error
of a double summation of <= 32,768 sites' terms is some 3.6e-12 A).  The verdict is checked against the
kernel's own dH with NumPy's exp; a step with |exp(-dH) - u| < 1e-12 could not be decided across two exp
implementations, and there must be none (on a hit: another seed, not another bound).  The physics test's
bounds are derived at the test.
"""
import math

import numpy as np
import pytest

from test_gpu_phi4_ens_heun import CLAMP, LAM, M2, SEEDS, _free_phi2
from test_oracle import same_bits
from test_phi4_ens_shapes import GPU_SHAPES, assert_shape

pytestmark = pytest.mark.gpu

SHAPES = list(GPU_SHAPES)
CS = [0.7, 1.0, 0.5]
COUNTERS = [7, 2 ** 32 - 3, 2 ** 40 + 5]      # one crosses into the high word during the six steps
STREAM_ACCEPT = 3                            # kStreamAccept (sq_noise_consts.h)
THERM = 100                                  # Euler steps before the first MALA step

_cache = {}


def _dtau(shape):
    return round(0.2 / (shape[0] * shape[1] * shape[2]) ** (1.0 / 3.0), 4)


def _ens(shape, R=3, **kw):
    from stochquant_amd import Phi4Ensemble
    kw.setdefault("dtau", _dtau(shape))
    kw.setdefault("m2", M2[:R])
    kw.setdefault("lam", LAM[:R])
    kw.setdefault("C", CS[:R])
    kw.setdefault("seeds", SEEDS[:R])
    kw.setdefault("clamp", CLAMP)
    return Phi4Ensemble(shape, R, **kw)


def _record(dtau, m2, lam, C):
    """The replica's float record in double: h, m2, lam6, sig (phi4_base_args' expressions)."""
    h = np.float32(dtau)
    lam6 = np.float32(float(np.float32(lam)) / 6.0)
    sig = np.float32(math.sqrt(2.0 * float(h)) * C)
    return float(h), float(np.float32(m2)), float(lam6), float(sig)


def uniform(o, seed, s):
    w = o.philox([0, STREAM_ACCEPT << 24, s & 0xFFFFFFFF, s >> 32], [seed & 0xFFFFFFFF, seed >> 32])[0]
    return (w + 0.5) * 2.0 ** -32


def dH_reference(phi, p, rec):
    """(dH, A) of the header's formula in float64, exactly rounded sums (math.fsum) of every term."""
    h, m2, lam6, sig = rec
    f, g = phi.astype(np.float64), p.astype(np.float64)

    def fwd(x):
        return [np.roll(x, -1, axis=a) for a in (2, 1, 0)]

    def drift(x):
        nb = sum(np.roll(x, d, axis=a) for a in (0, 1, 2) for d in (1, -1))
        return nb - 6.0 * x - x * (m2 + lam6 * x * x)

    a = g - f - h * drift(f)
    b = f - g - h * drift(g)
    km, l4 = 3.0 + 0.5 * m2, 0.25 * lam6
    terms = [2.0 * h * km * g * g, -2.0 * h * km * f * f, 2.0 * h * l4 * g ** 4, -2.0 * h * l4 * f ** 4,
             0.5 * b * b, -0.5 * a * a]
    terms += [-2.0 * h * g * n for n in fwd(g)] + [2.0 * h * f * n for n in fwd(f)]
    flat = np.concatenate([t.ravel() for t in terms])
    s2 = sig * sig
    return math.fsum(flat) / s2, math.fsum(np.abs(flat)) / s2


def check_steps(o, shape, par, phi, s0, rec, clamp=CLAMP):
    """Follow one replica through the records of a call from field phi at counter s0: every record against the
    oracle; returns (the field after each step, the verdicts)."""
    dtau, m2, lam, C, seed = par
    P = o.phi4_params(shape, dtau, m2, lam, seed, clamp=clamp, C=C)
    R = _record(dtau, m2, lam, C)
    fields, verdicts = [], []
    for k in range(rec.shape[0]):
        dH, u, v = (float(x) for x in rec[k])
        s = s0 + k
        p = o.phi4_step(P, phi, s)
        assert u == uniform(o, seed, s), (shape, k, u)
        ref, A = dH_reference(phi, p, R)
        assert abs(dH - ref) <= 1e-10 * A, (shape, k, dH, ref, A)
        with np.errstate(invalid="ignore"):
            hit = not bool(np.max(np.abs(p)) < clamp)
        assert (v == 2.0) == hit, (shape, k, v)
        if not hit:
            with np.errstate(over="ignore"):
                e = float(np.exp(-dH))
            assert abs(e - u) >= 1e-12, ("undecidable across exp implementations: change the seed", shape, k, e, u)
            assert v == float(dH <= 0.0 or u < e), (shape, k, dH, u, v)
        if v == 1.0:
            phi = p
        fields.append(phi)
        verdicts.append(int(v))
    return fields, verdicts


def _params(shape, r):
    return (_dtau(shape), M2[r], LAM[r], CS[r], SEEDS[r])


def _run_shape(o, shape):
    """The oracle test of one shape, once: calls of 3, 1, 1, 1 steps with records from thermalised fields; returns
    the verdicts of all replicas."""
    if shape in _cache:
        return _cache[shape]
    assert_shape(shape)
    calls = (3, 1, 1, 1)
    with _ens(shape) as E:
        E.init_field(0.5)
        E.step(THERM)
        E.step_counter = COUNTERS
        start = E.download()
        assert not E.flags().any()
        recs, after = [], []
        for n in calls:
            ser, rec = E.step_mala(n, record=True)
            assert ser is None and rec.shape == (n, 3, 3)
            recs.append(rec)
            after.append(E.download())
        assert [int(s) for s in E.step_counter] == [c + sum(calls) for c in COUNTERS]
        flags = E.flags()
        stats = E.mala_stats()
    rec = np.concatenate(recs)
    out = []
    for r in range(3):
        fields, verdicts = check_steps(o, shape, _params(shape, r), start[r], COUNTERS[r], rec[:, r])
        done = 0
        for n, got in zip(calls, after):
            done += n
            assert same_bits(got[r], fields[done - 1]), f"replica {r} after step {done}: " \
                f"{np.count_nonzero(got[r] != fields[done - 1])} sites differ"
        assert list(stats[r]) == [sum(calls), verdicts.count(1), verdicts.count(2)], (r, stats[r], verdicts)
        assert bool(flags[r]) == (2 in verdicts) and 2 not in verdicts, (r, flags, verdicts)
        out.append(verdicts)
    print(f"MALA {shape} dtau {_dtau(shape)} verdicts {out}", flush=True)
    _cache[shape] = out
    return out


@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_composed_oracle(gpu, dev_oracle, shape):
    _run_shape(dev_oracle, shape)


def test_both_verdicts_in_every_work_group_class(gpu, dev_oracle):
    """Over the shapes above, every (K, images) class has accepted and rejected steps."""
    seen = {}
    for shape in SHAPES:
        K, _, images, _ = GPU_SHAPES[shape]
        seen.setdefault((K, images), set()).update(v for vs in _run_shape(dev_oracle, shape) for v in vs)
    assert {k for k, _ in seen} == {1, 2, 4, 8} and (8, 1) in seen and (8, 2) in seen
    for cls, vs in seen.items():
        assert {0, 1} <= vs, (cls, vs)


@pytest.mark.parametrize("shape", [(8, 8, 8), (32, 32, 32)])
def test_guard_trip_rejects_and_flags(gpu, dev_oracle, shape):
    """Replica 0: a field at 9.9 everywhere under clamp 10 with noise of width 0.32: the proposal reaches the
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
        ser, rec = E.step_mala(1, record=True)
        _, rec1 = One.step_mala(1, record=True)
        got = E.download()
        assert list(E.flags()) == [True, False] and list(E.step_counter) == [1, 1]
        assert E.mala_stats().tolist() == [[1, 0, 1], [1, int(rec[0, 1, 2]), 0]]
        assert same_bits(got[1], One.download()[0])
        assert np.array_equal(rec[0, 1].view(np.uint64), rec1[0, 0].view(np.uint64))
    P = dev_oracle.phi4_params(shape, 0.05, 0.05, 0.0, 1, clamp=10.0, C=1.0)
    assert np.max(np.abs(dev_oracle.phi4_step(P, start[0], 0))) == np.float32(10.0)
    assert rec[0, 0, 2] == 2.0 and same_bits(got[0], start[0])
    fields, verdicts = check_steps(dev_oracle, shape, (0.05, 0.05, 0.0, 1.0, 2), start[1], 0, rec[:, 1], clamp=10.0)
    assert verdicts[0] in (0, 1) and same_bits(got[1], fields[0])


@pytest.mark.parametrize("shape", [(8, 2, 2), (16, 24, 24), (32, 32, 32)])
def test_calls_are_additive_and_schemes_mix(gpu, shape):
    """step_mala(2); step_mala(3) is step_mala(5) in fields, records and counts; and MALA, Heun and Euler calls
    interleaved on one handle give what the same calls give on twins, each of which gets the field and the
    counters by upload."""
    assert_shape(shape)
    with _ens(shape) as A, _ens(shape) as B, _ens(shape) as M:
        for E in (A, B, M):
            E.init_field(0.5)
            E.step(THERM)
            E.step_counter = COUNTERS
        _, ra = A.step_mala(5, record=True)
        _, rb1 = B.step_mala(2, record=True)
        _, rb2 = B.step_mala(3, record=True)
        assert np.array_equal(ra.view(np.uint64), np.concatenate([rb1, rb2]).view(np.uint64))
        assert same_bits(A.download(), B.download())
        assert np.array_equal(A.mala_stats(), B.mala_stats()) and A.mala_stats()[:, 0].tolist() == [5, 5, 5]
        assert list(A.step_counter) == list(B.step_counter)
        seq = [("mala", 2), ("heun", 2), ("euler", 1), ("mala", 3), ("heun", 1)]
        field, cnt = M.download(), np.array(COUNTERS, dtype=np.uint64)
        for scheme, n in seq:
            M.step(n, scheme=scheme)
            with _ens(shape) as T:
                T.upload(field)
                T.step_counter = cnt
                T.step(n, scheme=scheme)
                field, cnt = T.download(), T.step_counter
            assert same_bits(M.download(), field), (scheme, n)
            assert list(M.step_counter) == list(cnt)
        assert M.mala_stats()[:, 0].tolist() == [5, 5, 5]
        M.mala_reset(1, 1)
        assert M.mala_stats()[:, 0].tolist() == [5, 0, 5]


def test_independent_of_the_replica_count(gpu):
    shape, R = (8, 8, 8), 300
    assert_shape(shape)
    kw = dict(dtau=0.025, m2=0.5, lam=1.0, C=1.0)
    with _ens(shape, R, seeds=None, seed=500, **kw) as E:
        E.init_field(0.5)
        E.step(THERM)
        _, rec = E.step_mala(6, record=True)
        got = E.download()
        stats = E.mala_stats()
    assert 0 < stats[:, 1].sum() < 6 * R
    for r in (0, 1, 255, 256, 299):
        with _ens(shape, 1, seeds=[500 + r], **kw) as One:
            One.init_field(0.5)
            One.step(THERM)
            _, rec1 = One.step_mala(6, record=True)
            assert same_bits(got[r], One.download()[0]), f"replica {r}"
            assert np.array_equal(rec[:, r].view(np.uint64), rec1[:, 0].view(np.uint64)), f"replica {r}"
            assert np.array_equal(stats[r], One.mala_stats()[0])


@pytest.mark.parametrize("shape", [(8, 3, 5), (64, 16, 8), (8, 50, 51), (32, 32, 32)])
def test_measurements_in_flight(gpu, shape):
    """step_mala(6, every=2, correlate) against a second ensemble that takes two unmeasured MALA steps and measures
    the field it then holds with moments() / slices(), three times; a third makes the call without the series.  The
    accumulators advance once per measurement, after a rejected step too."""
    with _ens(shape) as A, _ens(shape) as B, _ens(shape) as N, _ens(shape) as P:
        for E in (A, B, N, P):
            E.init_field(0.5)
            E.step(THERM)
        ser, rec = A.step_mala(6, every=2, correlate=True, record=True)
        assert ser.shape == (3, 3, 4)
        G, S1 = np.zeros((3, A.nt)), np.zeros(3)
        for m in range(3):
            B.step_mala(2)
            mom = B.moments()
            row = np.stack([mom[k] for k in ("S1", "S2", "S4", "NN")], axis=1)
            assert np.array_equal(ser[m].view(np.uint64), row.view(np.uint64)), f"record {m}"
            S, g = B.slices()
            G = G + g
            s1 = np.zeros(3)
            for z in range(shape[2]):
                s1 = s1 + S[:, z]
            S1 = S1 + s1
        from stochquant_amd import _lib
        _lib.call("sq_phi4_ens_step_mala", N._h, 6, 2, None, 1, None)
        for E in (A, N):
            aG, aS1, aN = E.corr_sums()
            assert np.array_equal(aG.view(np.uint64), G.view(np.uint64))
            assert np.array_equal(aS1.view(np.uint64), S1.view(np.uint64))
            assert list(aN) == [3, 3, 3]
        # rejected steps among them: the measurements did not wait for an acceptance
        assert (rec[:, :, 2] == 0.0).any()
        assert same_bits(A.download(), B.download()) and same_bits(A.download(), N.download())
        # a measured call leaves the field, the counters and the counts of an unmeasured one
        assert P.step(6, scheme="mala") is None
        assert same_bits(A.download(), P.download())
        assert np.array_equal(A.mala_stats(), P.mala_stats()) and list(P.corr_sums()[2]) == [0, 0, 0]
        assert list(A.step_counter) == list(B.step_counter) == list(P.step_counter) == [THERM + 6] * 3
        assert A.step(5, every=7, scheme="mala").shape == (0, 3, 4)      # the incomplete tail


def test_argument_rules(gpu, sqlib):
    from stochquant_amd import StochQuantError
    assert sqlib.sq_phi4_ens_step_mala(None, 4, 0, None, 0, None) == -1
    assert sqlib.sq_phi4_ens_mala_stats(None, 0, 1, None) == -1 and sqlib.sq_phi4_ens_mala_reset(None, 0, 1) == -1
    with _ens((8, 8, 8)) as E:
        call = lambda *a: sqlib.sq_phi4_ens_step_mala(E._h, *a)      # noqa: E731
        assert call(-1, 0, None, 0, None) == -1
        assert call(4, -1, None, 0, None) == -1
        assert call(4, 2, None, 2, None) == -1 and call(4, 2, None, 3, None) == -1      # no momenta under MALA
        assert call(4, 0, None, 1, None) == -1                                        # a measurement needs every >= 1
        assert sqlib.sq_last_error().decode() != ""
        assert call(0, 0, None, 0, None) == 0 and call(0, 2, None, 1, None) == 0        # nsteps = 0 does nothing
        assert list(E.step_counter) == [0, 0, 0] and E.perf()["kernel_launches"] == 0
        assert E.mala_stats().tolist() == [[0, 0, 0]] * 3
        assert sqlib.sq_phi4_ens_mala_stats(E._h, 2, 2, None) == -1
        with pytest.raises(StochQuantError):
            E.step_mala(-1)
        for bad in (lambda: E.step(4, every=2, momenta=True, scheme="mala"),
                    lambda: E.step(4, every=2, flow=True, scheme="mala"),
                    lambda: E.step_flow(4, 2, scheme="mala"),
                    lambda: E.run_frames(2, scheme="mala"),
                    lambda: E.run_frames(2, flow=True, scheme="mala"),
                    lambda: E.run_frames_flow(2, scheme="mala"),
                    lambda: E.step_mala(4, every=0, correlate=True)):
            with pytest.raises(ValueError):
                bad()
        assert E.perf()["kernel_launches"] == 0
        E.step(2, scheme="mala")
        p = E.perf()
        assert p["steps"] == 2 * 3 and p["kernel_launches"] == 1 and list(E.step_counter) == [2, 2, 2]
        # one replica without noise: the whole call is refused before any launch, nothing moves
        E.set_params(C=0.0, first=1, count=1)
        assert call(4, 0, None, 0, None) == -4 and call(0, 0, None, 0, None) == -4
        with pytest.raises(StochQuantError):
            E.step(4, scheme="mala")
        assert E.perf()["kernel_launches"] == 1 and list(E.step_counter) == [2, 2, 2]
        assert E.mala_stats()[:, 0].tolist() == [2, 2, 2]
        E.step(1)                                                                     # the other schemes still run
        E.set_params(C=1.0, first=1, count=1)
        E.step(1, scheme="mala")
        assert list(E.step_counter) == [4, 4, 4]


def test_no_step_size_bias_in_the_free_field(gpu):
    """Free 8 x 4 x 4 lattices, R = 256, m2 = 1, dtau = 0.02: 500 Euler steps, then 4000 MALA steps with a record
    every 10, the first quarter dropped.  <phi^2> = S2 / 128 per replica, the standard error from the 256 replica
    means.

    Asserted: the standard error below 0.3 % of the mean; the mean within 0.5 % of the exact lattice value
    0.172701 (a float64 NumPy run of this protocol gave 0.17279 +- 0.00016, so 0.5 % is some 5 sigma) and more
    than 3 % from the Euler step's own stationary value at this dtau (0.183461 by _free_phi2, 6.2 % away); the
    acceptance between 0.7 and 0.9 (NumPy: 0.81); and the HMC identity <exp(-dH)> = 1 over all records within 5
    standard errors, the error from the replica means."""
    shape, R, dt = (8, 4, 4), 256, 0.02
    want = _free_phi2(shape, 1.0, dt)
    exact = 0.172701
    assert abs(want["continuum"] - exact) < 1e-6
    assert abs(want["euler"] - 0.183461) < 1e-6
    with _ens(shape, R, dtau=dt, m2=1.0, lam=0.0, C=1.0, seeds=None, seed=4242) as E:
        E.step(500)
        ser, rec = E.step_mala(4000, every=10, record=True)
        assert not E.flags().any()
        stats = E.mala_stats()
    assert ser.shape == (400, R, 4) and rec.shape == (4000, R, 3)
    per = ser[100:, :, 1].mean(axis=0) / 128.0
    mean, sem = float(per.mean()), float(per.std(ddof=1) / np.sqrt(R))
    acc = float(stats[:, 1].sum()) / float(stats[:, 0].sum())
    w = np.exp(-rec[:, :, 0]).mean(axis=0)
    wm, ws = float(w.mean()), float(w.std(ddof=1) / np.sqrt(R))
    print(f"MALA PHI2 {mean:.6f} +- {sem:.6f}  exact {exact:.6f}  deviation {100.0 * (mean / exact - 1.0):+.3f} %  "
          f"euler {want['euler']:.6f}  acceptance {acc:.4f}  <exp(-dH)> {wm:.6f} +- {ws:.6f}", flush=True)
    assert stats[:, 0].tolist() == [4000] * R and not stats[:, 2].any()
    assert acc == float((rec[:, :, 2] == 1.0).mean())
    assert sem < 0.003 * mean, (mean, sem)
    assert abs(mean - exact) < 0.005 * exact, (mean, sem)
    assert abs(mean - want["euler"]) > 0.03 * exact, (mean, want["euler"])
    assert 0.7 < acc < 0.9, acc
    assert abs(wm - 1.0) < 5.0 * ws, (wm, ws)
