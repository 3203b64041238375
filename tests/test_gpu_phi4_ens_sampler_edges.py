"""The edges of the phi^4 ensemble's two Metropolis-corrected samplers (phi4_ens_mala_kernel / step_mala,
phi4_ens_hmc_kernel / step_hmc) beyond test_gpu_phi4_ens_mala.py and test_gpu_phi4_ens_hmc.py, whose oracle,
records and tolerances are used unchanged (check_trajectories; a MALA step is followed as the trajectory of
one leapfrog step that it is, its record given a fourth column L = 1):

  1. the measuring instances (every / correlate) at every (K, plain images, correlator images) class;
  2. guard trips inside a call of many trajectories, behind accepted ones and with more to follow;
  3. the transitions between accepted and rejected trajectories of one and of several steps, shown to occur;
  4. a NaN or an infinity in the start field;
  5. nleap = 4096, the limit, fixed and randomised;
  7. the stationary law of the interacting theory at C != 1 against an independent Metropolis sampler
     (tests/golden/make_phi4_metropolis.py).
(6, the fuzz, is in test_gpu_fuzz.py.)

Every pattern asserted in 2 and 3 is asserted of oracle_chain's output: a chain followed on the CPU alone, the
verdict from the float64 dH.  That the kernel took the same path is check_trajectories' finding.

Tolerances: those of the two files named.  Everything discrete exact, dH within 1e-10 A of the float64 formula,
no trajectory with |exp(-dH) - u| < 1e-12.  The physics test's bounds are derived at the test.
"""
import json
import math
import os

import numpy as np
import pytest

import test_gpu_phi4_ens_hmc as hmc
import test_gpu_phi4_ens_mala as mala
from test_gpu_phi4_ens_heun import CLAMP, LAM, M2, SEEDS
from test_gpu_phi4_ens_hmc import accept_block, check_trajectories, dH_reference, length, trajectory
from test_gpu_phi4_ens_mala import COUNTERS, CS, THERM, _record
from test_oracle import same_bits
from test_phi4_ens_shapes import SAMPLER_MEASURE_SHAPES, TWO_TO_ONE, assert_shape, measure_class

pytestmark = pytest.mark.gpu

SAMPLERS = ("hmc", "mala")
MOD = {"hmc": hmc, "mala": mala}


def _seeds(k):
    """The three replicas' seeds, or with k != 0 the k-th seeds behind them: where the tests' own seeds do not
    give a sequence of verdicts that a test has to show, it says which k does."""
    return [s + k for s in SEEDS]


def _params(sampler, shape, r, k=0):
    return (MOD[sampler]._dtau(shape), M2[r], LAM[r], CS[r], SEEDS[r] + k)


def _thermalised(sampler, shape, n=1, k=0):
    """n ensembles of the sampler's own test module (its dtau rule, the three replicas), thermalised as there."""
    out = [MOD[sampler]._ens(shape, seeds=_seeds(k)) for _ in range(n)]
    for E in out:
        E.init_field(0.5)
        E.step(THERM)
        E.step_counter = COUNTERS
    return out


def _run(E, sampler, n, nleap=1, randomize=False, **kw):
    """(series, records (n, R, 4)) of n trajectories: a MALA step's record gets L = 1."""
    if sampler == "hmc":
        return E.step_hmc(n, nleap=nleap, randomize=randomize, record=True, **kw)
    ser, rec = E.step_mala(n, record=True, **kw)
    return ser, np.concatenate([rec, np.ones(rec.shape[:2] + (1,))], axis=2)


def _stats(E, sampler):
    return E.hmc_stats() if sampler == "hmc" else E.mala_stats()


def _want_stats(sampler, verdicts, lengths):
    s = [len(verdicts), verdicts.count(1), verdicts.count(2), sum(lengths)]
    return s if sampler == "hmc" else s[:3]


def oracle_chain(o, shape, par, phi, s0, n, nleap, randomize, clamp=CLAMP):
    """n trajectories from field phi at counter s0 on the CPU alone: ([(verdict, L)], the field held at the end).
    The verdict is the definition's, from the float64 dH of dH_reference."""
    dtau, m2, lam, C, seed = par
    R = _record(dtau, m2, lam, C)
    seq = []
    for k in range(n):
        s = s0 + k
        L = length(o, seed, s, nleap, randomize)
        u = (int(accept_block(o, seed, s)[0]) + 0.5) * 2.0 ** -32
        phi1, phim, phiL, hit = trajectory(o, shape, par, phi, s, L, clamp)
        if hit:
            v = 2
        else:
            dH = dH_reference(phi, phi1, phim, phiL, R)[0]
            v = int(dH <= 0.0 or u < math.exp(-dH))
        if v == 1:
            phi = phiL
        seq.append((v, L))
    return seq, phi


def has_run(seq, *preds):
    """Whether consecutive entries of seq satisfy the predicates, in order."""
    return any(all(p(*seq[i + j]) for j, p in enumerate(preds)) for i in range(len(seq) - len(preds) + 1))


def _follow(o, sampler, shape, start, rec, got, stats, flags, nleap, randomize, clamp=CLAMP, k=0):
    """Every replica of a call through check_trajectories and oracle_chain; returns the oracle's sequences."""
    n = rec.shape[0]
    if sampler == "mala":
        nleap, randomize = 1, False
    seqs = []
    for r in range(rec.shape[1]):
        par = _params(sampler, shape, r, k)
        fields, verdicts, lengths = check_trajectories(o, shape, par, start[r], COUNTERS[r], rec[:, r], nleap,
                                                       randomize, clamp=clamp)
        seq, last = oracle_chain(o, shape, par, start[r], COUNTERS[r], n, nleap, randomize, clamp=clamp)
        assert seq == list(zip(verdicts, lengths)), (sampler, shape, r, seq, verdicts, lengths)
        assert same_bits(fields[-1], last) and same_bits(got[r], last), (sampler, shape, r)
        assert list(stats[r]) == _want_stats(sampler, verdicts, lengths), (sampler, shape, r, stats[r], seq)
        assert bool(flags[r]) == (2 in verdicts), (sampler, shape, r, flags, verdicts)
        seqs.append(seq)
    return seqs


# 1. the measuring instances ------------------------------------------------------------------------------------

def test_the_measuring_shapes_are_the_classes(gpu):
    """The CPU suite enumerates the classes (test_phi4_ens_shapes.py); here: the list this file runs holds one
    one-image, one two-image and the two-to-one lattice at K = 8 and every smaller K."""
    have = {measure_class(s) for s in SAMPLER_MEASURE_SHAPES}
    assert have == {(1, 2, 2), (2, 2, 2), (4, 2, 2), (8, 2, 2), (8, 2, 1), (8, 1, 1)}
    assert measure_class(TWO_TO_ONE) == (8, 2, 1)


def _measured_twin(Q, sampler, shape):
    """Three times two unmeasured trajectories and a measurement of the field held: (rows, G, S1, records)."""
    rows, recs = [], []
    G, S1 = np.zeros((3, Q.nt)), np.zeros(3)
    for m in range(3):
        recs.append(_run(Q, sampler, 2, nleap=4, randomize=True)[1])
        mom = Q.moments()
        rows.append(np.stack([mom[k] for k in ("S1", "S2", "S4", "NN")], axis=1))
        Sz, g = Q.slices()
        G = G + g
        s1 = np.zeros(3)
        for z in range(shape[2]):
            s1 = s1 + Sz[:, z]
        S1 = S1 + s1
    return np.stack(rows), G, S1, np.concatenate(recs)


def _same_call(E, Q, sampler, rec, want_rec):
    assert np.array_equal(rec.view(np.uint64), want_rec.view(np.uint64))
    assert same_bits(E.download(), Q.download())
    assert np.array_equal(_stats(E, sampler), _stats(Q, sampler)) and _stats(E, sampler)[:, 0].tolist() == [6] * 3
    assert list(E.step_counter) == list(Q.step_counter) == [c + 6 for c in COUNTERS]
    assert list(E.flags()) == list(Q.flags())


@pytest.mark.parametrize("shape", SAMPLER_MEASURE_SHAPES)
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_measurements_in_flight_in_every_instance(gpu, sampler, shape):
    """Six trajectories (nleap = 4, randomised) with every = 2 and the correlator against a twin that makes the
    three unmeasured calls and measures with moments() / slices(): series rows, accumulators, records, fields and
    counts bit for bit.  At the two-to-one lattice and at (16, 24, 24) also the call with the correlator alone
    and the call with the series alone."""
    from stochquant_amd import _lib
    from stochquant_amd.langevin import _dptr
    assert_shape(shape)
    extra = shape in (TWO_TO_ONE, (16, 24, 24))
    ens = _thermalised(sampler, shape, 4 if extra else 2)
    try:
        S, Q = ens[:2]
        ser, rec = _run(S, sampler, 6, nleap=4, randomize=True, every=2, correlate=True)
        rows, G, S1, want_rec = _measured_twin(Q, sampler, shape)
        assert ser.shape == (3, 3, 4) and np.array_equal(ser.view(np.uint64), rows.view(np.uint64))
        aG, aS1, aN = S.corr_sums()
        assert np.array_equal(aG.view(np.uint64), G.view(np.uint64))
        assert np.array_equal(aS1.view(np.uint64), S1.view(np.uint64))
        assert list(aN) == [3, 3, 3] and list(Q.corr_sums()[2]) == [0, 0, 0]
        _same_call(S, Q, sampler, rec, want_rec)
        if sampler == "hmc":
            assert len(np.unique(rec[:, :, 3])) >= 2
        if extra:
            Co, So = ens[2:]
            if sampler == "hmc":
                r4 = np.zeros((6, 3, 4))
                _lib.call("sq_phi4_ens_step_hmc", Co._h, 6, 4, 1, 2, None, 1, _dptr(r4))
            else:
                r3 = np.zeros((6, 3, 3))
                _lib.call("sq_phi4_ens_step_mala", Co._h, 6, 2, None, 1, _dptr(r3))
                r4 = np.concatenate([r3, np.ones((6, 3, 1))], axis=2)
            cG, cS1, cN = Co.corr_sums()
            assert np.array_equal(cG.view(np.uint64), G.view(np.uint64))
            assert np.array_equal(cS1.view(np.uint64), S1.view(np.uint64)) and list(cN) == [3, 3, 3]
            _same_call(Co, Q, sampler, r4, want_rec)
            ser2, rec2 = _run(So, sampler, 6, nleap=4, randomize=True, every=2)
            assert np.array_equal(ser2.view(np.uint64), rows.view(np.uint64))
            assert list(So.corr_sums()[2]) == [0, 0, 0]
            _same_call(So, Q, sampler, rec2, want_rec)
    finally:
        for E in ens:
            E.close()


# 2. trips inside a call ----------------------------------------------------------------------------------------

# (k, factor) per sampler and shape: the seeds are _seeds(k), the clamp is factor x the largest |phi| of the three
# thermalised start fields.  Chosen on the CPU, with the oracle's own normals, among factors of 1.02 .. 1.05 and
# so that the factors 0.005 to either side give the same verdicts; the MI355X gave the CPU's verdicts in all
# eight.  With the tests' own seeds (k = 0) no factor from 1.001 to 1.08 gives HMC at (64, 11, 29) a replica with
# two trips (replica 1, the only one near the clamp: 211001111111 up to 1.024, 112101101111 up to 1.051, no trip
# beyond), none gives MALA at (16, 24, 24) a trip behind an accepted step and two trips at once (201021101111 up
# to 1.020, 112110101111 beyond), and MALA at (64, 11, 29) has both at 1.025 alone of 1.015, 1.02, 1.025, 1.03:
# those three run the nearest seeds behind that do.
TRIP_CASES = {("hmc", (8, 8, 8)): (0, 1.04), ("hmc", (16, 24, 24)): (0, 1.04), ("hmc", (8, 50, 51)): (0, 1.045),
              ("hmc", (64, 11, 29)): (1, 1.035),
              ("mala", (8, 8, 8)): (0, 1.035), ("mala", (16, 24, 24)): (6, 1.03), ("mala", (8, 50, 51)): (0, 1.035),
              ("mala", (64, 11, 29)): (2, 1.035)}
TRIP_SHAPES = [(8, 8, 8), (16, 24, 24), (8, 50, 51), (64, 11, 29)]


@pytest.mark.parametrize("shape", TRIP_SHAPES)
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_trips_inside_a_call(gpu, dev_oracle, sampler, shape):
    """Twelve trajectories in one call (nleap = 4, randomised) under a clamp a few per cent above the start
    fields' maximum.  Over the three replicas the oracle's verdicts hold a trip directly behind an accepted
    trajectory, an ordinary verdict behind a trip, and a replica with two trips or more; the kernel follows the
    oracle through all of it, the flags are the tripped replicas', the trip count is the oracle's."""
    assert_shape(shape)
    k, factor = TRIP_CASES[sampler, shape]
    (T,) = _thermalised(sampler, shape, k=k)
    with T:
        start = T.download()
        assert not T.flags().any()
    clamp = float(np.float32(factor * float(np.max(np.abs(start)))))
    with MOD[sampler]._ens(shape, clamp=clamp, seeds=_seeds(k)) as E:
        E.upload(start)
        E.step_counter = COUNTERS
        ser, rec = _run(E, sampler, 12, nleap=4, randomize=True)
        assert ser is None
        got, stats, flags = E.download(), _stats(E, sampler), E.flags()
        assert list(E.step_counter) == [c + 12 for c in COUNTERS]
    seqs = _follow(dev_oracle, sampler, shape, start, rec, got, stats, flags, 4, True, clamp=clamp, k=k)
    vs = [[v for v, _ in seq] for seq in seqs]
    print(f"TRIPS {sampler} {shape} seeds +{k} clamp {factor} x max = {clamp:.6f} "
          f"verdicts {[''.join(map(str, v)) for v in vs]} lengths {[[L for _, L in seq] for seq in seqs]}", flush=True)
    assert any(has_run(seq, lambda v, L: v == 1, lambda v, L: v == 2) for seq in seqs), vs
    assert any(has_run(seq, lambda v, L: v == 2, lambda v, L: v in (0, 1)) for seq in seqs), vs
    assert max(v.count(2) for v in vs) >= 2 and int(stats[:, 2].max()) == max(v.count(2) for v in vs), (vs, stats)


# 3. transitions ------------------------------------------------------------------------------------------------

TRANSITION_SHAPES = {2: [(8, 8, 8), (16, 24, 24)], 1: [(64, 11, 29)]}      # by images of the plain launch
# The tests' own seeds give three of the four transitions within 16 trajectories, in both image modes, but
# accept -> reject of one step -> reject of several in neither (the CPU oracle; replica 0 starts (1, 1) (1, 4)
# (0, 4) (0, 1) (0, 4) (0, 1) (1, 1)).  The next seeds give every one at least twice in each mode.
TRANSITION_K = 1
_transitions = {}


def _transition_run(o, shape):
    """One call of 16 randomised trajectories (nleap = 4) from the thermalised fields, followed; once a shape."""
    if shape not in _transitions:
        i = assert_shape(shape)
        (E,) = _thermalised("hmc", shape, k=TRANSITION_K)
        with E:
            start = E.download()
            _, rec = _run(E, "hmc", 16, nleap=4, randomize=True)
            got, stats, flags = E.download(), E.hmc_stats(), E.flags()
            assert list(E.step_counter) == [c + 16 for c in COUNTERS] and not flags.any()
        seqs = _follow(o, "hmc", shape, start, rec, got, stats, flags, 4, True, k=TRANSITION_K)
        print(f"TRANSITIONS {shape} {seqs}", flush=True)
        _transitions[shape] = (i["images"], seqs)
    return _transitions[shape]


@pytest.mark.parametrize("shape", [s for ss in TRANSITION_SHAPES.values() for s in ss])
def test_sixteen_mixed_trajectories(gpu, dev_oracle, shape):
    _transition_run(dev_oracle, shape)


@pytest.mark.parametrize("images", [2, 1])
def test_every_transition_occurs(gpu, dev_oracle, images):
    """In each image mode, over the replicas of its shapes, the oracle's (verdict, L) sequences hold: accept ->
    reject of several steps (the row flushed, then read back); accept -> reject of one step -> reject of several
    (the row stays behind across the one-step trajectory); a reject of one step straight after a trajectory of
    several; a reject of several steps -> accept."""
    seqs = []
    for shape in TRANSITION_SHAPES[images]:
        got, ss = _transition_run(dev_oracle, shape)
        assert got == images
        seqs += ss
    acc = lambda v, L: v == 1                         # noqa: E731
    rej1 = lambda v, L: v == 0 and L == 1             # noqa: E731
    rejn = lambda v, L: v == 0 and L > 1              # noqa: E731
    long = lambda v, L: L > 1                         # noqa: E731
    for name, run in (("accept, long reject", (acc, rejn)), ("accept, short reject, long reject", (acc, rej1, rejn)),
                      ("long, short reject", (long, rej1)), ("long reject, accept", (rejn, acc))):
        assert any(has_run(seq, *run) for seq in seqs), (images, name, seqs)


# 4. non-finite start fields ------------------------------------------------------------------------------------

@pytest.mark.parametrize("bad", ["nan", "inf"])
@pytest.mark.parametrize("shape", [(8, 8, 8), (64, 11, 29)])
@pytest.mark.parametrize("sampler", SAMPLERS)
def test_a_non_finite_start_field(gpu, dev_oracle, sampler, shape, bad):
    """Replica 0 with one NaN (or +inf) site at the last z and y: three trajectories (three leapfrog steps each
    under HMC), every one a guard trip, the field back bit for bit with the NaN's payload, the flag set, the
    counter advanced.  Replica 1, quiet, is bit for bit what it is alone.  The composed oracle trips as well."""
    assert_shape(shape)
    Lx, Ly, Lz = shape
    nleap = 3 if sampler == "hmc" else 1
    mk = lambda R, **kw: MOD[sampler]._ens(shape, R, **kw)      # noqa: E731
    with mk(2) as E, mk(1, m2=M2[1:2], lam=LAM[1:2], C=CS[1:2], seeds=SEEDS[1:2]) as One:
        E.init_field(0.5)
        E.step(THERM)
        start = E.download()
        start[0, Lz - 1, Ly - 1, 3] = np.float32(bad)
        if bad == "nan":      # a payload that is not the default quiet NaN's
            start[0].view(np.uint32)[Lz - 1, Ly - 1, 3] = 0x7FC12345
        E.upload(start)
        E.step_counter = COUNTERS[:2]
        One.upload(start[1:])
        One.step_counter = COUNTERS[1:2]
        _, rec = _run(E, sampler, 3, nleap=nleap)
        _, rec1 = _run(One, sampler, 3, nleap=nleap)
        got = E.download()
        assert list(E.flags()) == [True, False] and list(One.flags()) == [False]
        assert list(E.step_counter) == [c + 3 for c in COUNTERS[:2]]
        stats = _stats(E, sampler)
        assert stats[0].tolist() == ([3, 0, 3, 9] if sampler == "hmc" else [3, 0, 3])
        assert np.array_equal(stats[1], _stats(One, sampler)[0])
        assert same_bits(got[1], One.download()[0])
        assert np.array_equal(rec[:, 1].view(np.uint64), rec1[:, 0].view(np.uint64))
    assert (rec[:, 0, 2] == 2.0).all() and (rec[:, 0, 3] == nleap).all()
    assert np.array_equal(got[0].view(np.uint32), start[0].view(np.uint32))
    assert got[0].view(np.uint32)[Lz - 1, Ly - 1, 3] == start[0].view(np.uint32)[Lz - 1, Ly - 1, 3]
    assert hmc.reaches(start[0], CLAMP)
    for r in range(2):
        fields, verdicts, _ = check_trajectories(dev_oracle, shape, _params(sampler, shape, r), start[r], COUNTERS[r],
                                                 rec[:, r], nleap, False)
        assert np.array_equal(got[r].view(np.uint32), fields[-1].view(np.uint32)), r
        assert (verdicts == [2, 2, 2]) if r == 0 else (2 not in verdicts)


# 5. the length limit -------------------------------------------------------------------------------------------

MAX_LEAP = 4096


def _limit_ens(shape, R):
    """The three replicas from init_field(0.5) at the HMC tests' dtau = 0.4 / sqrt(V).  That is small enough:
    sig w stays below 2 for every mode, the leapfrog steps are stable, and over 4096 of them the CPU oracle's
    fields stay below 5.1 at (64, 11, 29) and 2.5 at (8, 2, 2), under a clamp of 1000."""
    E = hmc._ens(shape, R)
    E.init_field(0.5)
    E.step_counter = COUNTERS[:R]
    return E, hmc._dtau(shape)


@pytest.mark.parametrize("shape,R", [((8, 2, 2), 3), ((64, 11, 29), 1)])
def test_the_longest_trajectory(gpu, dev_oracle, shape, R):
    """One trajectory of nleap = 4096 = SQ_PHI4_ENS_MAX_LEAP steps, followed through the oracle; the fourth
    counter is 4096."""
    assert_shape(shape)
    E, dt = _limit_ens(shape, R)
    with E:
        start = E.download()
        _, rec = E.step_hmc(1, nleap=MAX_LEAP, record=True)
        got, stats, flags = E.download(), E.hmc_stats(), E.flags()
        assert list(E.step_counter) == [c + 1 for c in COUNTERS[:R]]
    assert stats[:, 3].tolist() == [MAX_LEAP] * R and stats[:, 0].tolist() == [1] * R and not flags.any()
    for r in range(R):
        par = (dt, M2[r], LAM[r], CS[r], SEEDS[r])
        fields, verdicts, lengths = check_trajectories(dev_oracle, shape, par, start[r], COUNTERS[r], rec[:, r],
                                                       MAX_LEAP, False)
        assert lengths == [MAX_LEAP] and verdicts[0] in (0, 1) and same_bits(got[r], fields[0])
        assert stats[r].tolist() == [1, verdicts[0], 0, MAX_LEAP]
        print(f"LIMIT {shape} replica {r} dH {rec[0, r, 0]:+.6e} verdict {verdicts[0]}", flush=True)


def test_randomised_lengths_up_to_the_limit(gpu, dev_oracle):
    """Eight trajectories with nleap = 4096 and randomize: every L is 1 + (o.y >> 20), the fourth counter their
    sum, the fields the oracle's."""
    shape = (8, 2, 2)
    assert_shape(shape)
    E, dt = _limit_ens(shape, 3)
    with E:
        start = E.download()
        _, rec = E.step_hmc(8, nleap=MAX_LEAP, randomize=True, record=True)
        got, stats, flags = E.download(), E.hmc_stats(), E.flags()
    assert not flags.any()
    for r in range(3):
        par = (dt, M2[r], LAM[r], CS[r], SEEDS[r])
        want = [1 + (int(accept_block(dev_oracle, SEEDS[r], COUNTERS[r] + k)[1]) >> 20) for k in range(8)]
        assert rec[:, r, 3].tolist() == [float(L) for L in want] and len(set(want)) >= 2 and max(want) > 64
        fields, verdicts, lengths = check_trajectories(dev_oracle, shape, par, start[r], COUNTERS[r], rec[:, r],
                                                       MAX_LEAP, True)
        assert lengths == want and same_bits(got[r], fields[-1])
        assert stats[r].tolist() == [8, verdicts.count(1), 0, sum(want)]
        print(f"LIMIT randomised replica {r} lengths {want} verdicts {verdicts}", flush=True)


# 7. the interacting law at C != 1 ------------------------------------------------------------------------------

LAW_DTAU = {"hmc": 0.025, "mala": 0.025}


def _metropolis():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "phi4_metropolis.json")) as fh:
        return json.load(fh)


@pytest.mark.parametrize("sampler", SAMPLERS)
def test_the_interacting_law_against_metropolis(gpu, sampler):
    """8 x 4 x 4 lattices, R = 256, m2 = 0.25, lam = 6, C = 0.7: the samplers' <phi^2> against the value of an
    independent float64 checkerboard Metropolis sampler of exp(-S / C^2) (tests/golden/phi4_metropolis.json; the
    CPU suite shows that the free and the C = 1 values lie far from it).  HMC: 300 Heun steps, then 1500
    trajectories of nleap = 8, randomised, a record each.  MALA: 300 Heun steps, then 4000 steps with a record
    every 10, the first quarter dropped.  <phi^2> = S2 / 128 per replica, the error from the 256 replica means.

    Asserted: |mean - ref| < 4 sqrt(sem^2 + sem_ref^2); <exp(-dH)> over all records within 4 standard errors of
    1; the acceptance in [0.6, 0.9] (the float32 definition composed from the CPU oracle, 12 replicas of 50
    trajectories from thermalised fields, gave 0.73 for HMC and 0.77 for MALA at dtau = 0.025, and 0.82 / 0.86 at
    0.02, 0.69 / 0.70 at 0.03); no flags."""
    ref = _metropolis()
    tgt = ref["target"]
    shape, R = tuple(ref["shape"]), 256
    assert shape == (8, 4, 4) and (tgt["m2"], tgt["lam"], tgt["C"]) == (0.25, 6.0, 0.7)
    with hmc._ens(shape, R, dtau=LAW_DTAU[sampler], m2=tgt["m2"], lam=tgt["lam"], C=tgt["C"], seeds=None,
                  seed=4242) as E:
        E.step(300, scheme="heun")
        if sampler == "hmc":
            ser, rec = E.step_hmc(1500, nleap=8, randomize=True, every=1, record=True)
            n = 1500
        else:
            ser, rec = E.step_mala(4000, every=10, record=True)
            ser, n = ser[100:], 4000
        assert not E.flags().any()
        stats = _stats(E, sampler)
    per = ser[:, :, 1].mean(axis=0) / 128.0
    mean, sem = float(per.mean()), float(per.std(ddof=1) / np.sqrt(R))
    acc = float(stats[:, 1].sum()) / float(stats[:, 0].sum())
    w = np.exp(-rec[:, :, 0]).mean(axis=0)
    wm, ws = float(w.mean()), float(w.std(ddof=1) / np.sqrt(R))
    err = math.sqrt(sem * sem + tgt["sem"] ** 2)
    print(f"LAW {sampler} dtau {LAW_DTAU[sampler]} PHI2 {mean:.6f} +- {sem:.6f}  metropolis {tgt['phi2']:.6f} +- "
          f"{tgt['sem']:.6f}  deviation {(mean - tgt['phi2']) / err:+.2f} sigma  acceptance {acc:.4f}  "
          f"<exp(-dH)> {wm:.6f} +- {ws:.6f}  free {ref['free']['phi2']:.6f}  C=1 {ref['unit_noise']['phi2']:.6f}",
          flush=True)
    assert stats[:, 0].tolist() == [n] * R and not stats[:, 2].any()
    assert abs(mean - tgt["phi2"]) < 4.0 * err, (mean, sem, tgt)
    assert abs(wm - 1.0) < 4.0 * ws, (wm, ws)
    assert 0.6 <= acc <= 0.9, acc
