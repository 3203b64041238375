"""The QM1D replica ensemble's kernel instances and frame edges on the MI355X
(Qm1dEnsemble, csrc/sq_qm1d_ens.hip), bit for bit against the oracle's Jacobi
frame (oracle.qm1d_frame with the device's Box-Muller factors).  The ensemble
is never compared with itself.  a = 0.1, h = 0.002.

The instances qm1d_ens_frame<K, MW, P3, HELP> that qm1d_wave_shape reaches
without a tuning override, and the shape that stands for each here:

    N            K  waves  potID 0            potID 3
    2 .. 64      1  1      one wave  (64, 0)  HELP      (17, 3)
    65 .. 128    2  1      one wave (100, 0)  HELP     (100, 3)
    129 .. 256   1  3..4   multi-wave         multi-wave (200, 3)
    257 .. 4096  4  2..16  multi-wave (1025, 0), (1025, 3): the last wave holds
                           one site; (4096, *): 16 full waves

<K=2, multi-wave>, <K=4, one wave> and <K=1, 16 waves> run only under the
SQ_QM1D_K override, which is read once per process:
tests/test_gpu_qm1d_forced_k.py.

What the cases add to tests/test_gpu_qm1d_ens.py: frames longer than one
64-step omega batch and than one 8-step helper chunk, and of whole chunks and
batches (test_long_frames); a frame that starts at lrgEl != 0, at a tick whose
high word is not 0 or changes inside the frame, and at a large `runs`
(test_frame_start_state); unstable frames in every instance, before and after
the first chunk and the first batch (test_unstable_ladder), and the state a
replica carries into the frames after one (test_frames_after_unstable); the
correlator on more than one block and with n < N (test_correlator_blocks)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A, H = 0.1, 0.002

# (N, pot) -> the instance it reaches
SHAPES = [
    (17, 3),     # <1, one wave, HELP>
    (100, 3),    # <2, one wave, HELP>
    (64, 0),     # <1, one wave>, every lane occupied
    (100, 0),    # <2, one wave>, 50 lanes
    (200, 3),    # <1, multi-wave>, W = 4, the last wave holds 8 sites
    (1025, 0),   # <4, multi-wave>, W = 5, the last wave holds one site
    (1025, 3),   # <4, multi-wave, potID 3>, W = 5
]
BIG = [(4096, 0), (4096, 3)]   # <4, multi-wave>, W = 16, every lane occupied


def _state(N, seed=3, amp=0.05):
    rng = np.random.default_rng(seed)
    return rng.normal(0, amp, N), rng.normal(0, amp, N), rng.normal(0, amp, N)


def _states(N, R):
    """Per-replica distinct f, x, xx0 of shape (R, N) (tests/test_gpu_qm1d_ens.py's recipe)."""
    s = [_state(N, seed=3 + r) for r in range(R)]
    return tuple(np.stack([t[k] for t in s]) for k in range(3))


def _assert_adopted(d, sc, r, ref, runs_after, tick_after):
    """Replica r holds the oracle's frame: field, means, omega, runs, scan state."""
    for k in ("f", "x", "xx0"):
        assert np.array_equal(d[k][r], ref[k]), (r, k, np.max(np.abs(d[k][r] - ref[k])))
    assert d["omega"][r] == ref["omega"], (r, d["omega"][r], ref["omega"])
    assert int(d["runs"][r]) == runs_after, (r, d["runs"][r])
    _assert_scan(sc, r, ref, tick_after)


def _assert_scan(sc, r, ref, tick_after):
    assert sc["lrgEl"][r] == ref["lrgEl"], (r, sc["lrgEl"][r], ref["lrgEl"])
    assert sc["lrgVl"][r] == ref["lrgVl"], (r, sc["lrgVl"][r], ref["lrgVl"])
    assert int(sc["tick"][r]) == tick_after, (r, sc["tick"][r])


def _stable_case(orc, N, pot, loops, lrgEl=0, tick=7, runs0=3, R=3):
    """One frame of R replicas with distinct seeds and states, none of which may
    fire, against the oracle: f, x, xx0, omega, runs, lrgEl, lrgVl, tick, verdict."""
    from stochquant_amd import Qm1dEnsemble
    seeds = np.arange(1000, 1000 + R, dtype=np.uint64)
    f, x, xx0 = _states(N, R)
    om = N * A / 2 + 0.013 + 0.01 * np.arange(R)
    runs = runs0 + np.arange(R)
    with Qm1dEnsemble(N, A, H, R, seeds=seeds, pot=pot, C=1.0, loops=loops, adapt_dtau=False) as e:
        e.upload(f, x, xx0, om, runs)
        e.set_scan(lrgEl, 1.0, tick)
        st = e.run_frame()
        d = e.download()
        sc = e.scan
        dt = e.dtau
    for r in range(R):
        ref = orc.qm1d_frame(N, A, H, pot, 1.0, loops, int(seeds[r]), tick, int(runs[r]), f[r], x[r], xx0[r], om[r],
                             lrgEl, 1.0)
        assert ref["stable"] == 1 and ref["steps_done"] == loops, (r, ref["steps_done"])
        assert st[r], r
        _assert_adopted(d, sc, r, ref, int(runs[r]) + loops, tick + loops)
        assert dt[r] == H


# ---- a. long frames --------------------------------------------------------

@pytest.mark.parametrize("loops", [8, 16, 63, 64, 65, 128, 130])
@pytest.mark.parametrize("N,pot", SHAPES)
def test_long_frames(gpu, dev_oracle, N, pot, loops):
    """loops = 8, 16: whole helper chunks; 63, 65: either side of one omega batch;
    64, 128: om_end is the batch's carry; 65, 128, 130: a second batch is drawn
    at j = 64, and the helper tables cross it."""
    _stable_case(dev_oracle, N, pot, loops)


@pytest.mark.parametrize("loops", [64, 130])
@pytest.mark.parametrize("N,pot", BIG)
def test_long_frames_4096(gpu, dev_oracle, N, pot, loops):
    _stable_case(dev_oracle, N, pot, loops)


# ---- b. the frame-start state ----------------------------------------------

# 2^32 - 20: the high word changes at step 20 of the frame; 2^32 - 3: at step 3,
# inside the first site_noise group of K = 1 (steps 0..3); 2^40 + 5: high word 256
TICKS = [2 ** 32 - 20, 2 ** 32 - 3, 2 ** 40 + 5]


@pytest.mark.parametrize("tick", TICKS)
@pytest.mark.parametrize("where", ["last", "mid", "one"])
@pytest.mark.parametrize("N,pot", SHAPES + BIG)
def test_frame_start_state(gpu, dev_oracle, N, pot, where, tick):
    """lrgEl = N - 1: the last site of the last occupied lane (in multi-wave
    shapes a wave other than 0 posts X' at lrgEl); N // 2: with K = 2 the second
    site of a lane when N // 2 is odd, with K = 4 site N // 2 % 4; 1: lane 0's
    second site when K > 1."""
    lrgEl = {"last": N - 1, "mid": N // 2, "one": 1}[where]
    _stable_case(dev_oracle, N, pot, 41, lrgEl=lrgEl, tick=tick)


@pytest.mark.parametrize("N,pot", SHAPES + BIG)
def test_frame_start_large_runs(gpu, dev_oracle, N, pot):
    """runs = 2 * 10^9: the running means' divisor runs + j + 1 stays below
    2^31 and inside udiv_prep's range, and their numerators are far smaller than
    it (K = 4 takes the shared-reciprocal quotient, K < 4 the full division)."""
    _stable_case(dev_oracle, N, pot, 41, lrgEl=N // 2, tick=2 ** 32 - 3, runs0=2_000_000_000)


# ---- c. unstable frames in every instance ------------------------------------

LADDER = [0.00450 + 0.00005 * k for k in range(10)]
LADDER_SEEDS = (1000, 1001, 1002)
LADDER_LOOPS, LADDER_TICK, LADDER_RUNS = 130, 7, 3
# shapes of which one replica at least must fire after step 64 (the second
# omega batch, helper chunk 8 and later); with the oracle's own transcendentals
# the firing steps after 64 are 119..124 at (17, 3), 89..121 at (100, 3), 81 and
# 124 at (200, 3) and 90 at (1025, 3)
LATE = {(17, 3), (100, 3), (200, 3), (1025, 3)}
# at N = 4096 four replicas as (seed, rung): stable, fired late, fired early twice
# (with the oracle's own transcendentals: 0, 76, 37, 6 and 0, 36, 8, 6)
PICKS_4096 = {0: [(1000, 7), (1000, 8), (1000, 9), (1002, 3)],
              3: [(1000, 1), (1000, 2), (1000, 9), (1002, 9)]}


def _ladder_groups(N, pot):
    """The ensembles of one shape as lists of (seed, Δτ): one per seed with the
    whole ladder, or the four picked replicas at N = 4096."""
    if N == 4096:
        return [[(s, LADDER[k]) for s, k in PICKS_4096[pot]]]
    return [[(s, dt) for dt in LADDER] for s in LADDER_SEEDS]


def _ladder_refs(orc, N, pot, groups):
    f, x, xx0 = _state(N)
    om = N * A / 2 + 0.013
    refs = [[orc.qm1d_frame(N, A, dt, pot, 1.0, LADDER_LOOPS, s, LADDER_TICK, LADDER_RUNS, f, x, xx0, om, 0, 1.0)
             for s, dt in g] for g in groups]
    flat = [r for g in refs for r in g]
    fired = [r["steps_done"] for r in flat if r["stable"] != 1]
    print(f"LADDER N={N} pot={pot} stable={len(flat) - len(fired)} fired_at={sorted(fired)}", flush=True)
    # the conditions that keep the comparison from passing vacuously
    assert len(fired) < len(flat), "no stable replica"
    assert any(s > 8 for s in fired), "no replica fires after the first helper chunk"
    if (N, pot) in LATE:
        assert any(s > 64 for s in fired), "no replica fires after the first omega batch"
    return (f, x, xx0, om), refs


@pytest.mark.parametrize("N,pot", SHAPES + [(64, 3), (200, 0)] + BIG)   # (64, 3): HELP with every lane occupied
def test_unstable_ladder(gpu, dev_oracle, N, pot):
    """Replicas that start from one state on a ladder of Δτ: some hold, some
    fire, early and late in the frame.  A replica that fired keeps f, x, xx0,
    omega and runs as uploaded; lrgEl, lrgVl and the tick are the frame's."""
    from stochquant_amd import Qm1dEnsemble
    groups = _ladder_groups(N, pot)
    (f, x, xx0, om), refs = _ladder_refs(dev_oracle, N, pot, groups)
    for g, gref in zip(groups, refs):
        R = len(g)
        seeds = np.array([s for s, _ in g], dtype=np.uint64)
        dts = np.array([dt for _, dt in g])
        with Qm1dEnsemble(N, A, H, R, seeds=seeds, pot=pot, C=1.0, loops=LADDER_LOOPS, adapt_dtau=False) as e:
            e.upload(f, x, xx0, om, LADDER_RUNS)
            e.set_scan(0, 1.0, LADDER_TICK)
            e.dtau = dts
            st = e.run_frame()
            d = e.download()
            sc = e.scan
            perf = e.perf()
            assert np.array_equal(e.dtau, dts)
        for r, ref in enumerate(gref):
            assert bool(st[r]) == (ref["stable"] == 1), (r, g[r], ref["steps_done"])
            if ref["stable"] == 1:
                _assert_adopted(d, sc, r, ref, LADDER_RUNS + LADDER_LOOPS, LADDER_TICK + LADDER_LOOPS)
            else:
                _assert_scan(sc, r, ref, LADDER_TICK + LADDER_LOOPS)
                assert np.array_equal(d["f"][r], f) and np.array_equal(d["x"][r], x), (r, g[r])
                assert np.array_equal(d["xx0"][r], xx0), (r, g[r])
                assert d["omega"][r] == om and int(d["runs"][r]) == LADDER_RUNS, (r, g[r])
        steps = sum(ref["steps_done"] for ref in gref)
        assert perf["steps"] == steps and perf["site_updates"] == steps * N


# ---- d. the frames after an unstable one --------------------------------------

def _controller(dtau, cnt, stable):
    """sq_qm1d_ens.hip's Δτ controller: (Δτ, stable-frame count) after a frame."""
    if stable:
        if cnt > 10:
            cnt = 0
            dtau = dtau / 0.950
        cnt += 1
    else:
        dtau = dtau * 0.950
        cnt = 0
    return dtau, cnt


@pytest.mark.parametrize("N,pot", [(100, 3), (1025, 3)])
def test_frames_after_unstable(gpu, dev_oracle, N, pot):
    """run_frames(3) with the controller on, against the oracle chained frame by
    frame: a frame that fired leaves f, x, xx0, omega and runs to the next one
    but hands it its own lrgEl, lrgVl, tick + loops and Δτ * 0.950."""
    from stochquant_amd import Qm1dEnsemble
    nframes, loops = 3, LADDER_LOOPS
    f0, x0, xx00 = _state(N)
    om0 = N * A / 2 + 0.013
    patterns = []
    for seed in LADDER_SEEDS:
        R = len(LADDER)
        want = np.zeros((nframes, R), dtype=bool)
        end = []
        for r, dt in enumerate(LADDER):
            f, x, xx0, om, runs = f0, x0, xx00, om0, LADDER_RUNS
            E, V, tick, cnt = 0, 1.0, LADDER_TICK, 0
            for k in range(nframes):
                ref = dev_oracle.qm1d_frame(N, A, dt, pot, 1.0, loops, seed, tick, runs, f, x, xx0, om, E, V)
                want[k, r] = ref["stable"] == 1
                E, V, tick = ref["lrgEl"], ref["lrgVl"], tick + loops
                if want[k, r]:
                    f, x, xx0, om, runs = ref["f"], ref["x"], ref["xx0"], ref["omega"], runs + loops
                dt, cnt = _controller(dt, cnt, want[k, r])
            end.append((f, x, xx0, om, runs, E, V, tick, dt))
            patterns.append("".join("s" if v else "u" for v in want[:, r]))
        with Qm1dEnsemble(N, A, H, R, seeds=np.full(R, seed, dtype=np.uint64), pot=pot, C=1.0, loops=loops) as e:
            e.upload(f0, x0, xx00, om0, LADDER_RUNS)
            e.set_scan(0, 1.0, LADDER_TICK)
            e.dtau = np.array(LADDER)
            got = e.run_frames(nframes)
            d, sc, dts = e.download(), e.scan, e.dtau
        assert got.shape == (nframes, R) and np.array_equal(got, want), (seed, got, want)
        for r, (f, x, xx0, om, runs, E, V, tick, dt) in enumerate(end):
            assert np.array_equal(d["f"][r], f) and np.array_equal(d["x"][r], x), (seed, r)
            assert np.array_equal(d["xx0"][r], xx0), (seed, r)
            assert d["omega"][r] == om and int(d["runs"][r]) == runs, (seed, r)
            assert sc["lrgEl"][r] == E and sc["lrgVl"][r] == V and int(sc["tick"][r]) == tick, (seed, r)
            assert dts[r] == dt, (seed, r, dts[r], dt)
    print(f"FRAMES N={N} pot={pot} {patterns}", flush=True)
    # a stable frame must follow an unstable one, or nothing was carried
    assert any("us" in p for p in patterns) and "sss" in patterns


# ---- e. the correlator on several blocks ----------------------------------------

@pytest.mark.parametrize("n", [1, 64, 65, 200])
def test_correlator_blocks(gpu, n):
    """N = 200: n = 200 is four 64-thread blocks, the last one partial; n = 65 a
    second block of one thread; n < N leaves mid = N / 2 beyond the sites asked
    for.  The bound is the summation-order bound R 2^-52 sum |c_r|."""
    from stochquant_amd import Qm1dEnsemble
    N, R = 200, 5
    f, x, xx0 = _states(N, R)
    with Qm1dEnsemble(N, A, H, R, pot=0, C=1.0, loops=5, adapt_dtau=False) as e:
        e.upload(f, x, xx0, N * A / 2, 3)
        e.set_scan(0, 1.0, 0)
        assert e.run_frame().all()
        d = e.download()
        mean, err = e.correlator(n)
    c = (d["xx0"] - d["x"] * d["x"][:, N // 2][:, None])[:, :n]
    bound = R * 2.0 ** -52 * np.abs(c).sum(axis=0)
    assert mean.shape == (n,) and err.shape == (n,)
    assert np.all(np.abs(mean - c.mean(axis=0)) <= bound)
    assert np.all(np.abs(err - c.std(axis=0, ddof=1) / np.sqrt(R)) <= bound)
    assert np.all(err > 0)
