"""The QM1D replica ensemble (Qm1dEnsemble, sq_ens_*, csrc/sq_qm1d_ens.hip) on
the MI355X: replica r must equal, bit for bit, what the oracle's Jacobi frame
(oracle.qm1d_frame, fed the device's Box-Muller factors when C != 0) and the
single-chain path (Qm1dChain) give for that replica's seed and state.  The
ensemble is never checked against itself.

Shapes: a = 0.1, h = 0.002; N covers touching boundaries (2, 3), a partial
wave (17), the wave and K boundaries (64, 65, 129), multi-wave (257, 1025)
and the maximum (4096)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

A, H = 0.1, 0.002


def _state(N, seed=3, amp=0.05):
    rng = np.random.default_rng(seed)
    return rng.normal(0, amp, N), rng.normal(0, amp, N), rng.normal(0, amp, N)


def _states(N, R):
    """Per-replica distinct f, x, xx0 of shape (R, N)."""
    s = [_state(N, seed=3 + r) for r in range(R)]
    return tuple(np.stack([t[k] for t in s]) for k in range(3))


def _frame_case(orc, N, pot, C, R=5, loops=41, tick=7):
    """One ensemble frame of R replicas with distinct states vs the oracle, everything bit for bit."""
    from stochquant_amd import Qm1dEnsemble
    seeds = np.arange(1000, 1000 + R, dtype=np.uint64)
    f, x, xx0 = _states(N, R)
    om = N * A / 2 + 0.013 + 0.01 * np.arange(R)
    runs = 3 + np.arange(R)
    with Qm1dEnsemble(N, A, H, R, seeds=seeds, pot=pot, C=C, loops=loops, adapt_dtau=False) as e:
        e.upload(f, x, xx0, om, runs)
        e.set_scan(0, 1.0, tick)
        st = e.run_frame()
        d = e.download()
        sc = e.scan
    for r in range(R):
        ref = orc.qm1d_frame(N, A, H, pot, C, loops, int(seeds[r]), tick, int(runs[r]), f[r], x[r], xx0[r], om[r], 0, 1.0)
        assert ref["stable"] == 1 and st[r], (r, ref["steps_done"])
        for k in ("f", "x", "xx0"):
            assert np.array_equal(d[k][r], ref[k]), (r, k, np.max(np.abs(d[k][r] - ref[k])))
        assert d["omega"][r] == ref["omega"]
        assert d["runs"][r] == runs[r] + loops
        assert sc["lrgEl"][r] == ref["lrgEl"] and sc["lrgVl"][r] == ref["lrgVl"]
        assert sc["tick"][r] == tick + loops


@pytest.mark.parametrize("pot", [0, 3])
@pytest.mark.parametrize("N", [2, 3, 17, 64, 65, 129, 257, 1025, 4096])
def test_frame_bitwise(gpu, dev_oracle, N, pot):
    """tick 7 is no multiple of 4 and loops = 41 is odd: the noise hand-round's edges."""
    _frame_case(dev_oracle, N, pot, 1.0)


@pytest.mark.parametrize("pot", [0, 3])
@pytest.mark.parametrize("N", [2, 17, 200, 4096])
def test_frame_bitwise_noiseless(gpu, oracle_mod, N, pot):
    _frame_case(oracle_mod, N, pot, 0.0)


def test_mixed_verdicts(gpu, dev_oracle):
    """Some replicas lose the frame: they keep f, x, xx0, omega and runs, while
    lrgEl / lrgVl are the frame's and the tick has advanced."""
    from stochquant_amd import Qm1dEnsemble
    N, R, loops = 17, 24, 10
    seeds = np.arange(1000, 1000 + R, dtype=np.uint64)
    f, x, xx0 = _state(N)
    om = N * A / 2 + 0.013
    with Qm1dEnsemble(N, A, H, R, seeds=seeds, pot=0, C=1.0, loops=loops, adapt_dtau=False) as e:
        e.upload(f, x, xx0, om, 3)
        e.set_scan(0, 0.02, 0)
        st = e.run_frame()
        d = e.download()
        sc = e.scan
    refs = [dev_oracle.qm1d_frame(N, A, H, 0, 1.0, loops, int(s), 0, 3, f, x, xx0, om, 0, 0.02) for s in seeds]
    n_unstable = sum(r["stable"] != 1 for r in refs)
    assert 0 < n_unstable < R
    for r, ref in enumerate(refs):
        assert bool(st[r]) == (ref["stable"] == 1), r
        assert sc["lrgEl"][r] == ref["lrgEl"] and sc["lrgVl"][r] == ref["lrgVl"], r
        assert sc["tick"][r] == loops
        if ref["stable"] == 1:
            for k in ("f", "x", "xx0"):
                assert np.array_equal(d[k][r], ref[k]), (r, k)
            assert d["omega"][r] == ref["omega"] and d["runs"][r] == 3 + loops
        else:
            assert np.array_equal(d["f"][r], f) and np.array_equal(d["x"][r], x) and np.array_equal(d["xx0"][r], xx0)
            assert d["omega"][r] == om and d["runs"][r] == 3


def _chains(N, seeds, pot, loops, f, x, xx0, om, runs, lrgVl, nframes, dtau0=None, adapt=True):
    """The same frames on one Qm1dChain per seed, frame by frame: verdicts (nframes, R), final states."""
    from stochquant_amd import Qm1dChain
    R = len(seeds)
    verdicts = np.zeros((nframes, R), dtype=bool)
    out = []
    for r, s in enumerate(seeds):
        with Qm1dChain(N, A, H, pot=pot, C=1.0, loops=loops, seed=int(s), adapt_dtau=adapt) as q:
            q.upload(f, x, xx0, om, runs)
            q.set_scan(0, lrgVl, 0)
            if dtau0 is not None:
                q.dtau = dtau0[r]
            for k in range(nframes):
                verdicts[k, r] = q.run_frame()
            out.append((q.download(), q.scan, q.dtau))
    return verdicts, out


def _assert_equals_chains(e, out):
    d, sc, dt = e.download(), e.scan, e.dtau
    for r, (cd, csc, cdt) in enumerate(out):
        for k in ("f", "x", "xx0"):
            assert np.array_equal(d[k][r], cd[k]), (r, k)
        assert d["omega"][r] == cd["omega"] and d["runs"][r] == cd["runs"], r
        assert sc["lrgEl"][r] == csc["lrgEl"] and sc["lrgVl"][r] == csc["lrgVl"] and sc["tick"][r] == csc["tick"], r
        assert dt[r] == cdt, (r, dt[r], cdt)


def test_frames_and_dtau_control(gpu):
    """run_frames(14) as one call, and as 14 run_frame calls, against 16 single
    chains run frame by frame: verdict matrix, final state, scan state, Δτ."""
    from stochquant_amd import Qm1dEnsemble
    N, R, loops, nframes = 17, 16, 5, 14
    seeds = np.arange(1000, 1000 + R, dtype=np.uint64)
    f, x, xx0 = _state(N)
    om = N * A / 2 + 0.013
    want, out = _chains(N, seeds, 0, loops, f, x, xx0, om, 3, 0.02, nframes)
    assert not want[0].all() and want[0].any()     # some replicas lose frame 0, some do not
    dts = np.array([o[2] for o in out])
    near = lambda v: np.isclose(dts, v, rtol=1e-12, atol=0)
    assert near(H).any() and near(H / 0.95).any() and (near(H) | near(H / 0.95)).all()
    with Qm1dEnsemble(N, A, H, R, seeds=seeds, pot=0, C=1.0, loops=loops) as e:
        e.upload(f, x, xx0, om, 3)
        e.set_scan(0, 0.02, 0)
        got = e.run_frames(nframes)
        assert got.shape == (nframes, R) and np.array_equal(got, want)
        _assert_equals_chains(e, out)
    with Qm1dEnsemble(N, A, H, R, seeds=seeds, pot=0, C=1.0, loops=loops) as e:
        e.upload(f, x, xx0, om, 3)
        e.set_scan(0, 0.02, 0)
        got = np.stack([e.run_frame() for _ in range(nframes)])
        assert np.array_equal(got, want)
        _assert_equals_chains(e, out)


def test_dtau_setter_acts_on_one_replica(gpu):
    from stochquant_amd import Qm1dEnsemble
    N, R, loops = 100, 4, 5
    seeds = np.arange(1000, 1000 + R, dtype=np.uint64)
    f, x, xx0 = np.zeros(N), np.zeros(N), np.zeros(N)
    dt0 = np.full(R, H)
    dt0[2] = 0.5                                    # Δτ/Δt² = 50: diverges
    want, out = _chains(N, seeds, 3, loops, f, x, xx0, 5.0, 0, 1.0, 1, dtau0=dt0)
    assert list(want[0]) == [True, True, False, True]
    with Qm1dEnsemble(N, A, H, R, seeds=seeds, pot=3, C=1.0, loops=loops) as e:
        e.upload(f, omega=5.0)
        e.set_scan(0, 1.0, 0)
        d = e.dtau
        assert np.array_equal(d, np.full(R, H))
        d[2] = 0.5
        e.dtau = d
        st = e.run_frame()
        assert list(st) == [True, True, False, True]
        assert e.dtau[2] == 0.5 * 0.95 and np.array_equal(np.delete(e.dtau, 2), np.full(R - 1, H))
        _assert_equals_chains(e, out)


def test_independent_of_ensemble_size_and_position(gpu, dev_oracle):
    """Seed s at index 1 of 3 replicas and at index 288 of 300 (more work-groups
    than CUs): the same bits, the oracle's; equal seeds with equal state give
    equal replicas, different seeds differ."""
    from stochquant_amd import Qm1dEnsemble
    N, loops, s = 65, 10, 4242
    f, x, xx0 = _state(N)
    om = N * A / 2 + 0.013
    res = []
    for R, idx in ((3, 1), (300, 288)):
        seeds = np.full(R, 7, dtype=np.uint64)
        seeds[idx] = s
        with Qm1dEnsemble(N, A, H, R, seeds=seeds, pot=3, C=1.0, loops=loops, adapt_dtau=False) as e:
            e.upload(f, x, xx0, om, 3)
            e.set_scan(0, 1.0, 5)
            st = e.run_frame()
            res.append((st, e.download(), e.scan, idx))
    ref = dev_oracle.qm1d_frame(N, A, H, 3, 1.0, loops, s, 5, 3, f, x, xx0, om, 0, 1.0)
    ref7 = dev_oracle.qm1d_frame(N, A, H, 3, 1.0, loops, 7, 5, 3, f, x, xx0, om, 0, 1.0)
    assert ref["stable"] == 1 and ref7["stable"] == 1
    for st, d, sc, idx in res:
        assert st.all()
        for k in ("f", "x", "xx0"):
            assert np.array_equal(d[k][idx], ref[k]), k
            others = np.delete(d[k], idx, axis=0)
            assert np.array_equal(others, np.broadcast_to(ref7[k], others.shape)), k   # equal seeds: equal replicas
        assert d["omega"][idx] == ref["omega"] and sc["lrgVl"][idx] == ref["lrgVl"] and sc["lrgEl"][idx] == ref["lrgEl"]
        assert not np.array_equal(d["f"][idx], d["f"][0])                               # different seeds differ


def test_large_ensemble(gpu, dev_oracle):
    """R = 8193 (default seeds seed + r): replicas 0, 4096 and 8192 against the
    oracle, and perf() counts the steps every replica ran."""
    from stochquant_amd import Qm1dEnsemble
    N, R, loops, seed = 64, 8193, 10, 0x5EED
    f, x, xx0 = _state(N)
    om = N * A / 2 + 0.013
    with Qm1dEnsemble(N, A, H, R, pot=0, C=1.0, loops=loops, seed=seed, adapt_dtau=False) as e:
        e.upload(f, x, xx0, om, 3)
        e.set_scan(0, 1.0, 0)
        st = e.run_frame()
        d = e.download()
        sc = e.scan
        perf = e.perf()
    steps = 0
    for r in range(R):
        ref = dev_oracle.qm1d_frame(N, A, H, 0, 1.0, loops, seed + r, 0, 3, f, x, xx0, om, 0, 1.0)
        steps += ref["steps_done"]
        assert bool(st[r]) == (ref["stable"] == 1), r
        if r in (0, 4096, 8192):
            assert ref["stable"] == 1
            for k in ("f", "x", "xx0"):
                assert np.array_equal(d[k][r], ref[k]), (r, k)
            assert d["omega"][r] == ref["omega"] and sc["lrgEl"][r] == ref["lrgEl"] and sc["lrgVl"][r] == ref["lrgVl"]
    assert perf["steps"] == steps and perf["site_updates"] == steps * N
    assert perf["kernel_launches"] == 1


def test_correlator(gpu):
    """mean and standard error over the replicas against numpy on the downloaded
    state; per site the bound is the summation-order bound R 2^-52 sum |c_r|."""
    from stochquant_amd import Qm1dEnsemble
    N, R = 17, 7
    f, x, xx0 = _states(N, R)
    with Qm1dEnsemble(N, A, H, R, pot=0, C=1.0, loops=5, adapt_dtau=False) as e:
        e.upload(f, x, xx0, N * A / 2, 3)
        e.set_scan(0, 1.0, 0)
        e.run_frame()
        d = e.download()
        mean, err = e.correlator()
    c = d["xx0"] - d["x"] * d["x"][:, N // 2][:, None]
    bound = R * 2.0 ** -52 * np.abs(c).sum(axis=0)
    assert mean.shape == (N,) and err.shape == (N,)
    assert np.all(np.abs(mean - c.mean(axis=0)) <= bound)
    assert np.all(np.abs(err - c.std(axis=0, ddof=1) / np.sqrt(R)) <= bound)
    assert np.all(err > 0)
    with Qm1dEnsemble(N, A, H, 1, pot=0, C=1.0, loops=5, adapt_dtau=False) as e:
        e.upload(f[0], x[0], xx0[0], N * A / 2, 3)
        mean, err = e.correlator()
    assert np.array_equal(mean, xx0[0] - x[0] * x[0][N // 2])
    assert np.array_equal(err, np.zeros(N))


def test_partial_ranges(gpu):
    from stochquant_amd import Qm1dEnsemble, StochQuantError
    N, R = 17, 6
    f, x, xx0 = _states(N, R)
    with Qm1dEnsemble(N, A, H, R, pot=0, loops=5) as e:
        e.upload(f[0])                                           # (N,): every replica
        e.upload(f[2:5], x[2:5], xx0[2:5], np.array([1.0, 2.0, 3.0]), np.array([7, 8, 9]), first=2)
        d = e.download()
        assert np.array_equal(d["f"][[0, 1, 5]], np.broadcast_to(f[0], (3, N)))
        assert np.array_equal(d["f"][2:5], f[2:5]) and np.array_equal(d["x"][2:5], x[2:5])
        assert np.array_equal(d["xx0"][2:5], xx0[2:5]) and not d["x"][[0, 1, 5]].any()
        assert list(d["omega"]) == [0, 0, 1, 2, 3, 0] and list(d["runs"]) == [0, 0, 7, 8, 9, 0]
        p = e.download(first=3, count=2)
        assert np.array_equal(p["f"], f[3:5]) and list(p["runs"]) == [8, 9]
        for first, count in ((5, 2), (-1, 1), (0, R + 1), (R + 1, 0)):
            with pytest.raises(StochQuantError) as ei:
                e.download(first=first, count=count)
            assert ei.value.code == -1
        with pytest.raises(StochQuantError) as ei:
            e.upload(f[0:3], first=4)
        assert ei.value.code == -1
