"""The QM1D kernel instances that only the SQ_QM1D_K tuning override reaches, on
the MI355X, bit for bit against the oracle's Jacobi frame (oracle.qm1d_frame
with the device's Box-Muller factors).  a = 0.1, h = 0.002.

qm1d_wave_shape (shared by Qm1dEnsemble and Qm1dChain) takes K from the override
and W = ceil(N / (64 K)) waves when that is at most 16:

    K = 4, N <= 256        <4, one wave>; potID 3 without helper waves (HELP
                           needs K <= 2).  N = 2, 3: one lane; 17: a partial last
                           lane; 255: the last lane lacks one site; 256: full
    K = 2, N > 128         <2, multi-wave>: N = 129 (W = 2, the second wave holds
                           one site), 1000 (W = 8), 2048 (W = 16, full)
    K = 1, N = 1024        <1, multi-wave> with W = 16
    K = 1, N = 4096        W would be 64: the override is ignored, K = 4

The override is read once per process, so each K runs in a child process
(tests/qm1d_forced_k.py) forked from conftest's fork server, one at a time.
Every case runs one Qm1dEnsemble frame (R = 3, loops = 70: a second omega
batch; tick = 2^32 - 9: the step counter's high word changes inside the frame;
lrgEl = N - 1) and one Qm1dChain frame with replica 0's seed and state."""
import numpy as np
import pytest

from conftest import rank_context

pytestmark = pytest.mark.gpu

A, H = 0.1, 0.002
TIMEOUT = 90
LOOPS, TICK, R = 70, 2 ** 32 - 9, 3
SEEDS = [1000, 1001, 1002]

CASES = {4: [2, 3, 17, 255, 256], 2: [129, 1000, 2048], 1: [1024, 4096]}

# the unstable ladder of tests/test_gpu_qm1d_ens_edges.py, at K = 2 with N = 1000, potID 3
LADDER = [0.00450 + 0.00005 * k for k in range(10)]
LADDER_N, LADDER_POT, LADDER_LOOPS, LADDER_TICK, LADDER_RUNS = 1000, 3, 130, 7, 3


def _state(N, seed=3, amp=0.05):
    rng = np.random.default_rng(seed)
    return rng.normal(0, amp, N), rng.normal(0, amp, N), rng.normal(0, amp, N)


def _states(N, nrep):
    """Per-replica distinct f, x, xx0 of shape (nrep, N) (tests/test_gpu_qm1d_ens.py's recipe)."""
    s = [_state(N, seed=3 + r) for r in range(nrep)]
    return tuple(np.stack([t[k] for t in s]) for k in range(3))


def run_child(k, jobs):
    """Run `jobs` in one child process under SQ_QM1D_K = k; its results, in order."""
    from qm1d_forced_k import worker_main
    ctx = rank_context()
    a, b = ctx.Pipe()
    p = ctx.Process(target=worker_main, args=(b, k, jobs), daemon=True)
    try:
        p.start()
        b.close()
        assert a.poll(TIMEOUT), "the child sent nothing"
        tag, val = a.recv()
        assert tag == "ok", val
        p.join(TIMEOUT)
        assert p.exitcode == 0
        return val
    finally:
        if p.is_alive():
            p.kill()
            p.join(5)


def _frame_jobs(N, pot):
    f, x, xx0 = _states(N, R)
    om = N * A / 2 + 0.013 + 0.01 * np.arange(R)
    runs = 3 + np.arange(R)
    common = dict(N=N, pot=pot, a=A, h=H, loops=LOOPS, lrgEl=N - 1, lrgVl=1.0, tick=TICK)
    return [dict(common, kind="ens", seeds=SEEDS, f=f, x=x, xx0=xx0, omega=om, runs=runs),
            dict(common, kind="chain", seed=SEEDS[0], f=f[0], x=x[0], xx0=xx0[0], omega=float(om[0]), runs=int(runs[0]))]


def _ref(orc, job, r=None):
    """The oracle's frame for replica r of an ensemble job, or for a chain job."""
    if r is None:
        seed, f, x, xx0, om, runs, dt = job["seed"], job["f"], job["x"], job["xx0"], job["omega"], job["runs"], job["h"]
    else:
        row = lambda v: v[r] if np.ndim(v) == 2 else v
        per = lambda v: v[r] if np.ndim(v) == 1 else v
        seed, f, x, xx0 = job["seeds"][r], row(job["f"]), row(job["x"]), row(job["xx0"])
        om, runs = per(job["omega"]), per(job["runs"])
        dt = job["h"] if job.get("dtau") is None else job["dtau"][r]
    return orc.qm1d_frame(job["N"], job["a"], float(dt), job["pot"], 1.0, job["loops"], int(seed), job["tick"],
                          int(runs), f, x, xx0, float(om), job["lrgEl"], job["lrgVl"]), f, x, xx0, float(om), int(runs)


def _check_ens(job, out, refs):
    d, sc = out["state"], out["scan"]
    for r, (ref, f, x, xx0, om, runs) in enumerate(refs):
        what = (job["N"], job["pot"], "replica", r)
        assert bool(out["stable"][r]) == (ref["stable"] == 1), what
        assert sc["lrgEl"][r] == ref["lrgEl"] and sc["lrgVl"][r] == ref["lrgVl"], what
        assert int(sc["tick"][r]) == job["tick"] + job["loops"], what
        if ref["stable"] == 1:
            for k in ("f", "x", "xx0"):
                assert np.array_equal(d[k][r], ref[k]), (what, k, np.max(np.abs(d[k][r] - ref[k])))
            assert d["omega"][r] == ref["omega"] and int(d["runs"][r]) == runs + job["loops"], what
        else:
            assert np.array_equal(d["f"][r], f) and np.array_equal(d["x"][r], x), what
            assert np.array_equal(d["xx0"][r], xx0), what
            assert d["omega"][r] == om and int(d["runs"][r]) == runs, what
    assert out["steps"] == sum(ref["steps_done"] for ref, *_ in refs), (job["N"], job["pot"])


def _check_chain(job, out, ref):
    d, sc = out["state"], out["scan"]
    what = (job["N"], job["pot"], "chain")
    assert ref["stable"] == 1 and out["stable"], what
    for k in ("f", "x", "xx0"):
        assert np.array_equal(d[k], ref[k]), (what, k, np.max(np.abs(d[k] - ref[k])))
    assert d["omega"] == ref["omega"] and d["runs"] == job["runs"] + job["loops"], what
    assert sc["lrgEl"] == ref["lrgEl"] and sc["lrgVl"] == ref["lrgVl"], what
    assert sc["tick"] == job["tick"] + job["loops"], what


@pytest.mark.parametrize("k", [4, 2, 1])
def test_forced_k_frames(gpu, dev_oracle, k):
    jobs = [j for N in CASES[k] for pot in (0, 3) for j in _frame_jobs(N, pot)]
    outs = run_child(k, jobs)
    assert len(outs) == len(jobs)
    for job, out in zip(jobs, outs):
        if job["kind"] == "ens":
            refs = [_ref(dev_oracle, job, r) for r in range(R)]
            assert all(ref["stable"] == 1 for ref, *_ in refs), (job["N"], job["pot"])
            _check_ens(job, out, refs)
            assert np.array_equal(out["dtau"], np.full(R, H))
        else:
            _check_chain(job, out, _ref(dev_oracle, job)[0])


def test_forced_k2_unstable_ladder(gpu, dev_oracle):
    """<2, multi-wave, potID 3> with W = 8: the verdict merge over the waves and
    the rollback, on the Δτ ladder for three seeds."""
    N = LADDER_N
    f, x, xx0 = _state(N)
    jobs = [dict(kind="ens", N=N, pot=LADDER_POT, a=A, h=H, loops=LADDER_LOOPS, lrgEl=0, lrgVl=1.0, tick=LADDER_TICK,
                 seeds=[s] * len(LADDER), f=f, x=x, xx0=xx0, omega=N * A / 2 + 0.013, runs=LADDER_RUNS,
                 dtau=np.array(LADDER)) for s in SEEDS]
    refs = [[_ref(dev_oracle, job, r) for r in range(len(LADDER))] for job in jobs]
    flat = [ref for g in refs for ref, *_ in g]
    fired = [ref["steps_done"] for ref in flat if ref["stable"] != 1]
    print(f"LADDER K=2 N={N} stable={len(flat) - len(fired)} fired_at={sorted(fired)}", flush=True)
    assert len(fired) < len(flat), "no stable replica"
    assert any(s > 8 for s in fired), "no replica fires after step 8"
    outs = run_child(2, jobs)
    for job, out, g in zip(jobs, outs, refs):
        _check_ens(job, out, g)
        assert np.array_equal(out["dtau"], job["dtau"])
