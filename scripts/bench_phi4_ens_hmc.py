"""Cost, acceptance and autocorrelation of the φ⁴ ensemble's hybrid Monte Carlo
trajectories (Phi4Ensemble.step_hmc), GPU only.

    python scripts/bench_phi4_ens_hmc.py [--steps 200] [--reps 5] [--out FILE] [--no-tau]
                                         [--parent-lib OTHER/libstochquant.so] [--pairs 5]

One child process under `timeout` (this process never opens the GPU) times, at
32³ R = 256, 16³ R = 1024 and 8³ R = 4096, from fields thermalised by 1000
Euler steps, these calls, interleaved round by round (`reps` rounds after a
warm-up round, medians per call):

  hmc1     step_hmc(steps, nleap=1)
  hmc10    step_hmc(steps, nleap=10)
  hmc10r   step_hmc(steps, nleap=10, randomize=True)
  mala     step(steps, scheme="mala")
  c0       step(steps) of a C = 0 ensemble of the same shape and R

Δτ is tuned per shape, before the timing, to an acceptance of 0.75 at nleap =
10 (each pilot of 200 trajectories rescales Δτ by the ratio of the spreads of dH
that the target and the measured acceptance stand for, to the power the last
two pilots measured, 1 at first).  Yardsticks, from kernels
the parent has, timed in the same process:

  T(hmc10) <= 1.15 x [T(mala) + 9 T(c0)]        per trajectory
  T(hmc1)  <= 1.15 x T(mala)

A second child (skipped with --no-tau) measures what the feature is for, at 16³
and 32³ with R = 256: the integrated autocorrelation times of Σφ² and |Σφ| from
every=1 series, for MALA at its Δτ of acceptance 0.75 and for HMC with
randomize, nleap chosen so that the mean trajectory length (nleap + 1) / 2 x σ
is near 1, Δτ tuned to acceptance 0.75; τ_int = 1/2 + Σ_{t<=W} ρ(t) with the
smallest window W >= 20 τ_int, ρ averaged over the replicas; and the products
τ_int x wall time per update.

--parent-lib: the existing calls must not move.  step(steps), step(steps,
scheme="heun"), step(steps, scheme="mala") and run_frames(50) at 32³ R = 256
with this build and with another build of the library (SQ_LIB), in interleaved
rounds of child processes, the other build first and then twice in a row as
well: the spread of the other build against itself is the allowance.
Writes profiles/r07/phi4_ens_hmc/bench.json.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r07", "phi4_ens_hmc", "bench.json")
# shape, replicas, the first guess of dtau (dH's variance grows with V dtau^2 at a fixed number of steps)
CASES = [((32, 32, 32), 256, 0.002), ((16, 16, 16), 1024, 0.0055), ((8, 8, 8), 4096, 0.016)]
# shape, replicas, MALA's dtau of acceptance 0.75 (README), the first guess of the trajectories' dtau
TAU_CASES = [((16, 16, 16), 256, 0.008, 0.004), ((32, 32, 32), 256, 0.004, 0.0015)]
PARAMS = dict(m2=0.5, lam=1.0, C=1.0)
THERMALISE = 1000
ALLOWANCE = 1.15
FRAMES = 50
NLEAP = 10
TARGET = 0.75
CHUNK = 1000


def _timed(fn):
    t0 = time.perf_counter()
    fn()          # every call ends in a stream synchronise
    return (time.perf_counter() - t0) * 1e3


def _spread(acc):
    """The standard deviation s of a Gaussian dH of mean s^2 / 2 whose acceptance erfc(s / (2 sqrt 2)) is acc."""
    lo, hi = 0.0, 20.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if math.erfc(mid / (2.0 * math.sqrt(2.0))) > acc else (lo, mid)
    return 0.5 * (lo + hi)


def _tune(e, dtau, nleap_of, randomize, pilots=4, ntraj=200):
    """dtau at which step_hmc(nleap_of(dtau), randomize) accepts TARGET of its trajectories; the pilots' trace."""
    trace, pts = [], []
    for _ in range(pilots):
        e.set_params(dtau=dtau)
        e.step_hmc(50, nleap=nleap_of(dtau), randomize=randomize)
        e.hmc_reset()
        e.step_hmc(ntraj, nleap=nleap_of(dtau), randomize=randomize)
        st = e.hmc_stats()
        acc = float(st[:, 1].sum()) / float(st[:, 0].sum())
        trace.append([round(dtau, 6), nleap_of(dtau), round(acc, 4)])
        pts.append((dtau, _spread(min(max(acc, 0.02), 0.98))))
        power = 1.0
        if len(pts) > 1 and pts[-1][0] != pts[-2][0]:      # the measured exponent of the spread in dtau
            power = math.log(pts[-1][1] / pts[-2][1]) / math.log(pts[-1][0] / pts[-2][0])
            power = min(max(power, 1.0), 3.0) if math.isfinite(power) else 1.0
        dtau = float(f"{dtau * (_spread(TARGET) / pts[-1][1]) ** (1.0 / power):.3g}")
    e.set_params(dtau=dtau)
    return dtau, trace


def worker(steps, reps):
    from stochquant_amd import Phi4Ensemble, _lib
    for shape, R, guess in CASES:
        with Phi4Ensemble(shape, R, seed=7, dtau=guess, **PARAMS) as e:
            e.init_field(0.5)
            e.step(THERMALISE)
            dtau, trace = _tune(e, guess, lambda d: NLEAP, False)
            with Phi4Ensemble(shape, R, seed=7, dtau=dtau, m2=PARAMS["m2"], lam=PARAMS["lam"], C=0.0) as z:
                z.init_field(0.5)
                calls = {"hmc1": lambda: e.step_hmc(steps, nleap=1),
                         "hmc10": lambda: e.step_hmc(steps, nleap=NLEAP),
                         "hmc10r": lambda: e.step_hmc(steps, nleap=NLEAP, randomize=True),
                         "mala": lambda: e.step(steps, scheme="mala"),
                         "c0": lambda: z.step(steps)}
                ts = {k: [] for k in calls}
                acc = {}
                for rnd in range(reps + 1):
                    for k, fn in calls.items():
                        if k.startswith("hmc"):
                            e.hmc_reset()
                        t = _timed(fn)
                        if rnd:
                            ts[k].append(t)
                        if k.startswith("hmc"):
                            st = e.hmc_stats()
                            acc.setdefault(k, []).append([int(st[:, 0].sum()), int(st[:, 1].sum()), int(st[:, 2].sum()),
                                                          int(st[:, 3].sum())])
                flagged = int(e.flags().sum())
                info = Phi4Ensemble.shape_info(shape)
        med = {k: statistics.median(v) for k, v in ts.items()}
        us = {k: v / steps * 1e3 for k, v in med.items()}          # per trajectory / step
        composed = us["mala"] + (NLEAP - 1) * us["c0"]
        tot = {k: [sum(c) for c in zip(*v[1:])] for k, v in acc.items()}   # the timed rounds
        rec = {"kind": "ensemble", "shape": list(shape), "R": R, "dtau": dtau, "dtau_pilots": trace, "steps": steps,
               "nleap": NLEAP, "K": info["K"], "T": info["T"], "images": info["images"],
               "ms": {k: round(v, 4) for k, v in med.items()},
               "ms_all": {k: [round(t, 4) for t in v] for k, v in ts.items()},
               "trajectory_us": {k: round(v, 3) for k, v in us.items()},
               "acceptance": {k: round(v[1] / v[0], 4) for k, v in tot.items()},
               "guard_trips": {k: v[2] for k, v in tot.items()},
               "mean_length": {k: round(v[3] / v[0], 3) for k, v in tot.items()},
               "leapfrog_steps_per_second": {k: round(tot[k][3] / (sum(ts[k]) * 1e-3), 1) for k in tot},
               "leapfrog_site_updates_per_second": {k: round(tot[k][3] * shape[0] * shape[1] * shape[2]
                                                             / (sum(ts[k]) * 1e-3), 1) for k in tot},
               "composed_us": round(composed, 3),
               "interior_step_us": round((us["hmc10"] - us["hmc1"]) / (NLEAP - 1), 3),
               "hmc10_over_composed": round(us["hmc10"] / composed, 4),
               "hmc1_over_mala": round(us["hmc1"] / us["mala"], 4),
               "allowance": ALLOWANCE,
               "yardstick_hmc10_met": bool(us["hmc10"] <= ALLOWANCE * composed),
               "yardstick_hmc1_met": bool(us["hmc1"] <= ALLOWANCE * us["mala"]),
               "guard_flags_set": flagged, "build_id": _lib.build_id()}
        print(json.dumps(rec), flush=True)


def tau_int(x):
    """(tau_int, window, rho(1)) of the series x[N][R]: rho averaged over the R replicas about the grand mean,
    tau = 1/2 + sum_{t<=W} rho(t), W the smallest window >= 20 tau."""
    import numpy as np
    n = x.shape[0]
    mean = x.mean()
    c = np.zeros(n)
    for r0 in range(0, x.shape[1], 32):      # a block of replicas at a time: the transforms are the memory
        f = np.fft.rfft(x[:, r0:r0 + 32] - mean, n=2 * n, axis=0)
        c += np.fft.irfft(f * np.conj(f), n=2 * n, axis=0)[:n].sum(axis=1)
    c /= np.arange(n, 0, -1) * x.shape[1]
    rho = c / c[0]
    tau = 0.5 + np.cumsum(rho[1:])
    for w in range(1, n - 1):
        if w >= 20.0 * tau[w - 1]:
            return float(tau[w - 1]), w, float(rho[1])
    return float(tau[-1]), n - 1, float(rho[1])


def _series(e, n, call):
    """Σφ² and |Σφ| after each of n updates, (n, R) each, taken in calls of CHUNK."""
    import numpy as np
    s2, m = [], []
    t = 0.0
    for _ in range(n // CHUNK):
        t0 = time.perf_counter()
        ser = call(CHUNK)
        t += time.perf_counter() - t0
        s2.append(ser[:, :, 1].copy())
        m.append(np.abs(ser[:, :, 0]))
    return np.concatenate(s2), np.concatenate(m), t


def tau_worker(n_mala, n_hmc):
    from stochquant_amd import Phi4Ensemble, _lib
    for shape, R, dt_mala, guess in TAU_CASES:
        out = {"kind": "autocorrelation", "shape": list(shape), "R": R, "build_id": _lib.build_id()}
        with Phi4Ensemble(shape, R, seed=11, dtau=dt_mala, **PARAMS) as e:
            e.init_field(0.5)
            e.step(THERMALISE)
            e.step(2000, scheme="mala")
            e.mala_reset()
            t0 = time.perf_counter()
            e.step(CHUNK, scheme="mala")
            plain = (time.perf_counter() - t0) / CHUNK
            s2, m, t = _series(e, n_mala, lambda k: e.step(k, every=1, scheme="mala"))
            st = e.mala_stats()
            a, b = tau_int(s2), tau_int(m)
            out["mala"] = {"dtau": dt_mala, "updates": n_mala, "acceptance": round(float(st[:, 1].sum() / st[:, 0].sum()), 4),
                           "update_us": round(plain * 1e6, 3), "update_us_with_series": round(t / n_mala * 1e6, 3),
                           "tau_int_S2": round(a[0], 2), "window_S2": a[1], "tau_int_absM": round(b[0], 2),
                           "window_absM": b[1], "series_over_window": round(n_mala / max(a[1], b[1]), 1),
                           "cost_S2_us": round(a[0] * plain * 1e6, 1), "cost_absM_us": round(b[0] * plain * 1e6, 1)}
        nleap_of = lambda d: max(1, int(round(2.0 / math.sqrt(2.0 * d))) - 1)      # noqa: E731
        with Phi4Ensemble(shape, R, seed=11, dtau=guess, **PARAMS) as e:
            e.init_field(0.5)
            e.step(THERMALISE)
            dtau, trace = _tune(e, guess, nleap_of, True)
            nleap = nleap_of(dtau)
            e.step_hmc(200, nleap=nleap, randomize=True)
            e.hmc_reset()
            t0 = time.perf_counter()
            e.step_hmc(CHUNK, nleap=nleap, randomize=True)
            plain = (time.perf_counter() - t0) / CHUNK
            s2, m, t = _series(e, n_hmc, lambda k: e.step_hmc(k, nleap=nleap, randomize=True, every=1))
            st = e.hmc_stats()
            a, b = tau_int(s2), tau_int(m)
            out["hmc"] = {"dtau": dtau, "dtau_pilots": trace, "nleap": nleap, "randomize": True, "updates": n_hmc,
                          "mean_length_sigma": round(0.5 * (nleap + 1) * math.sqrt(2.0 * dtau), 4),
                          "acceptance": round(float(st[:, 1].sum() / st[:, 0].sum()), 4),
                          "update_us": round(plain * 1e6, 3), "update_us_with_series": round(t / n_hmc * 1e6, 3),
                          "tau_int_S2": round(a[0], 2), "window_S2": a[1], "tau_int_absM": round(b[0], 2),
                          "window_absM": b[1], "series_over_window": round(n_hmc / max(a[1], b[1]), 1),
                          "cost_S2_us": round(a[0] * plain * 1e6, 1), "cost_absM_us": round(b[0] * plain * 1e6, 1)}
        out["mala_over_hmc_cost_S2"] = round(out["mala"]["cost_S2_us"] / out["hmc"]["cost_S2_us"], 2)
        out["mala_over_hmc_cost_absM"] = round(out["mala"]["cost_absM_us"] / out["hmc"]["cost_absM_us"], 2)
        print(json.dumps(out), flush=True)


def raw_worker(steps, reps):
    import ctypes
    from stochquant_amd import Phi4Ensemble, _lib
    # an older build lacks the newer exports, and these calls need none of them
    have = ctypes.CDLL(os.environ.get("SQ_LIB", _lib.LIB_PATH))
    for name in [n for n in _lib.SIGNATURES if not hasattr(have, n)]:
        del _lib.SIGNATURES[name]
    kw = dict(seed=7, dtau=0.004, **PARAMS)
    with Phi4Ensemble((32, 32, 32), 256, **kw) as ens:
        ens.init_field(0.5)
        ens.step(THERMALISE)
        ens.step(steps, scheme="heun")
        ens.step(steps, scheme="mala")
        euler = statistics.median(_timed(lambda: ens.step(steps)) for _ in range(reps))
        heun = statistics.median(_timed(lambda: ens.step(steps, scheme="heun")) for _ in range(reps))
        mala = statistics.median(_timed(lambda: ens.step(steps, scheme="mala")) for _ in range(reps))
    with Phi4Ensemble((32, 32, 32), 256, **kw) as ens:
        ens.init_field(0.5)
        ens.run_frames(FRAMES)
        frames = statistics.median(_timed(lambda: ens.run_frames(FRAMES)) for _ in range(reps))
    print(json.dumps({"euler_ms": round(euler, 4), "heun_ms": round(heun, 4), "mala_ms": round(mala, 4),
                      "frames_ms": round(frames, 4), "build_id": _lib.build_id()}), flush=True)


def _child(args, timeout, env=None):
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        print(f"bench_phi4_ens_hmc: a child failed with status {r.returncode}; stopping", file=sys.stderr)
        return None
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--parent-lib", default=None, help="another build of libstochquant.so for the A/B of existing calls")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--no-tau", action="store_true", help="skip the autocorrelation measurement")
    ap.add_argument("--tau-mala", type=int, default=80000, help="MALA steps of the autocorrelation series")
    ap.add_argument("--tau-hmc", type=int, default=4000, help="trajectories of the autocorrelation series")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tau-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--raw-worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.steps, a.reps)
        return 0
    if a.tau_worker:
        tau_worker(a.tau_mala, a.tau_hmc)
        return 0
    if a.raw_worker:
        raw_worker(a.steps, a.reps)
        return 0
    common = ["--steps", str(a.steps), "--reps", str(a.reps)]
    records = _child(common + ["--worker"], a.timeout)
    if records is None:
        return 1
    for r in records:
        print(json.dumps(r))
    if not a.no_tau:
        more = _child(["--tau-worker", "--tau-mala", str(a.tau_mala), "--tau-hmc", str(a.tau_hmc)], a.timeout)
        if more is None:
            return 1
        for r in more:
            print(json.dumps(r))
        records += more
    if a.parent_lib:
        penv = dict(os.environ, SQ_LIB=os.path.abspath(a.parent_lib))
        pairs = []
        for _ in range(a.pairs):   # parent, parent again, this build: two differences per round
            runs = [_child(common + ["--raw-worker"], a.timeout, penv)]
            runs.append(_child(common + ["--raw-worker"], a.timeout, penv) if runs[0] is not None else None)
            runs.append(_child(common + ["--raw-worker"], a.timeout) if runs[1] is not None else None)
            if runs[2] is None:
                return 1
            old, old2, new = (r[0] for r in runs)
            pairs.append({"parent": old, "parent_again": old2, "this": new})
        ab = {"kind": "existing_calls_vs_parent", "shape": [32, 32, 32], "R": 256, "steps": a.steps, "nframes": FRAMES,
              "pairs": pairs, "parent_build_id": pairs[0]["parent"]["build_id"],
              "this_build_id": pairs[0]["this"]["build_id"]}
        for k in ("euler_ms", "heun_ms", "mala_ms", "frames_ms"):
            d = [(p["this"][k] / p["parent"][k] - 1.0) * 100.0 for p in pairs]
            s = [(p["parent_again"][k] / p["parent"][k] - 1.0) * 100.0 for p in pairs]
            ab[k[:-3]] = {"parent_median_ms": round(statistics.median(p["parent"][k] for p in pairs), 4),
                          "this_median_ms": round(statistics.median(p["this"][k] for p in pairs), 4),
                          "median_diff_percent": round(statistics.median(d), 3),
                          "min_diff_percent": round(min(d), 3), "max_diff_percent": round(max(d), 3),
                          "parent_self_median_diff_percent": round(statistics.median(s), 3),
                          "parent_self_min_diff_percent": round(min(s), 3),
                          "parent_self_max_diff_percent": round(max(s), 3),
                          "within_parent_spread": bool(statistics.median(d) <= max(abs(x) for x in s))}
        print(json.dumps(ab))
        records.append(ab)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"steps_per_call": a.steps, "reps": a.reps, "params": PARAMS, "thermalise": THERMALISE,
                   "records": records}, fh, indent=1)
        fh.write("\n")
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
