"""Cost of the φ⁴ ensemble's gradient-flow measurements inside frames and Heun
steps (Phi4Ensemble.run_frames_flow, step_flow(scheme="heun")), GPU only.

    python scripts/bench_phi4_ens_flow_frames.py [--frames 50] [--loops 20] [--reps 5] [--out FILE]
                                                 [--parent-lib OTHER/libstochquant.so] [--rounds 5]

One child process under `timeout` (this process never opens the GPU) times, at
32³ R = 256, 16³ R = 1024 and 8³ R = 4096, with levels (0, 5, 20), these calls,
interleaved round by round (`reps` rounds after a warm-up round, medians):

  frames[s]      run_frames(frames, scheme=s)                       the simulation alone
  flow[s]        run_frames_flow(frames, scheme=s)                  one flow measurement per frame
  flow_corr[s]   run_frames_flow(frames, correlate=True, scheme=s)
  plain / sums / corr / zero                                        the yardstick's parts, as bench_phi4_ens_flow.py
  step[s], step_flow[s]   step(frames loops) and step_flow(..., every=loops) per scheme

One in-frame flow measurement costs (flow[s] − frames[s]) / frames.  The
yardstick is the flow pull request's own, made of existing kernels timed in the
same process: n_F steps of a C = 0 ensemble + F sums measurements (with
`correlate`: F measurements of the correlator call), times 1.15.  The host
route the call replaces, run_frames(1) + flowed() per frame, is timed beside it.
Δτ is held (adapt_dtau off) and small enough that every frame is stable, so
every frame of every call does the same work.

--parent-lib: the existing kernels must not move.  Euler and Heun step(200),
Euler and Heun run_frames(50) and the Euler step_flow at 32³ R = 256 with this
build and with another build of the library (SQ_LIB), `rounds` interleaved
rounds of child processes parent, this, parent.
Writes profiles/r07/phi4_ens_flow_frames/bench.json.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r07", "phi4_ens_flow_frames", "bench.json")
CASES = [((32, 32, 32), 256), ((16, 16, 16), 1024), ((8, 8, 8), 4096)]
PARAMS = dict(dtau=0.01, m2=0.5, lam=1.0, C=1.0)
EPS = 0.01
LEVELS = (0, 5, 20)
SCHEMES = ("euler", "heun")


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def worker(frames, loops, reps):
    from stochquant_amd import Phi4Ensemble, _lib
    steps = frames * loops
    F, nF = len(LEVELS), LEVELS[-1]
    kw = dict(seed=7, loops=loops, adapt_dtau=False, **PARAMS)
    for shape, R in CASES:
        zp = dict(kw, dtau=EPS, C=0.0)
        with Phi4Ensemble(shape, R, **kw) as ens, Phi4Ensemble(shape, R, **zp) as zero, \
                Phi4Ensemble(shape, R, **kw) as fl:
            for e in (ens, zero, fl):
                e.init_field(0.5)
            fl.set_flow(EPS, LEVELS)
            calls = {"plain": lambda: ens.step(steps), "sums": lambda: ens.step(steps, every=loops),
                     "corr": lambda: ens.step(steps, every=loops, correlate=True), "zero": lambda: zero.step(steps)}
            for s in SCHEMES:
                calls[("frames", s)] = (lambda s=s: ens.run_frames(frames, scheme=s))
                calls[("flow", s)] = (lambda s=s: fl.run_frames_flow(frames, scheme=s))
                calls[("flow_corr", s)] = (lambda s=s: fl.run_frames_flow(frames, correlate=True, scheme=s))
                calls[("step", s)] = (lambda s=s: ens.step(steps, scheme=s))
                calls[("step_flow", s)] = (lambda s=s: fl.step_flow(steps, loops, scheme=s))
            ts = {k: [] for k in calls}
            stable = True
            for rnd in range(reps + 1):
                for k, fn in calls.items():
                    t0 = time.perf_counter()
                    out = fn()
                    t = (time.perf_counter() - t0) * 1e3
                    if rnd:
                        ts[k].append(t)
                    if isinstance(k, tuple) and k[0] in ("frames", "flow", "flow_corr"):
                        stable = stable and bool(out[0].all())
            if stable:   # one correlator measurement per stable frame of the flow_corr calls, none elsewhere
                assert int(fl.fcorr_sums()[2][0]) == (reps + 1) * frames * len(SCHEMES)
            med = {k: statistics.median(v) for k, v in ts.items()}
            zero_us = med["zero"] / steps * 1e3
            sums_us = (med["sums"] - med["plain"]) / frames * 1e3
            corr_us = (med["corr"] - med["plain"]) / frames * 1e3
            sf = {s: (med[("step_flow", s)] - med[("step", s)]) / frames * 1e3 for s in SCHEMES}
            for s in SCHEMES:
                for co in (False, True):
                    t, base = med[("flow_corr" if co else "flow", s)], med[("frames", s)]
                    cost = (t - base) / frames * 1e3
                    yard = nF * zero_us + F * (corr_us if co else sums_us)

                    def host():
                        for _ in range(frames):
                            fl.run_frames(1, scheme=s)
                            fl.flowed()
                    host()
                    host_ms = statistics.median(_timed(host) for _ in range(3))
                    rec = {"kind": "ensemble", "shape": list(shape), "R": R, "frames": frames, "loops": loops,
                           "levels": list(LEVELS), "eps": EPS, "scheme": s, "correlate": co,
                           "every_frame_stable": stable, "frames_ms": round(base, 4), "frames_flow_ms": round(t, 4),
                           "frames_flow_ms_all": [round(x, 4) for x in ts[("flow_corr" if co else "flow", s)]],
                           "frames_ms_all": [round(x, 4) for x in ts[("frames", s)]],
                           "flow_measurement_us": round(cost, 3), "flow_step_us": round(zero_us, 3),
                           "sums_measurement_us": round(sums_us, 3), "corr_call_measurement_us": round(corr_us, 3),
                           "yardstick_us": round(yard, 3), "flow_over_yardstick": round(cost / yard, 3),
                           "yardstick_met": bool(cost <= 1.15 * yard),
                           "host_route_ms": round(host_ms, 3), "speedup_over_host_route": round(host_ms / t, 2),
                           "step_flow_measurement_us": round(sf[s], 3),
                           "heun_over_euler_step_flow_measurement": round(sf["heun"] / sf["euler"], 3),
                           "guard_flags_set": int(ens.flags().sum() + fl.flags().sum()), "build_id": _lib.build_id()}
                    print(json.dumps(rec), flush=True)


def gate_worker(reps):
    import ctypes
    from stochquant_amd import Phi4Ensemble, _lib
    # an older build lacks the newer exports, and the existing calls need none of them
    have = ctypes.CDLL(os.environ.get("SQ_LIB", _lib.LIB_PATH))
    for name in [n for n in _lib.SIGNATURES if not hasattr(have, n)]:
        del _lib.SIGNATURES[name]
    with Phi4Ensemble((32, 32, 32), 256, seed=7, loops=20, adapt_dtau=False, **PARAMS) as ens:
        ens.init_field(0.5)
        ens.set_flow(EPS, LEVELS)
        calls = {"raw_ms": lambda: ens.step(200), "heun_ms": lambda: ens.step(200, scheme="heun"),
                 "frames_ms": lambda: ens.run_frames(50), "heun_frames_ms": lambda: ens.run_frames(50, scheme="heun"),
                 "step_flow_ms": lambda: ens.step_flow(200, 20)}
        ts = {k: [] for k in calls}
        for rnd in range(reps + 1):
            for k, fn in calls.items():
                t = _timed(fn)
                if rnd:
                    ts[k].append(t)
    rec = {k: round(statistics.median(v), 4) for k, v in ts.items()}
    rec["build_id"] = _lib.build_id()
    print(json.dumps(rec), flush=True)


def _child(args, timeout, env=None):
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        print(f"bench_phi4_ens_flow_frames: a child failed with status {r.returncode}; stopping", file=sys.stderr)
        return None
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--loops", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--parent-lib", default=None, help="another build of libstochquant.so for the gate")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--gate-worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.frames, a.loops, a.reps)
        return 0
    if a.gate_worker:
        gate_worker(a.reps)
        return 0
    common = ["--frames", str(a.frames), "--loops", str(a.loops), "--reps", str(a.reps)]
    records = _child(common + ["--worker"], a.timeout)
    if records is None:
        return 1
    for r in records:
        print(json.dumps(r))
    if a.parent_lib:
        penv = dict(os.environ, SQ_LIB=os.path.abspath(a.parent_lib))
        rounds = []
        for _ in range(a.rounds):
            runs = []
            for env in (penv, None, penv):   # parent, this, parent: stop at the first child that fails
                got = _child(common + ["--gate-worker"], a.timeout, env)
                if got is None:
                    return 1
                runs.append(got[0])
            rounds.append({"parent": runs[0], "this": runs[1], "parent_again": runs[2]})
        gate = {"kind": "existing_kernels_vs_parent", "shape": [32, 32, 32], "R": 256, "steps": 200, "nframes": 50,
                "loops": 20, "rounds": rounds}
        for k in ("raw_ms", "heun_ms", "frames_ms", "heun_frames_ms", "step_flow_ms"):
            this = [(r["this"][k] / r["parent"][k] - 1.0) * 100.0 for r in rounds]
            self_ = [(r["parent_again"][k] / r["parent"][k] - 1.0) * 100.0 for r in rounds]
            spread = max(abs(x) for x in self_)
            gate[k[:-3]] = {"this_vs_parent_percent": [round(x, 3) for x in this],
                            "parent_vs_parent_percent": [round(x, 3) for x in self_],
                            "median_this_vs_parent_percent": round(statistics.median(this), 3),
                            "parent_spread_percent": round(spread, 3),
                            "within_parent_spread": bool(abs(statistics.median(this)) <= spread)}
        print(json.dumps(gate))
        records.append(gate)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"frames": a.frames, "loops": a.loops, "reps": a.reps, "params": PARAMS, "eps": EPS,
                   "levels": list(LEVELS), "records": records}, fh, indent=1)
        fh.write("\n")
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
