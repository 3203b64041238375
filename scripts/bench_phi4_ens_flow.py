"""Cost of the φ⁴ ensemble's in-kernel gradient-flow measurements
(Phi4Ensemble.step(flow=True)), GPU only.

    python scripts/bench_phi4_ens_flow.py [--steps 200] [--every 20] [--reps 5] [--out FILE]
                                          [--parent-lib OTHER/libstochquant.so] [--rounds 5]

One child process under `timeout` (this process never opens the GPU) times, at
32³ R = 256, 16³ R = 1024 and 8³ R = 4096, these calls, interleaved round by
round (`reps` rounds after a warm-up round, medians per call):

  plain       step(steps)                                  the simulation alone
  sums        step(steps, every=every)                     the existing four-sums measurement
  corr        step(steps, every=every, correlate=True)     the sums and the correlator
  zero        step(steps) of a C = 0 ensemble, Δτ = ε      the flow's own step, as the existing kernel runs it
  flow        step(steps, every=every, flow=True[, correlate=True]) with levels (0, 5, 20) and with (20,)

One flow measurement costs (flow − plain) / (steps / every).  The yardstick is
made of the existing kernels timed in the same process: n_F × (zero / steps) +
F × (one sums measurement, or one measurement of the correlator call); the flow
adds the stash and restore of the field and two barriers to that work, so the
record says whether the measurement stays within 1.15 × that sum.  The host
route the call replaces -- step(every), download, upload into the C = 0
ensemble, step to each level, moments (and slices) -- is timed once per
configuration as a figure.  The split of a flow measurement comes from two
more calls without the correlator: levels (0,) against `sums` is the stash and
restore alone, levels (40,) against (20,) is twenty flow steps inside the kernel.

--parent-lib: the existing kernels must not move.  step(steps), Heun
step(steps) and run_frames(50) at 32³ R = 256 with this build and with another
build of the library (SQ_LIB), `rounds` interleaved rounds of child processes
parent, this, parent: the record holds every round, this build against the
parent and the parent against itself.
Writes profiles/r07/phi4_ens_flow/bench.json.
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
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r07", "phi4_ens_flow", "bench.json")
CASES = [((32, 32, 32), 256), ((16, 16, 16), 1024), ((8, 8, 8), 4096)]
PARAMS = dict(dtau=0.01, m2=0.5, lam=1.0, C=1.0)
EPS = 0.01
LEVEL_SETS = [(0, 5, 20), (20,)]
SPLIT_SETS = [(0,), (40,)]   # the stash and restore alone; twenty more flow steps than (20,)


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def worker(steps, every, reps):
    from stochquant_amd import Phi4Ensemble, _lib
    nmeas = steps // every
    for shape, R in CASES:
        zp = dict(PARAMS, dtau=EPS, C=0.0)
        with Phi4Ensemble(shape, R, seed=7, **PARAMS) as ens, Phi4Ensemble(shape, R, seed=7, **zp) as zero, \
                Phi4Ensemble(shape, R, seed=7, **PARAMS) as f0, Phi4Ensemble(shape, R, seed=7, **PARAMS) as f1, \
                Phi4Ensemble(shape, R, seed=7, **PARAMS) as s0, Phi4Ensemble(shape, R, seed=7, **PARAMS) as s1:
            flows = dict(zip(LEVEL_SETS, (f0, f1)))
            splits = dict(zip(SPLIT_SETS, (s0, s1)))
            for e in (ens, zero, f0, f1, s0, s1):
                e.init_field(0.5)
            for lv, e in list(flows.items()) + list(splits.items()):
                e.set_flow(EPS, lv)
            calls = {"plain": lambda: ens.step(steps), "sums": lambda: ens.step(steps, every=every),
                     "corr": lambda: ens.step(steps, every=every, correlate=True), "zero": lambda: zero.step(steps)}
            for lv, e in flows.items():
                for co in (False, True):
                    calls[(lv, co)] = (lambda e=e, co=co: e.step(steps, every=every, flow=True, correlate=co))
            for lv, e in splits.items():
                calls[("split", lv)] = (lambda e=e: e.step(steps, every=every, flow=True))
            ts = {k: [] for k in calls}
            for rnd in range(reps + 1):
                for k, fn in calls.items():
                    t = _timed(fn)
                    if rnd:
                        ts[k].append(t)
            flagged = int(ens.flags().sum() + f0.flags().sum() + f1.flags().sum())
            assert int(f0.fcorr_sums()[2][0]) == (reps + 1) * nmeas
            med = {k: statistics.median(v) for k, v in ts.items()}
            step_us = med["plain"] / steps * 1e3
            zero_us = med["zero"] / steps * 1e3
            sums_us = (med["sums"] - med["plain"]) / nmeas * 1e3
            corr_us = (med["corr"] - med["plain"]) / nmeas * 1e3   # one measurement of the correlator call: sums and g
            base = {"kind": "ensemble", "shape": list(shape), "R": R, "steps": steps, "every": every, "eps": EPS,
                    "plain_ms": round(med["plain"], 4), "sums_ms": round(med["sums"], 4),
                    "corr_ms": round(med["corr"], 4), "zero_ms": round(med["zero"], 4),
                    "step_us": round(step_us, 3), "flow_step_us": round(zero_us, 3),
                    "sums_measurement_us": round(sums_us, 3), "corr_call_measurement_us": round(corr_us, 3),
                    "stash_and_restore_us": round((med[("split", (0,))] - med["sums"]) / nmeas * 1e3, 3),
                    "flow_step_in_kernel_us": round((med[("split", (40,))] - med[(LEVEL_SETS[1], False)])
                                                    / (nmeas * (40 - LEVEL_SETS[1][-1])) * 1e3, 3),
                    "guard_flags_set": flagged, "build_id": _lib.build_id()}
            for lv, e in flows.items():
                for co in (False, True):
                    t = med[(lv, co)]
                    flow_us = (t - med["plain"]) / nmeas * 1e3
                    yard = lv[-1] * zero_us + len(lv) * (corr_us if co else sums_us)
                    # the host route, once: every field over PCIe and back, the C = 0 ensemble stepped level by level
                    def host():
                        for _ in range(nmeas):
                            e.step(every)
                            zero.upload(e.download())
                            done = 0
                            for n in lv:
                                zero.step(n - done)
                                done = n
                                zero.moments()
                                if co:
                                    zero.slices()
                    host()
                    host_ms = statistics.median(_timed(host) for _ in range(3))
                    rec = dict(base, levels=list(lv), correlate=co, flow_ms=round(t, 4),
                               flow_ms_all=[round(x, 4) for x in ts[(lv, co)]],
                               flow_measurement_us=round(flow_us, 3),
                               yardstick_flow_steps_us=round(lv[-1] * zero_us, 3),
                               yardstick_measurements_us=round(len(lv) * (corr_us if co else sums_us), 3),
                               yardstick_us=round(yard, 3), flow_over_yardstick=round(flow_us / yard, 3),
                               yardstick_met=bool(flow_us <= 1.15 * yard),
                               flow_call_over_plain_percent=round((t / med["plain"] - 1.0) * 100.0, 2),
                               host_route_ms=round(host_ms, 3), speedup_over_host_route=round(host_ms / t, 2))
                    print(json.dumps(rec), flush=True)


def gate_worker(steps, reps):
    import ctypes
    from stochquant_amd import Phi4Ensemble, _lib
    # an older build lacks the newer exports, and the existing calls need none of them
    have = ctypes.CDLL(os.environ.get("SQ_LIB", _lib.LIB_PATH))
    for name in [n for n in _lib.SIGNATURES if not hasattr(have, n)]:
        del _lib.SIGNATURES[name]
    with Phi4Ensemble((32, 32, 32), 256, seed=7, loops=20, adapt_dtau=False, **PARAMS) as ens:
        ens.init_field(0.5)
        calls = {"raw_ms": lambda: ens.step(steps), "heun_ms": lambda: ens.step(steps, scheme="heun"),
                 "frames_ms": lambda: ens.run_frames(50)}
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
        print(f"bench_phi4_ens_flow: a child failed with status {r.returncode}; stopping", file=sys.stderr)
        return None
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--every", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--parent-lib", default=None, help="another build of libstochquant.so for the gate")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--gate-worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.steps, a.every, a.reps)
        return 0
    if a.gate_worker:
        gate_worker(a.steps, a.reps)
        return 0
    common = ["--steps", str(a.steps), "--every", str(a.every), "--reps", str(a.reps)]
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
        gate = {"kind": "existing_kernels_vs_parent", "shape": [32, 32, 32], "R": 256, "steps": a.steps,
                "frames": 50, "loops": 20, "rounds": rounds}
        for k, name in (("raw_ms", "raw_step"), ("heun_ms", "heun_step"), ("frames_ms", "run_frames")):
            this = [(r["this"][k] / r["parent"][k] - 1.0) * 100.0 for r in rounds]
            self_ = [(r["parent_again"][k] / r["parent"][k] - 1.0) * 100.0 for r in rounds]
            spread = max(abs(x) for x in self_)
            gate[name] = {"this_vs_parent_percent": [round(x, 3) for x in this],
                            "parent_vs_parent_percent": [round(x, 3) for x in self_],
                            "median_this_vs_parent_percent": round(statistics.median(this), 3),
                            "parent_spread_percent": round(spread, 3),
                            "within_parent_spread": bool(abs(statistics.median(this)) <= spread)}
        print(json.dumps(gate))
        records.append(gate)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"steps_per_call": a.steps, "every": a.every, "reps": a.reps, "params": PARAMS, "eps": EPS,
                   "records": records}, fh, indent=1)
        fh.write("\n")
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
