"""Cost of the φ⁴ ensemble's in-kernel time-slice correlator
(Phi4Ensemble.step(correlate=True)), GPU only.

    python scripts/bench_phi4_ens_corr.py [--steps 200] [--every 20] [--reps 5] [--out FILE]
                                          [--parent-lib OTHER/libstochquant.so] [--pairs 5]

One child process under `timeout` (this process never opens the GPU) times, at
32³ R = 256, 16³ R = 1024 and 8³ R = 4096, three calls of one ensemble,
interleaved round by round (plain, sums, correlator; `reps` rounds after a
warm-up round, medians per call):

  plain       step(steps)
  sums        step(steps, every=every)                   the existing four-sums measurement
  correlator  step(steps, every=every, correlate=True)   the sums and the correlator

and reports per shape one step, one sums measurement and one correlator
measurement ((correlator - sums) / measurements) in µs, the correlator in units
of a step and of a sums measurement, and whether it stays under the yardstick
"a sums measurement plus one step".  At 32³ R = 256 the same process also runs
the sequential loop the call replaces: one Phi4Lattice doing step(every) then
correlator(), steps / every times, times R.

--parent-lib: raw steps must not move.  step(steps) at 32³ R = 256 with this
build and with another build of the library (SQ_LIB), in interleaved pairs of
child processes; the record holds every pair and the spread.
Writes profiles/r07/phi4_ens_corr/bench.json.
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
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r07", "phi4_ens_corr", "bench.json")
CASES = [((32, 32, 32), 256), ((16, 16, 16), 1024), ((8, 8, 8), 4096)]
PARAMS = dict(dtau=0.01, m2=0.5, lam=1.0, C=1.0)


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def worker(steps, every, reps):
    from stochquant_amd import Phi4Ensemble, Phi4Lattice, _lib
    nmeas = steps // every
    for shape, R in CASES:
        with Phi4Ensemble(shape, R, seed=7, **PARAMS) as ens:
            ens.init_field(0.5)
            calls = {"plain": lambda: ens.step(steps), "sums": lambda: ens.step(steps, every=every),
                     "corr": lambda: ens.step(steps, every=every, correlate=True)}
            ts = {k: [] for k in calls}
            for rnd in range(reps + 1):
                for k, fn in calls.items():
                    t = _timed(fn)
                    if rnd:
                        ts[k].append(t)
            flagged = int(ens.flags().sum())
            assert int(ens.corr_sums()[2][0]) == (reps + 1) * nmeas
        med = {k: statistics.median(v) for k, v in ts.items()}
        step_us = med["plain"] / steps * 1e3
        sums_us = (med["sums"] - med["plain"]) / nmeas * 1e3
        corr_us = (med["corr"] - med["sums"]) / nmeas * 1e3
        rec = {"kind": "ensemble", "shape": list(shape), "R": R, "steps": steps, "every": every,
               "plain_ms": round(med["plain"], 4), "sums_ms": round(med["sums"], 4), "corr_ms": round(med["corr"], 4),
               "plain_ms_all": [round(t, 4) for t in ts["plain"]], "sums_ms_all": [round(t, 4) for t in ts["sums"]],
               "corr_ms_all": [round(t, 4) for t in ts["corr"]],
               "step_us": round(step_us, 3), "sums_measurement_us": round(sums_us, 3),
               "corr_measurement_us": round(corr_us, 3),
               "corr_measurement_in_steps": round(corr_us / step_us, 3),
               "sums_measurement_in_steps": round(sums_us / step_us, 3),
               "corr_over_sums_measurement": round(corr_us / sums_us, 3) if sums_us > 0 else None,
               "yardstick_sums_plus_one_step_us": round(sums_us + step_us, 3),
               "yardstick_met": bool(corr_us <= sums_us + step_us),
               "corr_call_over_plain_percent": round((med["corr"] / med["plain"] - 1.0) * 100.0, 2),
               "guard_flags_set": flagged, "build_id": _lib.build_id()}
        if shape == (32, 32, 32):
            with Phi4Lattice(shape, seed=7, **PARAMS) as lat:
                lat.init_field(0.5)

                def loop():
                    for _ in range(nmeas):
                        lat.step(every)
                        lat.correlator()
                loop()
                one = statistics.median(_timed(loop) for _ in range(reps))
            rec["single_context_loop_ms"] = round(one, 4)
            rec["sequential_loop_ms"] = round(one * R, 3)
            rec["speedup_over_sequential_loop"] = round(one * R / med["corr"], 2)
        print(json.dumps(rec), flush=True)


def raw_worker(steps, reps):
    import ctypes
    from stochquant_amd import Phi4Ensemble, _lib
    # an older build lacks the newer exports, and the raw step needs none of them
    have = ctypes.CDLL(os.environ.get("SQ_LIB", _lib.LIB_PATH))
    for name in [n for n in _lib.SIGNATURES if not hasattr(have, n)]:
        del _lib.SIGNATURES[name]
    with Phi4Ensemble((32, 32, 32), 256, seed=7, **PARAMS) as ens:
        ens.init_field(0.5)
        ens.step(steps)
        ms = statistics.median(_timed(lambda: ens.step(steps)) for _ in range(reps))
    print(json.dumps({"ms": round(ms, 4), "build_id": _lib.build_id()}), flush=True)


def _child(args, timeout, env=None):
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        print(f"bench_phi4_ens_corr: a child failed with status {r.returncode}; stopping", file=sys.stderr)
        return None
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--every", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--parent-lib", default=None, help="another build of libstochquant.so for the raw-step A/B")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--raw-worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.steps, a.every, a.reps)
        return 0
    if a.raw_worker:
        raw_worker(a.steps, a.reps)
        return 0
    common = ["--steps", str(a.steps), "--every", str(a.every), "--reps", str(a.reps)]
    records = _child(common + ["--worker"], a.timeout)
    if records is None:
        return 1
    for r in records:
        print(json.dumps(r))
    if a.parent_lib:
        pairs = []
        for _ in range(a.pairs):
            old = _child(common + ["--raw-worker"], a.timeout, dict(os.environ, SQ_LIB=os.path.abspath(a.parent_lib)))
            new = _child(common + ["--raw-worker"], a.timeout) if old is not None else None
            if new is None:
                return 1
            pairs.append({"parent_ms": old[0]["ms"], "this_ms": new[0]["ms"],
                          "diff_percent": round((new[0]["ms"] / old[0]["ms"] - 1.0) * 100.0, 3)})
        d = [p["diff_percent"] for p in pairs]
        ab = {"kind": "raw_steps_vs_parent", "shape": [32, 32, 32], "R": 256, "steps": a.steps, "pairs": pairs,
              "median_diff_percent": round(statistics.median(d), 3), "min_diff_percent": min(d),
              "max_diff_percent": max(d), "parent_build_id": old[0]["build_id"], "this_build_id": new[0]["build_id"]}
        print(json.dumps(ab))
        records.append(ab)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"steps_per_call": a.steps, "every": a.every, "reps": a.reps, "params": PARAMS, "records": records},
                  fh, indent=1)
        fh.write("\n")
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
