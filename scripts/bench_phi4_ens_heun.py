"""Cost of the φ⁴ ensemble's second-order (Heun) step
(Phi4Ensemble.step(scheme="heun")), GPU only.

    python scripts/bench_phi4_ens_heun.py [--steps 200] [--every 20] [--reps 5] [--out FILE]
                                          [--parent-lib OTHER/libstochquant.so] [--pairs 5]

One child process under `timeout` (this process never opens the GPU) times, at
32³ R = 256, 16³ R = 1024 and 8³ R = 4096, these calls, interleaved round by
round (`reps` rounds after a warm-up round, medians per call), on one ensemble:

  euler       step(steps)
  euler2      step(2 steps)                              the same number of site updates as heun
  heun        step(steps, scheme="heun")
  heun_sums   step(steps, every=every, scheme="heun")    the four-sums measurement
  heun_corr   step(steps, every=every, correlate=True, scheme="heun")
  euler_sums, euler_corr                                 the last two with the Euler step

and reports per shape the yardstick heun <= 1.10 x euler2 of the same process: a
Heun step is two Euler updates plus, per quad, one 16-byte LDS read, an add, a
multiply and the guard per site, and on one-image shapes the exchange of the
lane's own quads and two more barriers.

--parent-lib: raw Euler steps must not move.  step(steps) at 32³ R = 256 with
this build and with another build of the library (SQ_LIB), in interleaved
rounds of child processes, the other build first and then twice in a row as
well: the spread of the other build against itself is the allowance.
Writes profiles/r07/phi4_ens_heun/bench.json.
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
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r07", "phi4_ens_heun", "bench.json")
CASES = [((32, 32, 32), 256), ((16, 16, 16), 1024), ((8, 8, 8), 4096)]
PARAMS = dict(dtau=0.01, m2=0.5, lam=1.0, C=1.0)
ALLOWANCE = 1.10


def _timed(fn):
    t0 = time.perf_counter()
    fn()          # every step call ends in a stream synchronise
    return (time.perf_counter() - t0) * 1e3


def worker(steps, every, reps):
    from stochquant_amd import Phi4Ensemble, _lib
    nmeas = steps // every
    for shape, R in CASES:
        with Phi4Ensemble(shape, R, seed=7, **PARAMS) as e:
            e.init_field(0.5)
            calls = {"euler": lambda: e.step(steps),
                     "euler2": lambda: e.step(2 * steps),
                     "heun": lambda: e.step(steps, scheme="heun"),
                     "heun_sums": lambda: e.step(steps, every=every, scheme="heun"),
                     "heun_corr": lambda: e.step(steps, every=every, correlate=True, scheme="heun"),
                     "euler_sums": lambda: e.step(steps, every=every),
                     "euler_corr": lambda: e.step(steps, every=every, correlate=True)}
            ts = {k: [] for k in calls}
            for rnd in range(reps + 1):
                for k, fn in calls.items():
                    t = _timed(fn)
                    if rnd:
                        ts[k].append(t)
            flagged = int(e.flags().sum())
            assert int(e.corr_sums(count=1)[2][0]) == 2 * (reps + 1) * nmeas
            info = Phi4Ensemble.shape_info(shape)
        med = {k: statistics.median(v) for k, v in ts.items()}
        ratio = med["heun"] / med["euler2"]
        rec = {"kind": "ensemble", "shape": list(shape), "R": R, "steps": steps, "every": every,
               "K": info["K"], "T": info["T"], "images": info["images"],
               "ms": {k: round(v, 4) for k, v in med.items()},
               "ms_all": {k: [round(t, 4) for t in v] for k, v in ts.items()},
               "euler_step_us": round(med["euler"] / steps * 1e3, 3),
               "euler2_step_us": round(med["euler2"] / (2 * steps) * 1e3, 3),
               "heun_step_us": round(med["heun"] / steps * 1e3, 3),
               "heun_over_euler2": round(ratio, 4),
               "heun_over_euler": round(med["heun"] / med["euler"], 4),
               "allowance": ALLOWANCE, "yardstick_met": bool(ratio <= ALLOWANCE),
               "heun_sums_measurement_us": round((med["heun_sums"] - med["heun"]) / nmeas * 1e3, 3),
               "heun_corr_measurement_us": round((med["heun_corr"] - med["heun_sums"]) / nmeas * 1e3, 3),
               "euler_sums_measurement_us": round((med["euler_sums"] - med["euler"]) / nmeas * 1e3, 3),
               "euler_corr_measurement_us": round((med["euler_corr"] - med["euler_sums"]) / nmeas * 1e3, 3),
               "guard_flags_set": flagged, "build_id": _lib.build_id()}
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
        print(f"bench_phi4_ens_heun: a child failed with status {r.returncode}; stopping", file=sys.stderr)
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
        penv = dict(os.environ, SQ_LIB=os.path.abspath(a.parent_lib))
        pairs = []
        for _ in range(a.pairs):   # parent, parent again, this build: two differences per round
            runs = [_child(common + ["--raw-worker"], a.timeout, penv)]
            runs.append(_child(common + ["--raw-worker"], a.timeout, penv) if runs[0] is not None else None)
            runs.append(_child(common + ["--raw-worker"], a.timeout) if runs[1] is not None else None)
            if runs[2] is None:
                return 1
            old, old2, new = (r[0] for r in runs)
            pairs.append({"parent_ms": old["ms"], "parent_again_ms": old2["ms"], "this_ms": new["ms"],
                          "diff_percent": round((new["ms"] / old["ms"] - 1.0) * 100.0, 3),
                          "parent_self_diff_percent": round((old2["ms"] / old["ms"] - 1.0) * 100.0, 3)})
        d = [p["diff_percent"] for p in pairs]
        s = [p["parent_self_diff_percent"] for p in pairs]
        ab = {"kind": "raw_steps_vs_parent", "shape": [32, 32, 32], "R": 256, "steps": a.steps, "pairs": pairs,
              "median_diff_percent": round(statistics.median(d), 3), "min_diff_percent": min(d),
              "max_diff_percent": max(d), "parent_self_median_diff_percent": round(statistics.median(s), 3),
              "parent_self_min_diff_percent": min(s), "parent_self_max_diff_percent": max(s),
              "within_parent_spread": bool(statistics.median(d) <= max(abs(x) for x in s)),
              "parent_build_id": old["build_id"], "this_build_id": new["build_id"]}
        print(json.dumps(ab))
        records.append(ab)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"steps_per_call": a.steps, "every": a.every, "reps": a.reps, "params": PARAMS,
                   "records": records}, fh, indent=1)
        fh.write("\n")
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
