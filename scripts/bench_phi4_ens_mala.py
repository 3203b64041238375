"""Cost and acceptance of the φ⁴ ensemble's Metropolis-adjusted Langevin step
(Phi4Ensemble.step(scheme="mala")), GPU only.

    python scripts/bench_phi4_ens_mala.py [--steps 200] [--reps 5] [--out FILE]
                                          [--parent-lib OTHER/libstochquant.so] [--pairs 5]

One child process under `timeout` (this process never opens the GPU) times, at
32³ R = 256, 16³ R = 1024 and 8³ R = 4096, from fields thermalised by 1000
Euler steps at the shape's Δτ (chosen for an acceptance of 0.6 - 0.8), these
calls, interleaved round by round (`reps` rounds after a warm-up round,
medians per call), on one ensemble:

  mala        step(steps, scheme="mala")
  heun        step(steps, scheme="heun")
  heun_sums1  step(steps, every=1, scheme="heun")     the yardstick
  euler       step(steps)

and reports per shape the acceptance of the timed MALA calls and the yardstick
mala <= 1.15 x heun_sums1 of the same process, met or missed: that call does
the same two stencil passes plus one action evaluation per step; beyond it a
MALA step evaluates the drift twice in double and takes a decision (one fold,
one more barrier), and it drops Heun's second noise application.

--parent-lib: the existing calls must not move.  step(steps), step(steps,
scheme="heun") and run_frames(50) at 32³ R = 256 with this build and with
another build of the library (SQ_LIB), in interleaved rounds of child
processes, the other build first and then twice in a row as well: the spread
of the other build against itself is the allowance.
Writes profiles/r07/phi4_ens_mala/bench.json.
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
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r07", "phi4_ens_mala", "bench.json")
# shape, replicas, dtau: the acceptance falls with the volume at fixed dtau, so dtau ~ V^(-1/3)
CASES = [((32, 32, 32), 256, 0.004), ((16, 16, 16), 1024, 0.008), ((8, 8, 8), 4096, 0.016)]
PARAMS = dict(m2=0.5, lam=1.0, C=1.0)
THERMALISE = 1000
ALLOWANCE = 1.15
FRAMES = 50


def _timed(fn):
    t0 = time.perf_counter()
    fn()          # every call ends in a stream synchronise
    return (time.perf_counter() - t0) * 1e3


def worker(steps, reps):
    from stochquant_amd import Phi4Ensemble, _lib
    for shape, R, dtau in CASES:
        with Phi4Ensemble(shape, R, seed=7, dtau=dtau, **PARAMS) as e:
            e.init_field(0.5)
            e.step(THERMALISE)
            calls = {"mala": lambda: e.step(steps, scheme="mala"),
                     "heun": lambda: e.step(steps, scheme="heun"),
                     "heun_sums1": lambda: e.step(steps, every=1, scheme="heun"),
                     "euler": lambda: e.step(steps)}
            ts = {k: [] for k in calls}
            for rnd in range(reps + 1):
                if rnd == 1:
                    e.mala_reset()
                for k, fn in calls.items():
                    t = _timed(fn)
                    if rnd:
                        ts[k].append(t)
            st = e.mala_stats()
            flagged = int(e.flags().sum())
            info = Phi4Ensemble.shape_info(shape)
        assert int(st[:, 0].sum()) == reps * steps * R
        per = st[:, 1] / st[:, 0]
        med = {k: statistics.median(v) for k, v in ts.items()}
        ratio = med["mala"] / med["heun_sums1"]
        rec = {"kind": "ensemble", "shape": list(shape), "R": R, "dtau": dtau, "steps": steps,
               "K": info["K"], "T": info["T"], "images": info["images"],
               "ms": {k: round(v, 4) for k, v in med.items()},
               "ms_all": {k: [round(t, 4) for t in v] for k, v in ts.items()},
               "step_us": {k: round(v / steps * 1e3, 3) for k, v in med.items()},
               "acceptance": round(float(st[:, 1].sum()) / float(st[:, 0].sum()), 4),
               "acceptance_min_replica": round(float(per.min()), 4),
               "acceptance_max_replica": round(float(per.max()), 4),
               "guard_trips": int(st[:, 2].sum()),
               "mala_over_heun_sums1": round(ratio, 4),
               "mala_over_heun": round(med["mala"] / med["heun"], 4),
               "mala_over_euler": round(med["mala"] / med["euler"], 4),
               "allowance": ALLOWANCE, "yardstick_met": bool(ratio <= ALLOWANCE),
               "guard_flags_set": flagged, "build_id": _lib.build_id()}
        print(json.dumps(rec), flush=True)


def raw_worker(steps, reps):
    import ctypes
    from stochquant_amd import Phi4Ensemble, _lib
    # an older build lacks the newer exports, and these calls need none of them
    have = ctypes.CDLL(os.environ.get("SQ_LIB", _lib.LIB_PATH))
    for name in [n for n in _lib.SIGNATURES if not hasattr(have, n)]:
        del _lib.SIGNATURES[name]
    kw = dict(seed=7, dtau=0.01, **PARAMS)
    with Phi4Ensemble((32, 32, 32), 256, **kw) as ens:
        ens.init_field(0.5)
        ens.step(steps)
        ens.step(steps, scheme="heun")
        euler = statistics.median(_timed(lambda: ens.step(steps)) for _ in range(reps))
        heun = statistics.median(_timed(lambda: ens.step(steps, scheme="heun")) for _ in range(reps))
    with Phi4Ensemble((32, 32, 32), 256, **kw) as ens:
        ens.init_field(0.5)
        ens.run_frames(FRAMES)
        frames = statistics.median(_timed(lambda: ens.run_frames(FRAMES)) for _ in range(reps))
    print(json.dumps({"euler_ms": round(euler, 4), "heun_ms": round(heun, 4), "frames_ms": round(frames, 4),
                      "build_id": _lib.build_id()}), flush=True)


def _child(args, timeout, env=None):
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        print(f"bench_phi4_ens_mala: a child failed with status {r.returncode}; stopping", file=sys.stderr)
        return None
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--parent-lib", default=None, help="another build of libstochquant.so for the A/B of existing calls")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--raw-worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.steps, a.reps)
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
        for k in ("euler_ms", "heun_ms", "frames_ms"):
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
