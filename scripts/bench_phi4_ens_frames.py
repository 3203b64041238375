"""φ⁴ ensemble frames (Phi4Ensemble.run_frames) against the ensemble's raw steps,
the sequential loop of single-context frames they replace, and the single
context's own frame overhead, GPU only.

    python scripts/bench_phi4_ens_frames.py [--frames 50] [--loops 20] [--reps 5] [--out FILE]

Frames of `loops` steps at Δτ = 0.01 (every frame stable), `frames` frames per
call.  One child process under `timeout` (this process never opens the GPU)
times everything, so the ratios compare numbers of one process:

  ensemble frames     run_frames(frames) at 32³ R = 256 / 1024, 16³ R = 1024, 8³ R = 4096
  ensemble raw steps  step(frames * loops) at the same shapes
  sequential loop     one Phi4Lattice of the shape doing run_frames(frames), times R
  single context      run_frames(frames) against step(frames * loops) of a 256³ Phi4Lattice

and one case with rollbacks: Δτ = 0.19 held (adapt_dtau off, so every call
meets the same mix of rejected frames), 32³, R = 256, with the share of stable
frames and of executed steps.  Times are medians of `reps` calls after a
warm-up call, host clock around calls that return with the stream idle.
Writes profiles/r07/phi4_ens_frames/bench.json.
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
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r07", "phi4_ens_frames", "bench.json")
CASES = [((32, 32, 32), 256), ((32, 32, 32), 1024), ((16, 16, 16), 1024), ((8, 8, 8), 4096)]
PARAMS = dict(dtau=0.01, m2=0.5, lam=1.0, C=1.0)


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def worker(frames, loops, reps):
    from stochquant_amd import Phi4Ensemble, Phi4Lattice, _lib
    steps = frames * loops

    def lattice(shape):
        """(frames ms, raw ms) of one Phi4Lattice: run_frames(frames) and step(frames * loops)."""
        with Phi4Lattice(shape, seed=7, loops=loops, **PARAMS) as lat:
            lat.init_field(0.5)

            def raw():
                lat.step(steps)
                lat.sync()
            raw()
            raw_ms = _median_ms(raw, reps)
            ok, _ = lat.run_frames(frames)  # warm-up
            assert ok.all()
            fr_ms = _median_ms(lambda: lat.run_frames(frames), reps)
            return fr_ms, raw_ms

    big_fr, big_raw = lattice((256, 256, 256))
    big_over = big_fr[0] / big_raw[0] - 1.0
    print(json.dumps({"kind": "single_256", "frames": frames, "loops": loops, "frames_ms": round(big_fr[0], 4),
                      "frames_ms_min": round(big_fr[1], 4), "frames_ms_max": round(big_fr[2], 4),
                      "raw_ms": round(big_raw[0], 4), "raw_ms_min": round(big_raw[1], 4),
                      "raw_ms_max": round(big_raw[2], 4), "frame_overhead": round(big_over, 4),
                      "build_id": _lib.build_id()}), flush=True)
    single = {}
    for shape, R in CASES:
        sites = shape[0] * shape[1] * shape[2]
        if shape not in single:
            single[shape] = lattice(shape)
        one_fr, _ = single[shape]
        with Phi4Ensemble(shape, R, seed=7, loops=loops, **PARAMS) as ens:
            ens.init_field(0.5)
            ens.step(steps)  # warm-up
            raw = _median_ms(lambda: ens.step(steps), reps)
            ok, _ = ens.run_frames(frames)  # warm-up
            assert ok.all()
            fr = _median_ms(lambda: ens.run_frames(frames), reps)
            ms = _median_ms(lambda: ens.run_frames(frames, measure=True), reps)
            flagged = int(ens.flags().sum())
        print(json.dumps({"kind": "ensemble", "shape": list(shape), "R": R, "frames": frames, "loops": loops,
                          "frames_ms": round(fr[0], 4), "frames_ms_min": round(fr[1], 4),
                          "frames_ms_max": round(fr[2], 4), "raw_ms": round(raw[0], 4),
                          "raw_ms_min": round(raw[1], 4), "raw_ms_max": round(raw[2], 4),
                          "frame_overhead": round(fr[0] / raw[0] - 1.0, 4),
                          "frames_measure_ms": round(ms[0], 4),
                          "frames_per_s": R * frames / fr[0] * 1e3,
                          "site_updates_per_s": R * sites * steps / fr[0] * 1e3,
                          "single_context_frames_ms": round(one_fr[0], 4),
                          "sequential_loop_ms": round(one_fr[0] * R, 3),
                          "speedup_over_sequential_loop": round(one_fr[0] * R / fr[0], 2),
                          "single_256_frame_overhead": round(big_over, 4), "guard_flags_set": flagged}), flush=True)
    # rollbacks: Δτ above the Euler limit, held
    shape, R = (32, 32, 32), 256
    with Phi4Ensemble(shape, R, seed=7, loops=loops, adapt_dtau=False, dtau=0.19, m2=1.0, lam=1.0, C=1.0) as ens:
        ens.init_field(0.3)
        ens.run_frames(frames)  # warm-up
        s0 = ens.perf()["steps"]
        oks = []
        fr = _median_ms(lambda: oks.append(ens.run_frames(frames)[0]), reps)
        executed = ens.perf()["steps"] - s0
    stable = float(sum(o.mean() for o in oks) / len(oks))
    print(json.dumps({"kind": "ensemble_rollbacks", "shape": list(shape), "R": R, "frames": frames, "loops": loops,
                      "dtau": 0.19, "adapt_dtau": False, "frames_ms": round(fr[0], 4),
                      "frames_ms_min": round(fr[1], 4), "frames_ms_max": round(fr[2], 4),
                      "frames_per_s": R * frames / fr[0] * 1e3, "stable_fraction": round(stable, 4),
                      "executed_step_fraction": round(executed / (reps * R * frames * loops), 4)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--loops", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--timeout", type=int, default=400, help="seconds for the child process")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.frames, a.loops, a.reps)
        return 0
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--frames", str(a.frames),
           "--loops", str(a.loops), "--reps", str(a.reps), "--worker"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    sys.stdout.flush()
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        print(f"bench_phi4_ens_frames: the worker failed with status {r.returncode}", file=sys.stderr)
        return r.returncode
    records = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"frames_per_call": a.frames, "loops": a.loops, "reps": a.reps, "params": PARAMS,
                   "records": records}, fh, indent=1)
        fh.write("\n")
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
