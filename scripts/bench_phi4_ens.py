"""φ⁴ ensemble step time (Phi4Ensemble) against the sequential loop it replaces
(one Phi4Lattice of the same shape stepped R times over), GPU only.

    python scripts/bench_phi4_ens.py [--steps 200] [--reps 5] [--out FILE]

Shapes 8³, 16³, 32³; R in {1, 256, 1024} and 4096 for 8³ and 16³; `steps`
steps per call with every = 0 and every = 20.  Each shape runs in a child
process of its own under `timeout` (this process never opens the GPU), which
times, in that one process: one Phi4Lattice of the shape for the same steps
(x R = the cost of the sequential loop), the 256³ sq_step rate, and every
ensemble case.  Times are medians of `reps` calls after a warm-up call, host
clock around calls that return with the stream idle.  The first failing child
ends the run.  Writes profiles/r07/phi4_ens/bench_phi4_ens.json.
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
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r07", "phi4_ens", "bench_phi4_ens.json")
SHAPES = [(8, 8, 8), (16, 16, 16), (32, 32, 32)]
PARAMS = dict(dtau=0.01, m2=0.5, lam=1.0, C=1.0)


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def worker(shape, steps, reps):
    from stochquant_amd import Phi4Ensemble, Phi4Lattice, _lib
    sites = shape[0] * shape[1] * shape[2]

    def lattice_ms(shp):
        with Phi4Lattice(shp, seed=7, **PARAMS) as lat:
            lat.init_field(0.5)

            def call():
                lat.step(steps)
                lat.sync()
            call()  # warm-up: code objects, the context's launch choices
            call()
            return _median_ms(call, reps)

    single_ms, single_min, single_max = lattice_ms(shape)
    big_ms, _, _ = lattice_ms((256, 256, 256))
    big_rate = 256 ** 3 * steps / big_ms * 1e3
    print(json.dumps({"kind": "single", "shape": list(shape), "steps": steps, "ms_per_call": round(single_ms, 4),
                      "ms_min": round(single_min, 4), "ms_max": round(single_max, 4),
                      "site_updates_per_s": sites * steps / single_ms * 1e3,
                      "sq_step_256_ms_per_call": round(big_ms, 4), "sq_step_256_site_updates_per_s": big_rate,
                      "build_id": _lib.build_id()}), flush=True)
    Rs = [1, 256, 1024] + ([4096] if sites <= 4096 else [])
    for R in Rs:
        ms0 = None
        for every in (0, 20):
            with Phi4Ensemble(shape, R, seed=7, **PARAMS) as ens:
                ens.init_field(0.5)
                ens.step(steps, every=every)  # warm-up
                ms, lo, hi = _median_ms(lambda: ens.step(steps, every=every), reps)
                flagged = int(ens.flags().sum())
            rate = R * sites * steps / ms * 1e3
            rec = {"kind": "ensemble", "shape": list(shape), "R": R, "steps": steps, "every": every,
                   "ms_per_call": round(ms, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                   "site_updates_per_s": rate, "sequential_loop_ms": round(single_ms * R, 3),
                   "speedup_over_sequential_loop": round(single_ms * R / ms, 2),
                   "rate_over_sq_step_256": round(rate / big_rate, 4), "guard_flags_set": flagged}
            if every == 0:
                ms0 = ms
            else:
                rec["every_overhead_percent"] = round((ms / ms0 - 1.0) * 100.0, 2)
            print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per shape (one child process each)")
    ap.add_argument("--worker", type=int, nargs=3, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(tuple(a.worker), a.steps, a.reps)
        return 0
    records = []
    for shape in SHAPES:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--steps", str(a.steps),
               "--reps", str(a.reps), "--worker"] + [str(s) for s in shape]
        r = subprocess.run(cmd, capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode != 0:
            sys.stderr.write(r.stderr)
            print(f"bench_phi4_ens: shape {shape} failed with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
        records += [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"steps_per_call": a.steps, "reps": a.reps, "params": PARAMS, "records": records}, fh, indent=1)
        fh.write("\n")
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
