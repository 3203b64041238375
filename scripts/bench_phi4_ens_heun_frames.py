"""φ⁴ ensemble Heun frames (Phi4Ensemble.run_frames(scheme="heun")) against the
raw Heun steps they wrap, with the Euler pair beside them, GPU only.

    python scripts/bench_phi4_ens_heun_frames.py [--frames 50] [--loops 20] [--reps 5] [--out FILE]
    python scripts/bench_phi4_ens_heun_frames.py --against PARENT_CHECKOUT [--rounds 5]

Frames of `loops` steps at Δτ = 0.01 held (adapt_dtau off; every frame stable,
asserted), `frames` frames per call, at 32³ R = 256, 16³ R = 1024 and 8³
R = 4096.  One child process under `timeout` (this process never opens the GPU)
times, interleaved call by call, medians of `reps` after a warm-up of each:

  heun frames    run_frames(frames, scheme="heun")
  heun raw       step(frames * loops, scheme="heun")
  euler frames   run_frames(frames)
  euler raw      step(frames * loops)
  and both frames calls with measure=True

and one Heun case with rollbacks only: Δτ = 3 held (adapt_dtau off; the guard
rejects every frame), 32³, R = 256.  The yardstick per shape: the Heun frames'
overhead over the raw Heun steps, frames / raw - 1, is no larger than the Euler
frames' overhead of the same run (the record is taken once per Heun step, two
updates of work, so its share must not grow).  It is reported as met or missed
on the medians, with the overheads at the extremes of the run's spread beside
it.  Writes profiles/r07/phi4_ens_heun_frames/bench.json.

--against: the kernels that existed before (raw Euler step(200), raw Heun
step(200), Euler run_frames(50) at 32³ R = 256) from this tree and from a built
checkout of the parent commit, in `rounds` interleaved rounds of processes
(parent, this tree, parent again): per call the ratio this / parent and, as the
allowance, the ratio of the parent's two runs.  Added to the same file.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r07", "phi4_ens_heun_frames", "bench.json")
CASES = [((32, 32, 32), 256), ((16, 16, 16), 1024), ((8, 8, 8), 4096)]
PARAMS = dict(dtau=0.01, m2=0.5, lam=1.0, C=1.0)


def _interleaved_ms(fns, reps):
    """{name: (median, min, max)} of `reps` rounds, each timing every call once in turn."""
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            ts[k].append((time.perf_counter() - t0) * 1e3)
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}


def worker(frames, loops, reps):
    from stochquant_amd import Phi4Ensemble, _lib
    steps = frames * loops
    for shape, R in CASES:
        sites = shape[0] * shape[1] * shape[2]
        # Δτ held: with the controller on it grows by 1 / 0.95 every eleven stable frames, and the several
        # thousand frames of this run would carry it past the stability limit
        with Phi4Ensemble(shape, R, seed=7, loops=loops, adapt_dtau=False, **PARAMS) as ens:
            ens.init_field(0.5)

            def stable_frames(**kw):
                assert ens.run_frames(frames, **kw)[0].all()

            fns = {"heun_frames": lambda: stable_frames(scheme="heun"),
                   "heun_raw": lambda: ens.step(steps, scheme="heun"),
                   "euler_frames": lambda: stable_frames(),
                   "euler_raw": lambda: ens.step(steps),
                   "heun_frames_measure": lambda: stable_frames(measure=True, scheme="heun"),
                   "euler_frames_measure": lambda: stable_frames(measure=True)}
            for fn in fns.values():  # warm-up
                fn()
            t = _interleaved_ms(fns, reps)
            flagged = int(ens.flags().sum())
        over = {s: t[s + "_frames"][0] / t[s + "_raw"][0] - 1.0 for s in ("heun", "euler")}
        lo = {s: t[s + "_frames"][1] / t[s + "_raw"][2] - 1.0 for s in ("heun", "euler")}
        hi = {s: t[s + "_frames"][2] / t[s + "_raw"][1] - 1.0 for s in ("heun", "euler")}
        rec = {"kind": "ensemble", "shape": list(shape), "R": R, "frames": frames, "loops": loops}
        for k, (med, mn, mx) in t.items():
            rec[k + "_ms"] = round(med, 4)
            rec[k + "_ms_min"] = round(mn, 4)
            rec[k + "_ms_max"] = round(mx, 4)
        for s in ("heun", "euler"):
            rec[s + "_frame_overhead"] = round(over[s], 4)
            rec[s + "_frame_overhead_spread"] = [round(lo[s], 4), round(hi[s], 4)]
        rec["yardstick_heun_overhead_le_euler"] = bool(over["heun"] <= over["euler"])
        rec["heun_frames_per_s"] = R * frames / t["heun_frames"][0] * 1e3
        rec["heun_site_steps_per_s"] = R * sites * steps / t["heun_frames"][0] * 1e3
        rec["heun_over_euler_frames"] = round(t["heun_frames"][0] / t["euler_frames"][0], 4)
        rec["guard_flags_set"] = flagged
        rec["build_id"] = _lib.build_id()
        print(json.dumps(rec), flush=True)
    # rollbacks only: every frame trips the guard in its first steps and runs on to its end
    shape, R = (32, 32, 32), 256
    with Phi4Ensemble(shape, R, seed=7, loops=loops, adapt_dtau=False, dtau=3.0, m2=1.0, lam=1.0, C=1.0) as ens:
        ens.init_field(0.3)
        ens.run_frames(frames, scheme="heun")  # warm-up
        s0 = ens.perf()["steps"]
        oks = []
        t = _interleaved_ms({"fr": lambda: oks.append(ens.run_frames(frames, scheme="heun")[0])}, reps)["fr"]
        executed = ens.perf()["steps"] - s0
    stable = float(sum(o.mean() for o in oks) / len(oks))
    print(json.dumps({"kind": "ensemble_rollbacks", "scheme": "heun", "shape": list(shape), "R": R, "frames": frames,
                      "loops": loops, "dtau": 3.0, "adapt_dtau": False, "frames_ms": round(t[0], 4),
                      "frames_ms_min": round(t[1], 4), "frames_ms_max": round(t[2], 4),
                      "frames_per_s": R * frames / t[0] * 1e3, "stable_fraction": round(stable, 4),
                      "executed_step_fraction": round(executed / (reps * R * frames * loops), 4)}), flush=True)


def ab_worker(reps):
    """The calls both builds have, 32³ R = 256: one JSON line of medians."""
    from stochquant_amd import Phi4Ensemble, _lib
    with Phi4Ensemble((32, 32, 32), 256, seed=7, loops=20, adapt_dtau=False, **PARAMS) as ens:
        ens.init_field(0.5)
        fns = {"euler_step_200": lambda: ens.step(200),
               "heun_step_200": lambda: ens.step(200, scheme="heun"),
               "euler_frames_50": lambda: ens.run_frames(50)}
        for fn in fns.values():
            fn()
        t = _interleaved_ms(fns, reps)
    print(json.dumps({"build_id": _lib.build_id(), **{k: round(v[0], 4) for k, v in t.items()}}), flush=True)


def _child(root, args, timeout):
    env = dict(os.environ, PYTHONPATH=root)
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=root)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        raise SystemExit(f"bench_phi4_ens_heun_frames: a worker in {root} failed with status {r.returncode}")
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def _update(out, **fields):
    doc = {}
    if os.path.exists(out):
        with open(out) as fh:
            doc = json.load(fh)
    doc.update(fields)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(f"wrote {out}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=50)
    ap.add_argument("--loops", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--timeout", type=int, default=400, help="seconds for a child process")
    ap.add_argument("--against", help="a built checkout of the parent commit: time the calls both have")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--ab-worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker or a.ab_worker:
        sys.path.insert(0, os.getcwd())  # the tree the parent process chose
        if a.worker:
            worker(a.frames, a.loops, a.reps)
        else:
            ab_worker(a.reps)
        return 0
    if a.against:
        parent = os.path.abspath(a.against)
        runs = {"parent_a": [], "this": [], "parent_b": []}
        for _ in range(a.rounds):
            for name, root in (("parent_a", parent), ("this", ROOT), ("parent_b", parent)):
                runs[name].append(_child(root, ["--ab-worker", "--reps", str(a.reps)], a.timeout)[0])
        calls = ("euler_step_200", "heun_step_200", "euler_frames_50")
        med = {n: {c: statistics.median(r[c] for r in rs) for c in calls} for n, rs in runs.items()}
        summary = {c: {"parent_ms": round(med["parent_a"][c], 4), "this_ms": round(med["this"][c], 4),
                       "this_over_parent": round(med["this"][c] / med["parent_a"][c], 4),
                       "parent_over_parent": round(med["parent_b"][c] / med["parent_a"][c], 4)} for c in calls}
        print(json.dumps(summary, indent=1))
        _update(a.out, existing_kernels_vs_parent={"rounds": a.rounds, "reps": a.reps, "summary": summary,
                                                   "runs": runs})
        return 0
    records = _child(ROOT, ["--worker", "--frames", str(a.frames), "--loops", str(a.loops), "--reps", str(a.reps)],
                     a.timeout)
    for r in records:
        print(json.dumps(r))
    _update(a.out, frames_per_call=a.frames, loops=a.loops, reps=a.reps, params=PARAMS, records=records)
    return 0


if __name__ == "__main__":
    sys.exit(main())
