"""Cost of the φ⁴ ensemble's field digest and checkpoint (Phi4Ensemble.digest, save, load), GPU only.

    python scripts/bench_phi4_ens_checkpoint.py [--reps 5] [--dir SCRATCH] [--out FILE]
                                                [--parent-lib OTHER/libstochquant.so] [--pairs 5]

Child processes under `timeout` (this process never opens the GPU), one per measurement point, at 32³ R = 256,
16³ R = 1024 and 8³ R = 4096 -- 32 MiB of fields each:

  digest  digest() of all replicas against moments() of all replicas, which reads the same bytes, does more
          arithmetic (in double) and reads back five doubles per replica to the digest's one word: `reps`
          interleaved rounds after a warm-up round, CALLS calls per timing; medians, spreads, the ratio.
          Bound: digest <= 1.10 x moments.  With the kernel's resource use (isa_check.kernel_metadata).
  io      save(path) against download() + np.save + os.fsync of the same array, and load(path) against np.load +
          upload(), to files in --dir (default: the system's temporary directory), interleaved likewise.
          Bound: <= 1.5 x each.  The checkpoint moves the same bytes, makes one more pass over them on the host
          (the digest) and one launch of the digest kernel; the state file is small beside the field.
  --parent-lib: the existing calls must not move.  bench_phi4_ens_cluster.py's step(200) / run_frames(50) set with
          another build of the library (SQ_LIB), in `pairs` interleaved rounds of child processes: the other
          build, the other build again, this build.

A missed bound is recorded as missed.  Writes profiles/r07/phi4_ens_checkpoint/bench.json.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r07", "phi4_ens_checkpoint", "bench.json")
CASES = [((32, 32, 32), 256), ((16, 16, 16), 1024), ((8, 8, 8), 4096)]
CALLS = 20
DIGEST_BOUND, IO_BOUND = 1.10, 1.5


def _timed(fn, n=1):
    t0 = time.perf_counter()
    for _ in range(n):
        fn()          # every call ends in a stream synchronise
    return (time.perf_counter() - t0) * 1e3 / n


def _ens(shape, R):
    from stochquant_amd import Phi4Ensemble
    e = Phi4Ensemble(shape, R, seed=7, dtau=0.01)
    e.init_field(0.5)
    e.step(20)
    return e


def _rounds(calls, reps, n=1):
    ts = {k: [] for k in calls}
    for rnd in range(reps + 1):
        for k, fn in calls.items():
            t = _timed(fn, n)
            if rnd:
                ts[k].append(t)
    return ts


def _summary(ts, scale=1.0):
    return {"median": {k: round(statistics.median(v) * scale, 3) for k, v in ts.items()},
            "min_max": {k: [round(min(v) * scale, 3), round(max(v) * scale, 3)] for k, v in ts.items()}}


def digest_worker(case, reps):
    import numpy as np
    from stochquant_amd import _lib, isa_check
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import phi4_ens_checkpoint_format as fmt
    shape, R = CASES[case]
    with _ens(shape, R) as e:
        phi = e.download()
        assert int(e.digest(3, 1)[0]) == fmt.field_digest(phi[3])  # a spot check; the suite has the exact one
        ts = _rounds({"digest": e.digest, "moments": e.moments}, reps, CALLS)
    s = _summary(ts, 1e3)
    ratio = s["median"]["digest"] / s["median"]["moments"]
    md = isa_check.kernel_metadata(_lib.LIB_PATH)
    res = {k: v for k, v in md.items() if "phi4_ens_digest_kernel" in k}
    print(json.dumps({"kind": "digest", "shape": list(shape), "R": R, "calls_per_timing": CALLS, "us": s["median"],
                      "us_min_max": s["min_max"], "digest_over_moments": round(ratio, 4), "bound": DIGEST_BOUND,
                      "bound_met": bool(ratio <= DIGEST_BOUND), "kernel": next(iter(res.values()), None),
                      "build_id": _lib.build_id()}), flush=True)


def io_worker(case, reps, scratch):
    import numpy as np
    from stochquant_amd import _lib
    shape, R = CASES[case]
    d = tempfile.mkdtemp(prefix="sq_ckpt_bench_", dir=scratch)
    ck, ref = os.path.join(d, "ck.npy"), os.path.join(d, "ref.npy")

    def np_save(e):
        a = e.download()
        with open(ref, "wb") as fh:
            np.save(fh, a)
            fh.flush()
            os.fsync(fh.fileno())

    try:
        with _ens(shape, R) as e:
            save = _rounds({"save": lambda: e.save(ck), "download_np_save_fsync": lambda: np_save(e)}, reps)
            load = _rounds({"load": lambda: e.load(ck), "np_load_upload": lambda: e.upload(np.load(ref))}, reps)
            sizes = {s: os.path.getsize(ck + s) for s in ("", ".state", ".json")}
    finally:
        for f in os.listdir(d):
            os.remove(os.path.join(d, f))
        os.rmdir(d)
    out = {"kind": "io", "shape": list(shape), "R": R, "bytes": sizes, "bound": IO_BOUND, "build_id": _lib.build_id()}
    for name, ts, a, b in (("save", save, "save", "download_np_save_fsync"), ("load", load, "load", "np_load_upload")):
        s = _summary(ts)
        ratio = s["median"][a] / s["median"][b]
        out[name] = {"ms": s["median"], "ms_min_max": s["min_max"], "ratio": round(ratio, 4),
                     "bound_met": bool(ratio <= IO_BOUND)}
    print(json.dumps(out), flush=True)


def _child(args, timeout, env=None, script=__file__):
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(script)] + args
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        print(f"bench_phi4_ens_checkpoint: a child failed with status {r.returncode}; stopping", file=sys.stderr)
        return None
    print("done: " + " ".join(args), file=sys.stderr, flush=True)
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per call of the A/B of existing calls")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the timed files go (default: the temporary directory)")
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--parent-lib", default=None, help="another build of libstochquant.so for the A/B of existing calls")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--case", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--digest-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--io-worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.digest_worker:
        digest_worker(a.case, a.reps)
        return 0
    if a.io_worker:
        io_worker(a.case, a.reps, a.dir)
        return 0
    records = []

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"reps": a.reps, "records": records}, fh, indent=1)
            fh.write("\n")

    for worker in ("--digest-worker", "--io-worker"):
        for case in range(len(CASES)):
            args = ["--reps", str(a.reps), worker, "--case", str(case)] + (["--dir", a.dir] if a.dir else [])
            got = _child(args, a.timeout)
            if got is None:
                return 1
            records += got
            save()
    if a.parent_lib:
        penv = dict(os.environ, SQ_LIB=os.path.abspath(a.parent_lib))
        raw = os.path.join(ROOT, "scripts", "bench_phi4_ens_cluster.py")
        args = ["--steps", str(a.steps), "--reps", str(a.reps), "--raw-worker"]
        pairs = []
        for _ in range(a.pairs):   # parent, parent again, this build: two differences per round
            row = {}
            for name, env in (("parent", penv), ("parent_again", penv), ("this", None)):
                got = _child(args, a.timeout, env, raw)
                if got is None:
                    return 1
                row[name] = got[0]
            pairs.append(row)
        ab = {"kind": "existing_calls_vs_parent", "steps": a.steps, "pairs": pairs}
        for k in [k for k in pairs[0]["this"] if k.endswith("_ms")]:
            d = [(p["this"][k] / p["parent"][k] - 1.0) * 100.0 for p in pairs]
            s = [(p["parent_again"][k] / p["parent"][k] - 1.0) * 100.0 for p in pairs]
            ab[k[:-3]] = {"parent_median_ms": round(statistics.median(p["parent"][k] for p in pairs), 4),
                          "this_median_ms": round(statistics.median(p["this"][k] for p in pairs), 4),
                          "median_diff_percent": round(statistics.median(d), 3),
                          "min_diff_percent": round(min(d), 3), "max_diff_percent": round(max(d), 3),
                          "parent_self_median_diff_percent": round(statistics.median(s), 3),
                          "parent_self_min_diff_percent": round(min(s), 3),
                          "parent_self_max_diff_percent": round(max(s), 3),
                          "within_parent_spread": bool(abs(statistics.median(d)) <= max(abs(x) for x in s))}
        records.append(ab)
        save()
    for r in records:
        print(json.dumps(r))
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
