"""Cost and use of the φ⁴ ensemble's cluster sums (Phi4Ensemble.cluster_improved,
Phi4Ensemble.step_hmc_cluster_improved), GPU only.

    python scripts/bench_phi4_ens_cluster_improved.py [--reps 5] [--out FILE] [--no-gain]
                                                      [--parent-lib OTHER/libstochquant.so] [--pairs 5]

Child processes under `timeout` (this process never opens the GPU), one per
measurement point, at 32³ R = 256, 16³ R = 1024 and 8³ R = 4096, λ = 1, C = 1
and the pseudo-critical m² of bench_phi4_ens_cluster.py (−0.12 / −0.12 / −0.14):

  cost   on thermalised fields, `reps` interleaved rounds after a warm-up round:
         cluster(50) / 50 against cluster_improved(50) / 50 of one process;
         medians, spreads, the ratio, and beside it the passes synchronous
         minimum propagation takes on four replicas' recorded bonds in NumPy
         (tests/phi4_cluster_model.py; the kernel's own passes are not counted).
  gain   (skipped with --no-gain) R = 256 chains of randomised trajectories of
         mean length 1 with one sweep each, GAIN_ROUNDS rounds: the time per
         round of step_hmc_cluster and of step_hmc_cluster_improved (chunks of
         500, interleaved), then round by round the naive M² = (Σφ)² and
         |Σφ e^{ipz}|² of the field behind the sweep (pslices() at spatial
         momentum 0) beside the sweep's I2 and F_z.  The error of each mean by
         binning (the largest over bin lengths 1, 2, 4, .. with at least 16 bins
         per chain, bins pooled over the chains), and the yardstick
         (error_naive / error_improved)² > time_improved / time_plain.
  --parent-lib: the plain sweep and the existing calls must not move.
         cluster(50) at the three points and bench_phi4_ens_cluster.py's
         step(200) / run_frames(50) set with another build of the library
         (SQ_LIB), in `pairs` interleaved rounds of child processes: the other
         build, the other build again, this build.

Writes profiles/r07/phi4_ens_cluster_improved/bench.json.
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_phi4_ens_cluster import CASES, LAM, NLEAP, _thermal, _timed  # noqa: E402

DEFAULT_OUT = os.path.join(ROOT, "profiles", "r07", "phi4_ens_cluster_improved", "bench.json")
M2C = (-0.12, -0.12, -0.14)
GAIN_ROUNDS = 4000
CHUNK = 500
MIN_BINS = 16


def _drop_missing_signatures():
    """An older build lacks the newer exports, and the calls timed with it need none of them."""
    import ctypes
    from stochquant_amd import _lib
    have = ctypes.CDLL(os.environ.get("SQ_LIB", _lib.LIB_PATH))
    for name in [n for n in _lib.SIGNATURES if not hasattr(have, n)]:
        del _lib.SIGNATURES[name]


def cost_worker(case, reps):
    import numpy as np
    from stochquant_amd import Phi4Ensemble, _lib
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import phi4_cluster_model as cm
    (shape, R, dtau, _), m2 = CASES[case], M2C[case]
    with _thermal(shape, R, dtau, m2) as e:
        calls = {"plain": lambda: e.cluster(50), "improved": lambda: e.cluster_improved(50)}
        ts = {k: [] for k in calls}
        for rnd in range(reps + 1):
            for k, fn in calls.items():
                t = _timed(fn)
                if rnd:
                    ts[k].append(t)
        e.cluster_reset()
        ser, bonds, labels, _ = e.cluster_improved(1, record=True)
        st = e.cluster_stats()
        info = Phi4Ensemble.cluster_improved_shape_info(shape)
    lab, passes = zip(*(cm.components(bonds[0, r:r + 1], shape) for r in range(4)))
    assert all(np.array_equal(lab[r][0], labels[0, r]) for r in range(4))
    us = {k: statistics.median(v) / 50 * 1e3 for k, v in ts.items()}
    print(json.dumps({"kind": "cost", "shape": list(shape), "R": R, "dtau": dtau, "m2": m2, "lam": LAM, **info,
                      "ms_all": {k: [round(t, 4) for t in v] for k, v in ts.items()},
                      "us": {k: round(v, 3) for k, v in us.items()},
                      "us_min_max": {k: [round(min(v) / 50 * 1e3, 3), round(max(v) / 50 * 1e3, 3)]
                                     for k, v in ts.items()},
                      "improved_over_plain": round(us["improved"] / us["plain"], 4),
                      "model_passes_mean_of_4": round(float(np.mean(passes)), 2),
                      "clusters_per_sweep": round(float(st[:, 1].mean()), 1), "unconverged": int(st[:, 4].sum()),
                      "saturated_sites": float(ser[:, :, 7].sum()), "build_id": _lib.build_id()}), flush=True)


def binned_error(x):
    """(error, bin length) of the mean of x (rounds, chains): the largest standard error over bin lengths 1, 2, 4,
    .. that leave at least MIN_BINS bins per chain, the bins pooled over the chains."""
    import numpy as np
    n = x.shape[0]
    best, b = (0.0, 1), 1
    while n // b >= MIN_BINS:
        k = n // b
        m = x[:k * b].reshape(k, b, -1).mean(axis=1)
        err = float(m.std(ddof=1) / np.sqrt(m.size))
        if err > best[0]:
            best = (err, b)
        b *= 2
    return best


def gain_worker(case):
    import numpy as np
    from stochquant_amd import _lib
    (shape, _, dtau, nleap), m2, R = CASES[case], M2C[case], 256
    V, Lz = shape[0] * shape[1] * shape[2], shape[2]
    with _thermal(shape, R, dtau, m2, seed=31) as e:
        kw = dict(ntraj=1, nleap=nleap, randomize=True)
        calls = {"plain": lambda: e.step_hmc_cluster(CHUNK, **kw), "improved": lambda: e.step_hmc_cluster_improved(CHUNK, **kw)}
        ts = {k: [] for k in calls}
        for rnd in range(4):
            for k, fn in calls.items():
                t = _timed(fn)
                if rnd:
                    ts[k].append(t)
        e.set_momenta([(0, 0)])
        tw = np.exp(2j * np.pi * np.arange(Lz) / Lz)
        naive = np.zeros((GAIN_ROUNDS, R, 2))
        imp = np.zeros((GAIN_ROUNDS, R, 2))
        for i in range(GAIN_ROUNDS):
            _, cs = e.step_hmc_cluster_improved(1, **kw)
            AB, _ = e.pslices()
            S = AB[:, 0, :, 0]
            naive[i, :, 0] = S.sum(axis=1) ** 2
            naive[i, :, 1] = np.abs(S @ tw) ** 2
            imp[i, :, 0], imp[i, :, 1] = cs[0, :, 0], cs[0, :, 4]
        flagged, st = int(e.flags().sum()), e.cluster_stats()
    us = {k: statistics.median(v) / CHUNK * 1e3 for k, v in ts.items()}
    out = {"kind": "gain", "shape": list(shape), "R": R, "dtau": dtau, "m2": m2, "lam": LAM, "nleap": nleap,
           "rounds": GAIN_ROUNDS, "us_per_round": {k: round(v, 2) for k, v in us.items()},
           "time_ratio": round(us["improved"] / us["plain"], 4), "guard_flags_set": flagged,
           "unconverged": int(st[:, 4].sum()), "build_id": _lib.build_id()}
    for j, name in enumerate(("M2", "Fz")):
        en, ei = binned_error(naive[:, :, j]), binned_error(imp[:, :, j])
        gain = (en[0] / ei[0]) ** 2
        out[name] = {"naive_mean_over_V": round(float(naive[:, :, j].mean()) / V, 5),
                     "improved_mean_over_V": round(float(imp[:, :, j].mean()) / V, 5),
                     "naive_error_over_V": round(en[0] / V, 6), "naive_bin": en[1],
                     "improved_error_over_V": round(ei[0] / V, 6), "improved_bin": ei[1],
                     "variance_gain": round(gain, 3), "yardstick_met": bool(gain > us["improved"] / us["plain"])}
    print(json.dumps(out), flush=True)


def sweep_worker(reps):
    """The plain sweep at the three points, with whichever build SQ_LIB names."""
    from stochquant_amd import _lib
    _drop_missing_signatures()
    out = {}
    for (shape, R, dtau, _), m2 in zip(CASES, M2C):
        with _thermal(shape, R, dtau, m2) as e:
            e.cluster(50)
            out["sweep%d_ms" % shape[0]] = round(statistics.median(_timed(lambda: e.cluster(50)) for _ in range(reps)), 4)
    out["build_id"] = _lib.build_id()
    print(json.dumps(out), flush=True)


def _child(args, timeout, env=None, script=__file__):
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(script)] + args
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        print(f"bench_phi4_ens_cluster_improved: a child failed with status {r.returncode}; stopping", file=sys.stderr)
        return None
    print("done: " + " ".join(args), file=sys.stderr, flush=True)
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per call of the A/B of existing calls")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--parent-lib", default=None, help="another build of libstochquant.so for the A/B of existing calls")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--no-gain", action="store_true", help="skip the error-bar measurement")
    ap.add_argument("--no-cost", action="store_true", help="skip the cost measurement")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--case", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--cost-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--gain-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--sweep-worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.cost_worker:
        cost_worker(a.case, a.reps)
        return 0
    if a.gain_worker:
        gain_worker(a.case)
        return 0
    if a.sweep_worker:
        sweep_worker(a.reps)
        return 0
    records = []

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"reps": a.reps, "lam": LAM, "nleap": NLEAP, "m2c": list(M2C), "records": records}, fh, indent=1)
            fh.write("\n")

    for worker, skip in (("--cost-worker", a.no_cost), ("--gain-worker", a.no_gain)):
        for case in range(len(CASES)):
            if skip:
                continue
            got = _child(["--reps", str(a.reps), worker, "--case", str(case)], a.timeout)
            if got is None:
                return 1
            records += got
            save()
    if a.parent_lib:
        penv = dict(os.environ, SQ_LIB=os.path.abspath(a.parent_lib))
        raw = os.path.join(ROOT, "scripts", "bench_phi4_ens_cluster.py")
        jobs = ((["--reps", str(a.reps), "--sweep-worker"], __file__),
                (["--steps", str(a.steps), "--reps", str(a.reps), "--raw-worker"], raw))
        pairs = []
        for _ in range(a.pairs):   # parent, parent again, this build: two differences per round
            row = {}
            for name, env in (("parent", penv), ("parent_again", penv), ("this", None)):
                row[name] = {}
                for args, script in jobs:
                    got = _child(args, a.timeout, env, script)
                    if got is None:
                        return 1
                    row[name].update(got[0])
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
