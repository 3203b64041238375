"""Cost and use of the φ⁴ ensemble's cluster sweep (Phi4Ensemble.cluster,
Phi4Ensemble.step_hmc_cluster), GPU only.

    python scripts/bench_phi4_ens_cluster.py [--reps 5] [--out FILE] [--no-gain]
                                             [--parent-lib OTHER/libstochquant.so] [--pairs 5] [--ab-only]

Child processes under `timeout` (this process never opens the GPU), at 32³
R = 256, 16³ R = 1024 and 8³ R = 4096, λ = 1, C = 1:

  scan   the pseudo-critical m² of the shape: one ensemble whose replicas are
         dealt to a list of m², thermalised by Euler steps and rounds of
         trajectories with sweeps, then SCAN_ROUNDS rounds of step_hmc_cluster
         with a record each; χ = (<M²> - <|M|>²) / V per m², M = Σφ; the peak.
         (The sums are those `step(every=..)` records; the sampler is the one
         that decorrelates near the peak.)
  cost   at m² = 0.5 (small clusters), the pseudo-critical m² and m² = -0.3 (a
         percolating cluster), on thermalised fields, interleaved round by round
         (`reps` rounds after a warm-up round, medians):
           sweep     cluster(50) / 50
           traj      step_hmc(50, nleap=10) / 50: the yardstick, sweep <= traj
           fused     step_hmc_cluster(50, ntraj=1, nleap=10) / 50
           loop      50 x [step_hmc(1, nleap=10), cluster(1)]
         and, of one replica's recorded bonds, the clusters, the largest one and
         the passes synchronous minimum propagation with pointer jumping takes
         in NumPy (tests/phi4_cluster_model.py: a measure of the clusters'
         extent; the kernel's own passes are not counted).
  gain   (skipped with --no-gain) at the pseudo-critical m² of 16³ and 32³,
         R = 256: τ_int of |Σφ| and Σφ² (window 20 τ_int, ρ averaged over the
         replicas) and the wall time per update, for randomised HMC alone and
         for the same HMC with one sweep per trajectory, and their products;
         at 8³, m² = -0.3: the sign changes of Σφ per 1000 updates of both.

--parent-lib: the existing calls must not move (their objects are the other
build's byte for byte).  step(200) with the Euler, Heun, MALA and HMC schemes
and run_frames(50) at 32³ R = 256 with this build and with another build of the
library (SQ_LIB), in interleaved rounds of child processes, the other build
twice.  Writes profiles/r07/phi4_ens_cluster/bench.json.
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
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r07", "phi4_ens_cluster", "bench.json")
# shape, replicas, dtau (bench_phi4_ens_hmc.py: acceptance 0.75 at nleap = 10), nleap of mean trajectory length 1
CASES = [((32, 32, 32), 256, 0.00106, 36), ((16, 16, 16), 1024, 0.00657, 21), ((8, 8, 8), 4096, 0.0101, 14)]
LAM = 1.0
NLEAP = 10
THERMALISE = 1000
SCAN_M2 = (-0.02, -0.05, -0.08, -0.10, -0.12, -0.14, -0.17, -0.21)
SCAN_ROUNDS = 1000
GAIN_UPDATES = 4000
FRAMES = 50


def _timed(fn):
    t0 = time.perf_counter()
    fn()          # every call ends in a stream synchronise
    return (time.perf_counter() - t0) * 1e3


def _thermal(shape, R, dtau, m2, seed=7, rounds=200):
    from stochquant_amd import Phi4Ensemble
    e = Phi4Ensemble(shape, R, seed=seed, dtau=dtau, m2=m2, lam=LAM, C=1.0)
    e.init_field(0.5)
    e.step(THERMALISE)
    e.step_hmc_cluster(rounds, ntraj=1, nleap=NLEAP, randomize=True)
    return e


def scan_worker():
    import numpy as np
    from stochquant_amd import _lib
    for shape, R, dtau, _ in CASES:
        V = shape[0] * shape[1] * shape[2]
        per = R // len(SCAN_M2)
        m2 = np.repeat(np.asarray(SCAN_M2), per)
        with _thermal(shape, len(m2), dtau, m2, rounds=500) as e:
            M = e.step_hmc_cluster(SCAN_ROUNDS, ntraj=1, nleap=NLEAP, randomize=True, every=1)[:, :, 0]
            flagged = int(e.flags().sum())
        M = M.reshape(SCAN_ROUNDS, len(SCAN_M2), per)
        chi = ((M * M).mean(axis=(0, 2)) - np.abs(M).mean(axis=(0, 2)) ** 2) / V
        absm = np.abs(M).mean(axis=(0, 2)) / V
        k = int(np.argmax(chi))
        print(json.dumps({"kind": "scan", "shape": list(shape), "R": len(m2), "replicas_per_m2": per, "dtau": dtau,
                          "lam": LAM, "rounds": SCAN_ROUNDS, "m2": list(SCAN_M2),
                          "chi": [round(float(c), 4) for c in chi], "abs_m": [round(float(a), 5) for a in absm],
                          "m2_peak": SCAN_M2[k], "peak_inside": bool(0 < k < len(SCAN_M2) - 1),
                          "guard_flags_set": flagged, "build_id": _lib.build_id()}), flush=True)


def cost_worker(reps, m2c):
    import numpy as np
    from stochquant_amd import Phi4Ensemble, _lib
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import phi4_cluster_model as cm
    for (shape, R, dtau, _), crit in zip(CASES, m2c):
        V = shape[0] * shape[1] * shape[2]
        for name, m2 in (("small", 0.5), ("critical", crit), ("percolating", -0.3)):
            with _thermal(shape, R, dtau, m2) as e:
                def loop():
                    for _ in range(50):
                        e.step_hmc(1, nleap=NLEAP)
                        e.cluster(1)

                calls = {"sweep": lambda: e.cluster(50), "traj": lambda: e.step_hmc(50, nleap=NLEAP),
                         "fused": lambda: e.step_hmc_cluster(50, ntraj=1, nleap=NLEAP), "loop": loop}
                ts = {k: [] for k in calls}
                for rnd in range(reps + 1):
                    for k, fn in calls.items():
                        t = _timed(fn)
                        if rnd:
                            ts[k].append(t)
                e.cluster_reset()
                bonds, labels = e.cluster(1, record=True)
                st = e.cluster_stats()
                hs = e.hmc_stats()
                flagged = int(e.flags().sum())
                info = Phi4Ensemble.cluster_shape_info(shape)
            lab, passes = cm.components(bonds[0, :1], shape)
            assert np.array_equal(lab[0], labels[0, 0])
            us = {k: statistics.median(v) / 50 * 1e3 for k, v in ts.items()}
            print(json.dumps({"kind": "cost", "point": name, "shape": list(shape), "R": R, "dtau": dtau, "m2": m2,
                              "lam": LAM, "K": info["K"], "T": info["T"], "lds_bytes": info["lds_bytes"],
                              "ms_all": {k: [round(t, 4) for t in v] for k, v in ts.items()},
                              "us": {k: round(v, 3) for k, v in us.items()},
                              "sweep_over_traj": round(us["sweep"] / us["traj"], 4),
                              "sweep_yardstick_met": bool(us["sweep"] <= us["traj"]),
                              "fused_over_loop": round(us["fused"] / us["loop"], 4),
                              "fused_over_sum": round(us["fused"] / (us["sweep"] + us["traj"]), 4),
                              "clusters_per_sweep": round(float(st[:, 1].mean()), 1),
                              "flipped_sites_per_sweep": round(float(st[:, 3].mean()), 1),
                              "unconverged": int(st[:, 4].sum()),
                              "largest_cluster_fraction_replica0": round(float(np.bincount(lab[0]).max()) / V, 4),
                              "model_passes_replica0": passes,
                              "hmc_acceptance": round(float(hs[:, 1].sum() / max(hs[:, 0].sum(), 1)), 4),
                              "guard_flags_set": flagged, "build_id": _lib.build_id()}), flush=True)


def _sign_changes(s1):
    import numpy as np
    s = np.sign(s1)
    return (s[1:] * s[:-1] < 0).sum(axis=0)


def gain_worker(m2c):
    import numpy as np
    from bench_phi4_ens_hmc import tau_int
    from stochquant_amd import _lib
    chunk = 1000
    for (shape, _, dtau, nleap), crit in zip(CASES, m2c):
        R = 256
        broken = shape == (8, 8, 8)
        m2 = -0.3 if broken else crit
        out = {"kind": "gain", "shape": list(shape), "R": R, "dtau": dtau, "m2": m2, "lam": LAM, "nleap": nleap,
               "randomize": True, "updates": GAIN_UPDATES, "build_id": _lib.build_id()}
        for name in ("hmc", "hmc_cluster"):
            with _thermal(shape, R, dtau, m2, seed=31) as e:
                run = (lambda: e.step_hmc(chunk, nleap=nleap, randomize=True, every=1)) if name == "hmc" else \
                      (lambda: e.step_hmc_cluster(chunk, ntraj=1, nleap=nleap, randomize=True, every=1))
                run()
                parts = []
                t0 = time.perf_counter()
                for _ in range(GAIN_UPDATES // chunk):
                    parts.append(run()[:, :, :2].copy())
                wall = (time.perf_counter() - t0) / GAIN_UPDATES
                flagged = int(e.flags().sum())
            ser = np.concatenate(parts)
            a, b = tau_int(ser[:, :, 1]), tau_int(np.abs(ser[:, :, 0]))
            ch = _sign_changes(ser[:, :, 0])
            out[name] = {"us_per_update": round(wall * 1e6, 2), "tau_int_S2": round(a[0], 2), "window_S2": a[1],
                         "tau_int_absM": round(b[0], 2), "window_absM": b[1],
                         "series_over_window": round(GAIN_UPDATES / max(a[1], b[1]), 1),
                         "cost_S2_us": round(a[0] * wall * 1e6, 1), "cost_absM_us": round(b[0] * wall * 1e6, 1),
                         "sign_changes_per_1000_updates": round(float(ch.mean()) / GAIN_UPDATES * 1e3, 3),
                         "chains_that_changed_sign": int((ch > 0).sum()), "guard_flags_set": flagged}
        h, c = out["hmc"], out["hmc_cluster"]
        out["cost_ratio_hmc_over_cluster_S2"] = round(h["cost_S2_us"] / c["cost_S2_us"], 2)
        out["cost_ratio_hmc_over_cluster_absM"] = round(h["cost_absM_us"] / c["cost_absM_us"], 2)
        print(json.dumps(out), flush=True)


def raw_worker(steps, reps):
    import ctypes
    from stochquant_amd import Phi4Ensemble, _lib
    # an older build lacks the newer exports, and these calls need none of them
    have = ctypes.CDLL(os.environ.get("SQ_LIB", _lib.LIB_PATH))
    for name in [n for n in _lib.SIGNATURES if not hasattr(have, n)]:
        del _lib.SIGNATURES[name]
    kw = dict(seed=7, dtau=0.004, m2=0.5, lam=1.0, C=1.0)
    with Phi4Ensemble((32, 32, 32), 256, **kw) as ens:
        ens.init_field(0.5)
        ens.step(THERMALISE)
        ens.step(steps, scheme="heun")
        ens.step(steps, scheme="mala")
        ens.step_hmc(steps, nleap=NLEAP)
        euler = statistics.median(_timed(lambda: ens.step(steps)) for _ in range(reps))
        heun = statistics.median(_timed(lambda: ens.step(steps, scheme="heun")) for _ in range(reps))
        mala = statistics.median(_timed(lambda: ens.step(steps, scheme="mala")) for _ in range(reps))
        hmc = statistics.median(_timed(lambda: ens.step_hmc(steps, nleap=NLEAP)) for _ in range(reps))
    with Phi4Ensemble((32, 32, 32), 256, **kw) as ens:
        ens.init_field(0.5)
        ens.run_frames(FRAMES)
        frames = statistics.median(_timed(lambda: ens.run_frames(FRAMES)) for _ in range(reps))
    print(json.dumps({"euler_ms": round(euler, 4), "heun_ms": round(heun, 4), "mala_ms": round(mala, 4),
                      "hmc_ms": round(hmc, 4), "frames_ms": round(frames, 4), "build_id": _lib.build_id()}), flush=True)


def _child(args, timeout, env=None):
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        print(f"bench_phi4_ens_cluster: a child failed with status {r.returncode}; stopping", file=sys.stderr)
        return None
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per call of the A/B of existing calls")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--parent-lib", default=None, help="another build of libstochquant.so for the A/B of existing calls")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--no-gain", action="store_true", help="skip the autocorrelation measurement")
    ap.add_argument("--ab-only", action="store_true", help="only the A/B of existing calls (needs --parent-lib)")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--m2c", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--scan-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--cost-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--gain-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--raw-worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    m2c = [float(v) for v in a.m2c.split(",")] if a.m2c else None
    if a.scan_worker:
        scan_worker()
        return 0
    if a.cost_worker:
        cost_worker(a.reps, m2c)
        return 0
    if a.gain_worker:
        gain_worker(m2c)
        return 0
    if a.raw_worker:
        raw_worker(a.steps, a.reps)
        return 0
    records = []

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"reps": a.reps, "lam": LAM, "thermalise": THERMALISE, "nleap": NLEAP, "records": records}, fh,
                      indent=1)
            fh.write("\n")

    if not a.ab_only:
        got = _child(["--scan-worker"], a.timeout)
        if got is None:
            return 1
        records += got
        save()
        crit = ",".join(str(r["m2_peak"]) for r in got)
        got = _child(["--reps", str(a.reps), "--cost-worker", "--m2c=" + crit], a.timeout)
        if got is None:
            return 1
        records += got
        save()
    if not a.no_gain and not a.ab_only:
        got = _child(["--gain-worker", "--m2c=" + crit], a.timeout)
        if got is None:
            return 1
        records += got
        save()
    if a.parent_lib:
        common = ["--steps", str(a.steps), "--reps", str(a.reps), "--raw-worker"]
        penv = dict(os.environ, SQ_LIB=os.path.abspath(a.parent_lib))
        pairs = []
        for _ in range(a.pairs):   # parent, parent again, this build: two differences per round
            runs = [_child(common, a.timeout, penv)]
            runs.append(_child(common, a.timeout, penv) if runs[0] is not None else None)
            runs.append(_child(common, a.timeout) if runs[1] is not None else None)
            if runs[2] is None:
                return 1
            old, old2, new = (r[0] for r in runs)
            pairs.append({"parent": old, "parent_again": old2, "this": new})
        ab = {"kind": "existing_calls_vs_parent", "shape": [32, 32, 32], "R": 256, "steps": a.steps, "nframes": FRAMES,
              "pairs": pairs, "parent_build_id": pairs[0]["parent"]["build_id"],
              "this_build_id": pairs[0]["this"]["build_id"]}
        for k in ("euler_ms", "heun_ms", "mala_ms", "hmc_ms", "frames_ms"):
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
        records.append(ab)
        save()
    for r in records:
        print(json.dumps(r))
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
