"""Cost and acceptance of the single φ⁴ lattice's HMC trajectories (Phi4Lattice.step_hmc), GPU only.

    python scripts/bench_phi4_hmc.py [--shapes 64,256,512] [--reps 5] [--out FILE]

Per shape L³: 200 Euler steps, then Δτ tuned to an acceptance near 0.75 at nleap = 10 (pilots of 40
trajectories; Δτ x 1.25 above 0.80, x 0.8 below 0.70), then `reps` rounds after a warm-up round of these calls,
interleaved, each ended by a device synchronise, medians and min / max per call:

  euler   20 x step(1)                 the plain one-step kernel, the trajectory's first step
  hmc1    step_hmc(n, nleap=1)         first step + two term passes + verdict + commit
  hmc2    step_hmc(n, nleap=2)
  hmc10   step_hmc(n, nleap=10)
  copy    sq_copy_bandwidth of one field (device to device, 8 B per site)

Derived: leap = (hmc10 - hmc2) / 8 per interior step; rest = hmc1 - euler (the term passes, the verdict and the
commit together: the term passes cannot be timed alone through the public interface, so the whole-trajectory
yardstick of 1.15 x [euler + 9 leap + 2 term] is reported with `rest` in place of the two term passes).
Yardstick of the leap step: 1.5 x 1.25 x copy (12 B against 8 B per site, 25 % for halo re-reads).
Writes profiles/r07/phi4_hmc/bench.json.
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r07", "phi4_hmc", "bench.json")
PARAMS = dict(m2=0.5, lam=1.0, C=1.0)
DTAU0 = {64: 0.0016, 256: 0.0004, 512: 0.00018}


def timed(L, fn):
    L.sync()
    t0 = time.perf_counter()
    fn()
    L.sync()
    return time.perf_counter() - t0


def tune(L):
    acc = None
    for _ in range(8):
        L.hmc_reset()
        L.step_hmc(40, nleap=10)
        st = L.hmc_stats()
        acc = st[1] / st[0]
        if 0.70 <= acc <= 0.80:
            break
        L.dtau = L.dtau * (1.25 if acc > 0.80 else 0.8)
    return acc


def bench_shape(n, reps):
    from stochquant_amd import Phi4Lattice, _lib
    ntraj = 20 if n <= 256 else 6
    with Phi4Lattice((n, n, n), dtau=DTAU0.get(n, 0.1 / n ** 1.5), seed=1234, **PARAMS) as L:
        L.init_field(0.5)
        L.step(200)
        acc = tune(L)
        calls = {
            "euler": (20, lambda: [L.step(1) for _ in range(20)]),
            "hmc1": (ntraj, lambda: L.step_hmc(ntraj, nleap=1)),
            "hmc2": (ntraj, lambda: L.step_hmc(ntraj, nleap=2)),
            "hmc10": (ntraj, lambda: L.step_hmc(ntraj, nleap=10)),
        }
        us = {k: [] for k in list(calls) + ["copy"]}
        for r in range(reps + 1):
            for k, (cnt, fn) in calls.items():
                t = timed(L, fn) / cnt * 1e6
                if r:
                    us[k].append(t)
            g = ctypes.c_double()
            _lib.call("sq_copy_bandwidth", 0, 4 * n ** 3, 20, ctypes.byref(g))
            if r:
                us["copy"].append(2.0 * 4 * n ** 3 / (g.value * 1e9) * 1e6)
        L.hmc_reset()
        L.step_hmc(5 * ntraj, nleap=10)
        st = L.hmc_stats()
        med = {k: statistics.median(v) for k, v in us.items()}
        leap = (med["hmc10"] - med["hmc2"]) / 8.0
        rest = med["hmc1"] - med["euler"]
        out = {
            "shape": [n, n, n], "dtau": L.dtau, "pilot_acceptance": acc, "acceptance": st[1] / st[0],
            "guard_trips": int(st[2]), "us": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in us.items()},
            "us_per_leap_step": leap, "us_terms_verdict_commit": rest,
            "leap_yardstick_us": 1.5 * 1.25 * med["copy"], "leap_met": leap <= 1.5 * 1.25 * med["copy"],
            "trajectory_yardstick_us": 1.15 * (med["euler"] + 9.0 * leap + rest),
            "trajectory_met": med["hmc10"] <= 1.15 * (med["euler"] + 9.0 * leap + rest),
        }
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64,256,512")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    from stochquant_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("no HIP device: this benchmark measures on the GPU only")
    res = [bench_shape(int(s), a.reps) for s in a.shapes.split(",")]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"reps": a.reps, "params": PARAMS, "results": res}, fh, indent=1)


if __name__ == "__main__":
    main()
