"""Cost of the single φ⁴ lattice's cluster sweeps (Phi4Lattice.cluster), GPU only.

    python scripts/bench_phi4_cluster.py [--reps 5] [--out FILE] [--sweeps-only SHAPE]

λ = 1, C = 1, at m² = 0.5 and at m² = -0.14, the pseudo-critical m² of 32³ from bench_phi4_ens_cluster.py's scan.
Fields: 100 Euler steps, then 20 HMC trajectories of nleap = 10.  After a warm-up round, `reps` rounds of these
calls, interleaved in one process, each ended by a device synchronise; medians, min and max per unit:

  ens      Phi4Ensemble(32³, R = 256).cluster(4) / 4     the yardstick's sweep: 8,388,608 sites in one launch
  sweep    Phi4Lattice(256 x 256 x 128).cluster(4) / 4   the same site count
  copy     device-to-device copy moving the bytes the design adds per site: the label array written, read and
           written again (12 B), the bond byte written and read (2 B), the second pass over the field (4 B) --
           18 B per site, timed as a copy of 9 B per site (sq_copy_bandwidth counts both directions)
  sweep / (1.25 (ens + copy)): the yardstick, 25 % for the seam unions and two more launch tails.
  per shape 64³, 256 x 256 x 128, 256³: cluster(4) / 4 against step_hmc(2, nleap=10) / 2 (yardstick <= 1 x).

--sweeps-only Lx,Ly,Lz: 10 sweeps of that lattice at m² = -0.14 and nothing else, for a kernel trace.
Writes profiles/r07/phi4_cluster/bench.json.
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
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r07", "phi4_cluster", "bench.json")
LAM, C, M2S = 1.0, 1.0, (0.5, -0.14)
BIG = (256, 256, 128)
SHAPES = {(64, 64, 64): 0.0016, BIG: 0.0004, (256, 256, 256): 0.0004}
COPY_BYTES = 9


def timed(sync, fn):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return time.perf_counter() - t0


def lattice(shape, m2):
    from stochquant_amd import Phi4Lattice
    L = Phi4Lattice(shape, dtau=SHAPES.get(tuple(shape), 0.0004), m2=m2, lam=LAM, C=C, seed=1234)
    L.init_field(0.5)
    L.step(100)
    L.step_hmc(20, nleap=10)
    return L


def stat(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def bench_m2(m2, reps):
    from stochquant_amd import Phi4Ensemble, _lib
    out = {"m2": m2}
    with Phi4Ensemble((32, 32, 32), 256, dtau=0.004, m2=m2, lam=LAM, C=C, seed=7) as E:
        E.init_field(0.5)
        E.step(100)
        E.step_hmc(20, nleap=10)
        lats = {s: lattice(s, m2) for s in SHAPES}
        calls = {"ens": (lambda: None, lambda: E.cluster(4), 4)}    # the ensemble call waits for its launches itself
        for s, L in lats.items():
            calls["sweep %dx%dx%d" % s] = (L.sync, (lambda L=L: L.cluster(4)), 4)
            calls["hmc10 %dx%dx%d" % s] = (L.sync, (lambda L=L: L.step_hmc(2, nleap=10)), 2)
        us = {k: [] for k in list(calls) + ["copy"]}
        sites = BIG[0] * BIG[1] * BIG[2]
        for r in range(reps + 1):
            for k, (sync, fn, cnt) in calls.items():
                t = timed(sync, fn) / cnt * 1e6
                if r:
                    us[k].append(t)
            g = ctypes.c_double()
            _lib.call("sq_copy_bandwidth", 0, COPY_BYTES * sites, 20, ctypes.byref(g))
            if r:
                us["copy"].append(2.0 * COPY_BYTES * sites / (g.value * 1e9) * 1e6)
        out["us"] = {k: stat(v) for k, v in us.items()}
        med = {k: out["us"][k]["median"] for k in us}
        big = "%dx%dx%d" % BIG
        out["yardstick_us"] = 1.25 * (med["ens"] + med["copy"])
        out["sweep_over_yardstick"] = med["sweep " + big] / out["yardstick_us"]
        out["yardstick_met"] = out["sweep_over_yardstick"] <= 1.0
        out["sweep_over_hmc10"] = {"%dx%dx%d" % s: med["sweep %dx%dx%d" % s] / med["hmc10 %dx%dx%d" % s] for s in lats}
        out["cluster_stats"] = {"%dx%dx%d" % s: [int(v) for v in L.cluster_stats()] for s, L in lats.items()}
        out["ens_unconverged"] = int(E.cluster_stats()[:, 4].sum())
        for L in lats.values():
            L.close()
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--sweeps-only", default=None)
    a = ap.parse_args()
    from stochquant_amd import Phi4Lattice, _lib
    if _lib.device_count() < 1:
        raise SystemExit("no HIP device: this benchmark measures on the GPU only")
    if a.sweeps_only:
        shape = tuple(int(v) for v in a.sweeps_only.split(","))
        with lattice(shape, M2S[1]) as L:
            L.cluster(10)
            L.sync()
            print(json.dumps({"shape": shape, "tile": Phi4Lattice.cluster_shape_info(shape), "stats": [int(v) for v in L.cluster_stats()]}))
        return
    res = [bench_m2(m2, a.reps) for m2 in M2S]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"reps": a.reps, "lam": LAM, "C": C, "results": res}, fh, indent=1)


if __name__ == "__main__":
    main()
