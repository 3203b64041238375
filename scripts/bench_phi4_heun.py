"""Cost and bias of the single φ⁴ lattice's Heun step (Phi4Lattice.step(n, scheme="heun")), GPU only.

    python scripts/bench_phi4_heun.py [--shapes 64,256,512] [--reps 5] [--bias 64] [--out FILE]

Per shape L³: 200 Euler steps, then `reps` rounds after a warm-up round of these calls, interleaved, each ended by
a device synchronise (a window repeats its call until it holds about 50 ms of work), medians and min / max:

  heun      step(200, scheme="heun")       200 Heun steps = 400 launches
  euler1    400 x step(1), one sync        400 launches of the plain one-step kernel, the one stage 1 runs
  fused     step(400)                      the fused Euler path of sq_step

Yardstick (gated): heun / euler1 <= 1.20.  Reported beside it: heun / fused.

--bias L (0: skip): a free lattice L³ (λ = 0, m² = 1, C = 1, Δτ = 0.05), 2000 steps of thermalisation, then 200
measurements of ⟨φ²⟩ = Σφ² / V, one every 50 steps, with each scheme; beside them the stationary ⟨φ²⟩ of each
scheme and of the continuum equation, exact on that lattice: per momentum, with K = m² + Σ_μ (2 − 2 cos p_μ),
1 / (K (1 − ΔτK / 2)) for Euler, b² / (1 − a²) with a = 1 − ΔτK + (ΔτK)² / 2, b² = 2Δτ (1 − ΔτK / 2)² for Heun,
1 / K for the continuum.  The error is the standard error of the 200 values taken as independent.
Writes profiles/r07/phi4_heun/bench.json.
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r07", "phi4_heun", "bench.json")
PARAMS = dict(m2=0.5, lam=1.0, C=1.0)
DTAU0 = {64: 0.0016, 256: 0.0004, 512: 0.00018}
NHEUN = 200
WINDOW_S = 0.05
BIAS = dict(dtau=0.05, m2=1.0, therm=2000, every=50, nmeas=200)


def timed(L, fn, inner):
    L.sync()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    L.sync()
    return (time.perf_counter() - t0) / inner


def bench_shape(n, reps):
    from stochquant_amd import Phi4Lattice
    with Phi4Lattice((n, n, n), dtau=DTAU0.get(n, 0.1 / n ** 1.5), seed=1234, **PARAMS) as L:
        L.init_field(0.5)
        L.step(200)

        def euler1():
            for _ in range(2 * NHEUN):
                L.step(1)

        calls = {"heun": lambda: L.step(NHEUN, scheme="heun"), "euler1": euler1, "fused": lambda: L.step(2 * NHEUN)}
        inner = {k: max(1, int(WINDOW_S / timed(L, fn, 1))) for k, fn in calls.items()}     # also the warm-up round
        us = {k: [] for k in calls}
        for _ in range(reps):
            for k, fn in calls.items():
                us[k].append(timed(L, fn, inner[k]) * 1e6)
        med = {k: statistics.median(v) for k, v in us.items()}
        out = {
            "shape": [n, n, n], "dtau": L.dtau, "calls_per_window": inner,
            "us_per_call": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in us.items()},
            "us_per_heun_step": med["heun"] / NHEUN, "us_per_single_euler_launch": med["euler1"] / (2 * NHEUN),
            "us_per_fused_euler_step": med["fused"] / (2 * NHEUN),
            "heun_over_euler1": med["heun"] / med["euler1"],
            "heun_over_euler1_range": [min(h / e for h, e in zip(us["heun"], us["euler1"])),
                                       max(h / e for h, e in zip(us["heun"], us["euler1"]))],
            "yardstick": 1.20, "yardstick_met": med["heun"] / med["euler1"] <= 1.20,
            "heun_over_fused": med["heun"] / med["fused"],
        }
    print(json.dumps(out), flush=True)
    return out


def free_phi2(shape, dtau, m2):
    """The stationary <phi^2> of the free lattice with C = 1: (Euler, Heun, continuum), exact per momentum."""
    tot = [0.0, 0.0, 0.0]
    for kx in range(shape[0]):
        for ky in range(shape[1]):
            for kz in range(shape[2]):
                K = m2 + sum(2.0 - 2.0 * math.cos(2.0 * math.pi * k / n) for k, n in zip((kx, ky, kz), shape))
                a = 1.0 - dtau * K + 0.5 * (dtau * K) ** 2
                tot[0] += 1.0 / (K * (1.0 - 0.5 * dtau * K))
                tot[1] += 2.0 * dtau * (1.0 - 0.5 * dtau * K) ** 2 / (1.0 - a * a)
                tot[2] += 1.0 / K
    V = shape[0] * shape[1] * shape[2]
    return [t / V for t in tot]


def bias(n):
    import numpy as np
    from stochquant_amd import Phi4Lattice
    shape, V, b = (n, n, n), n ** 3, BIAS
    exact = dict(zip(("euler", "heun", "continuum"), free_phi2(shape, b["dtau"], b["m2"])))
    got = {}
    for scheme in ("euler", "heun"):
        with Phi4Lattice(shape, dtau=b["dtau"], m2=b["m2"], lam=0.0, C=1.0, seed=4321) as L:
            L.init_field(0.4)
            L.step(b["therm"], scheme=scheme)
            if scheme == "heun":
                s2 = L.step(b["every"] * b["nmeas"], scheme="heun", every=b["every"])[:, 1]
            else:
                s2 = []
                for _ in range(b["nmeas"]):
                    L.step(b["every"])
                    s2.append(L.measure()["sums"][1])
            v = np.asarray(s2) / V
            got[scheme] = {"phi2": float(v.mean()), "stderr": float(v.std(ddof=1) / math.sqrt(len(v))),
                           "exact_for_scheme": exact[scheme],
                           "bias_against_continuum": float(v.mean()) / exact["continuum"] - 1.0}
    out = {"shape": list(shape), **b, "continuum": exact["continuum"], **got}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="64,256,512")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bias", type=int, default=64)
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    from stochquant_amd import _lib
    if _lib.device_count() < 1:
        raise SystemExit("no HIP device: this benchmark measures on the GPU only")
    res = [bench_shape(int(s), a.reps) for s in a.shapes.split(",") if s]
    doc = {"reps": a.reps, "params": PARAMS, "results": res}
    if a.bias:
        doc["bias"] = bias(a.bias)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
