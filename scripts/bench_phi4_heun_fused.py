"""Cost of the single φ⁴ lattice's one-launch Heun step (Phi4Lattice.step(n, scheme="heun", fused=True)), GPU only.

    python scripts/bench_phi4_heun_fused.py [--shapes 256,512] [--reps 5] [--out FILE]

Per shape L³ (shapes the fused step does not serve are skipped and listed): 200 Euler steps, then `reps` rounds
after a warm-up round of these calls, interleaved in one process, each ended by a device synchronise (a window
repeats its call until it holds about 0.25 s of work), medians and min / max:

  fused     step(200, scheme="heun", fused=True)   200 launches of phi4_heun_tb_kernel
  heun      step(200, scheme="heun")               200 two-launch Heun steps: the path the fused step replaces
  euler2    200 x step(2), one sync                200 launches of the fused Euler two-step kernel: the same 8 B
                                                   per site with two noise evaluations where fused has one

Reported: µs per fused Heun step, per two-launch Heun step and per Euler two-step launch; fused / heun (the number
that must fall below 1); fused / euler2 beside the spread of euler2 against itself over the rounds (max / min);
the yardstick is met when fused / euler2 is at most that spread.  The bits of the two Heun paths are compared at
every size timed.  Writes profiles/r07/phi4_heun_fused/bench.json.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r07", "phi4_heun_fused", "bench.json")
PARAMS = dict(m2=0.5, lam=1.0, C=1.0)
DTAU0 = {64: 0.0016, 256: 0.0004, 512: 0.00018}
NSTEP = 200
WINDOW_S = 0.25


def timed(L, fn, inner):
    L.sync()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    L.sync()
    return (time.perf_counter() - t0) / inner


def same_result(n):
    """Three steps of each Heun path from one start: the fields' bits."""
    import numpy as np
    from stochquant_amd import Phi4Lattice
    got = []
    for fused in (False, True):
        with Phi4Lattice((n, n, n), dtau=DTAU0.get(n, 0.1 / n ** 1.5), seed=1234, **PARAMS) as L:
            L.init_field(0.5)
            L.step(3, scheme="heun", fused=fused)
            got.append(L.download())
    return bool(np.array_equal(got[0].view(np.uint32), got[1].view(np.uint32)))


def bench_shape(n, reps):
    from stochquant_amd import Phi4Lattice
    with Phi4Lattice((n, n, n), dtau=DTAU0.get(n, 0.1 / n ** 1.5), seed=1234, **PARAMS) as L:
        L.init_field(0.5)
        L.step(200)

        def euler2():
            for _ in range(NSTEP):
                L.step(2)

        calls = {"fused": lambda: L.step(NSTEP, scheme="heun", fused=True), "heun": lambda: L.step(NSTEP, scheme="heun"),
                 "euler2": euler2}
        inner = {k: max(1, int(WINDOW_S / timed(L, fn, 1))) for k, fn in calls.items()}     # also the warm-up round
        us = {k: [] for k in calls}
        for _ in range(reps):
            for k, fn in calls.items():
                us[k].append(timed(L, fn, inner[k]) * 1e6)
        med = {k: statistics.median(v) for k, v in us.items()}
        spread = max(us["euler2"]) / min(us["euler2"])
        ratio = med["fused"] / med["euler2"]
        out = {
            "shape": [n, n, n], "dtau": L.dtau, "calls_per_window": inner,
            "us_per_call": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in us.items()},
            "us_per_fused_heun_step": med["fused"] / NSTEP, "us_per_two_launch_heun_step": med["heun"] / NSTEP,
            "us_per_euler_two_step_launch": med["euler2"] / NSTEP,
            "fused_over_heun": med["fused"] / med["heun"],
            "fused_over_euler2": ratio, "euler2_spread_max_over_min": spread,
            "yardstick": "fused_over_euler2 <= euler2_spread_max_over_min", "yardstick_met": ratio <= spread,
        }
    out["same_bits_as_two_launch"] = same_result(n)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="256,512")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=DEFAULT_OUT)
    a = ap.parse_args()
    from stochquant_amd import Phi4Lattice, _lib
    if _lib.device_count() < 1:
        raise SystemExit("no HIP device: this benchmark measures on the GPU only")
    sizes = [int(s) for s in a.shapes.split(",") if s]
    served = [n for n in sizes if Phi4Lattice.heun_fused_shape_info((n, n, n))["supported"]]
    doc = {"reps": a.reps, "params": PARAMS, "wide_wpe": os.environ.get("SQ_HEUN_TB_WPE", "1"),
           "not_served": [n for n in sizes if n not in served], "results": [bench_shape(n, a.reps) for n in served]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
