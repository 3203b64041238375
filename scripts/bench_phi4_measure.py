"""Cost of the single φ⁴ lattice's in-stream measurements (Phi4Lattice.step_hmc(every=...), measure), GPU only.

    python scripts/bench_phi4_measure.py [--shapes 64,256,512] [--reps 5] [--out FILE]

Per shape L³: 200 Euler steps, then `reps` rounds after a warm-up round of these calls, interleaved, each ended by
a device synchronise, medians and min / max per unit:

  hmc1        step_hmc(n, nleap=1)                                  per trajectory
  hmc1_m0     step_hmc(n, nleap=1, every=1, correlate=True)         per trajectory, M = 0: sums + correlator
  hmc1_m4/8   ... momenta=True as well, with 4 / 8 momenta set
  alone       measure()                                             one stand-alone call (one sync, 32 B read back)
  hmc10       step_hmc(50, nleap=10)                                per trajectory
  instream    step_hmc(50, nleap=10, every=1, correlate=True)       per trajectory
  host        50 x { step_hmc(1, nleap=10); moments(); correlator() }  per trajectory: the loop `instream` replaces
  copy        sq_copy_bandwidth of one field (device to device, 8 B per site)

Derived: meas_m0 / m4 / m8 = hmc1_mX - hmc1, one in-stream measurement (the three launches; a difference of two
medians, so small shapes carry the launch gaps of both).  Yardstick: meas_m0 <= 1.25 x copy.  host_over_instream
is the ratio of the two routes; meas_share_of_trajectory = meas_m0 / hmc10.
Writes profiles/r07/phi4_measure/bench.json.
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
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r07", "phi4_measure", "bench.json")
PARAMS = dict(m2=0.5, lam=1.0, C=1.0)
DTAU0 = {64: 0.0016, 256: 0.0004, 512: 0.00018}
MOMENTA = [(1, 0), (0, 1), (1, 1), (2, 1), (0, 2), (2, 0), (3, 1), (1, 3)]
NTRAJ = 50


def timed(L, fn):
    L.sync()
    t0 = time.perf_counter()
    fn()
    L.sync()
    return time.perf_counter() - t0


def bench_shape(n, reps):
    from stochquant_amd import Phi4Lattice, _lib
    with Phi4Lattice((n, n, n), dtau=DTAU0.get(n, 0.1 / n ** 1.5), seed=1234, **PARAMS) as L:
        L.init_field(0.5)
        L.step(200)

        def host_route():
            for _ in range(NTRAJ):
                L.step_hmc(1, nleap=10)
                L.moments()
                L.correlator()

        def with_momenta(k):
            def run():
                L.step_hmc(NTRAJ, nleap=1, every=1, correlate=True, momenta=True)
            return k, run

        calls = {
            "hmc1": (NTRAJ, None, lambda: L.step_hmc(NTRAJ, nleap=1)),
            "hmc1_m0": (NTRAJ, None, lambda: L.step_hmc(NTRAJ, nleap=1, every=1, correlate=True)),
            "hmc1_m4": (NTRAJ,) + with_momenta(4),
            "hmc1_m8": (NTRAJ,) + with_momenta(8),
            "alone": (10, None, lambda: [L.measure() for _ in range(10)]),
            "hmc10": (NTRAJ, None, lambda: L.step_hmc(NTRAJ, nleap=10)),
            "instream": (NTRAJ, None, lambda: L.step_hmc(NTRAJ, nleap=10, every=1, correlate=True)),
            "host": (NTRAJ, None, host_route),
        }
        us = {k: [] for k in list(calls) + ["copy"]}
        for r in range(reps + 1):
            for k, (cnt, nmom, fn) in calls.items():
                if nmom is not None:
                    L.set_momenta(MOMENTA[:nmom])  # outside the timed window
                t = timed(L, fn) / cnt * 1e6
                if r:
                    us[k].append(t)
            g = ctypes.c_double()
            _lib.call("sq_copy_bandwidth", 0, 4 * n ** 3, 20, ctypes.byref(g))
            if r:
                us["copy"].append(2.0 * 4 * n ** 3 / (g.value * 1e9) * 1e6)
        med = {k: statistics.median(v) for k, v in us.items()}
        meas = {k: med["hmc1_" + k] - med["hmc1"] for k in ("m0", "m4", "m8")}
        out = {
            "shape": [n, n, n], "dtau": L.dtau, "info": Phi4Lattice.measure_shape_info((n, n, n), 8),
            "us": {k: {"median": med[k], "min": min(v), "max": max(v)} for k, v in us.items()},
            "us_per_measurement": meas, "yardstick_us": 1.25 * med["copy"], "yardstick_met": meas["m0"] <= 1.25 * med["copy"],
            "meas_over_copy": meas["m0"] / med["copy"], "host_over_instream": med["host"] / med["instream"],
            "meas_share_of_trajectory": meas["m0"] / med["hmc10"],
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
