"""Replica-ensemble frame time (Qm1dEnsemble) vs the single chain (Qm1dChain),
timed in the same process with the same warm-up, for the shapes of
scripts/bench_qm1d.py and R in {1, CUs, 4 CUs, 16 CUs}.  GPU only; prints one
JSON line per (shape, R).

    python scripts/bench_qm1d_ens.py [--frames 5] [--cus 256] [--out FILE]

ens_ms_per_frame: run_frame() called `frames` times (one launch and one
read-back per frame, the single chain's protocol); ens_ms_per_frame_batched:
one run_frames(frames) call (frames launches, one read-back).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--cus", type=int, default=256, help="compute units of the device (MI355X: 256)")
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    a = ap.parse_args()
    from stochquant_amd import Qm1dChain, Qm1dEnsemble
    frames = max(5, a.frames)
    # (N, dt, dtau, potID, loops): scripts/bench_qm1d.py's register-kernel shapes
    shapes = [(100, 0.1, 0.002, 3, 1000), (200, 0.1, 0.002, 3, 200), (1000, 0.05, 0.0005, 0, 1000)]
    lines = []
    for N, dt, dtau, pot, loops in shapes:
        f0 = 0.1 * np.random.default_rng(1).standard_normal(N)
        with Qm1dChain(N, dt, dtau, pot=pot, C=1.0, loops=loops) as g:
            g.upload(f0, omega=dt * (N // 2))
            g.run_frame()  # warm-up (allocations, code objects)
            g.sync()
            t0 = time.perf_counter()
            st1 = [g.run_frame() for _ in range(frames)]
            g.sync()
            single_ms = (time.perf_counter() - t0) * 1e3 / frames
        for R in (1, a.cus, 4 * a.cus, 16 * a.cus):
            with Qm1dEnsemble(N, dt, dtau, R, pot=pot, C=1.0, loops=loops) as e:
                e.upload(f0, omega=dt * (N // 2))
                e.run_frame()  # warm-up; every call returns with the stream idle
                t0 = time.perf_counter()
                st = np.stack([e.run_frame() for _ in range(frames)])
                ens_ms = (time.perf_counter() - t0) * 1e3 / frames
                t0 = time.perf_counter()
                stb = e.run_frames(frames)
                ens_b_ms = (time.perf_counter() - t0) * 1e3 / frames
            rec = {"N": N, "loops": loops, "pot": pot, "R": R, "frames": frames,
                   "ens_ms_per_frame": round(ens_ms, 3), "ens_ms_per_frame_batched": round(ens_b_ms, 3),
                   "ens_site_updates_per_s": R * N * loops / ens_ms * 1e3,
                   "ens_site_updates_per_s_batched": R * N * loops / ens_b_ms * 1e3,
                   "single_ms_per_frame": round(single_ms, 3),
                   "ens_over_single": round(ens_ms / single_ms, 3),
                   "stable_fraction": float((st.mean() + stb.mean()) / 2), "single_stable_frames": int(sum(st1))}
            print(json.dumps(rec), flush=True)
            lines.append(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
