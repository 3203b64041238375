"""Interleaved A/B of two library builds on the raw fused step, in one job.

Per round and build one fresh process (SQ_LIB picks the library, so each has a
context of its own) times one sq_step(--steps) call by wall clock after a
warm-up call; the order of the builds alternates from round to round.  Prints
every round's us/step, the medians, the base build's round-to-round range
and how many rounds the other build won.

    python scripts/ab_step_libs.py base:path/to/a.so new:path/to/b.so --shape 256x256x256 --rounds 6
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(shape, steps, warmup):
    sys.path.insert(0, ROOT)
    from stochquant_amd import Phi4Lattice
    with Phi4Lattice(shape, dtau=0.01, m2=1.0, lam=1.0, seed=0x5EED) as lat:
        lat.init_field(0.1)
        lat.step(warmup)
        lat.sync()
        t0 = time.perf_counter()
        lat.step(steps)
        lat.sync()
        us = (time.perf_counter() - t0) / steps * 1e6
        print(json.dumps({"us_per_step": us, "kernel": lat.launch_info()["kernel"]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*", help="name:path, the first is the base")
    ap.add_argument("--shape", default="256x256x256")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    shape = tuple(int(v) for v in a.shape.split("x"))
    if a.child:
        return child(shape, a.steps, a.warmup)
    libs = [s.split(":", 1) for s in a.libs]
    res = {n: [] for n, _ in libs}
    for rnd in range(a.rounds):
        order = libs if rnd % 2 == 0 else libs[::-1]
        for name, path in order:
            env = dict(os.environ, SQ_LIB=os.path.abspath(path))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--shape", a.shape, "--steps",
                                str(a.steps), "--warmup", str(a.warmup)], env=env, capture_output=True, text=True,
                               timeout=300)
            if r.returncode != 0:
                sys.exit(f"{name} round {rnd}: exit {r.returncode}\n{r.stdout}{r.stderr}")
            d = json.loads(r.stdout.strip().splitlines()[-1])
            res[name].append(d["us_per_step"])
            print(json.dumps({"shape": a.shape, "round": rnd, "lib": name, "us_per_step": round(d["us_per_step"], 3),
                              "kernel": d["kernel"]}), flush=True)
    base, other = libs[0][0], libs[1][0]
    mb, mo = statistics.median(res[base]), statistics.median(res[other])
    rng = max(res[base]) - min(res[base])
    wins = sum(o < b for b, o in zip(res[base], res[other]))
    print(json.dumps({"shape": a.shape, "steps": a.steps, "rounds": a.rounds, f"median_{base}": round(mb, 3),
                      f"median_{other}": round(mo, 3), f"range_{base}": round(rng, 3),
                      "gain_us": round(mb - mo, 3), "gain_over_range": mb - mo > rng,
                      f"rounds_{other}_faster": wins}))


if __name__ == "__main__":
    main()
