"""Host time of the φ⁴ ensemble's calls, this build against another build of the
library (the parent of a change that touches only the host side), GPU only.

    python scripts/bench_phi4_ens_host_ab.py --parent-lib OTHER/libstochquant.so
                                             [--rounds 5] [--reps 5] [--out FILE]

The kernels being the same, only per-call host time can differ.  Timed, at the
three standard points 32³ R = 256, 16³ R = 1024 and 8³ R = 4096:

  step200   step(200), every = 0               bench_phi4_ens.py's case and parameters
  step1     step(1): the shortest call, where host time is the largest share
  round     exchange(200) / 200                bench_phi4_ens_exchange.py's `round`
  fused_x   step_hmc_exchange(50, ntraj=2, nleap=10) / 50      ... its `fused`
  fused_c   step_hmc_cluster(50, ntraj=1, nleap=10) / 50       bench_phi4_ens_cluster.py's `fused`

with those scripts' Δτ per shape, ladders of 8 rungs in the geometric ladder
they start from, and fields thermalised by 1000 Euler steps.  Each figure is the
median of `reps` calls after a warm-up call, in µs per call (per round for the
last three).

`rounds` interleaved rounds of three child processes, each under `timeout`:
parent, this build, parent again (SQ_LIB selects the parent).  The yardstick is
the parent against itself: for every quantity the median over the rounds of
this / parent has to lie inside [min, max] of parent_again / parent.  The first
failing child ends the run.  Writes profiles/r07/phi4_ens_host_split/ab.json.
"""
import argparse
import json
import math
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r07", "phi4_ens_host_split", "ab.json")
CASES = [((32, 32, 32), 256, 0.00106), ((16, 16, 16), 1024, 0.00657), ((8, 8, 8), 4096, 0.0101)]
NLAD, NLEAP, THERMALISE = 8, 10, 1000


def _median_us(fn, reps, per=1):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()          # every call ends in a stream synchronise
        ts.append((time.perf_counter() - t0) * 1e6 / per)
    return round(statistics.median(ts), 3)


def worker(reps):
    from stochquant_amd import Phi4Ensemble, _lib
    out = {"build_id": _lib.build_id()}
    for shape, R, dtau in CASES:
        tag = f"{shape[0]}^3"
        with Phi4Ensemble(shape, R, seed=7, dtau=0.01, m2=0.5, lam=1.0, C=1.0) as e:
            e.init_field(0.5)
            e.step(200)
            out[f"step200 {tag}"] = _median_us(lambda: e.step(200), reps)
            out[f"step1 {tag}"] = _median_us(lambda: e.step(1), 4 * reps)
        g = math.exp(0.765 / math.sqrt(shape[0] * shape[1] * shape[2]))
        with Phi4Ensemble(shape, R, seeds=[7 + r for r in range(R)], dtau=dtau, m2=0.5, lam=1.0,
                          C=[g ** (r % NLAD) for r in range(R)]) as e:
            e.set_ladder(NLAD)
            e.init_field(0.5)
            e.step(THERMALISE)
            e.step_hmc_exchange(50, ntraj=2, nleap=NLEAP)
            out[f"round {tag}"] = _median_us(lambda: e.exchange(200), reps, 200)
            out[f"fused_x {tag}"] = _median_us(lambda: e.step_hmc_exchange(50, ntraj=2, nleap=NLEAP), reps, 50)
            out[f"fused_c {tag}"] = _median_us(lambda: e.step_hmc_cluster(50, ntraj=1, nleap=NLEAP), reps, 50)
            out[f"flags {tag}"] = int(e.flags().sum())
    print(json.dumps(out), flush=True)


def _child(reps, timeout, env=None):
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__), "--reps", str(reps), "--worker"]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        print(f"bench_phi4_ens_host_ab: a child failed with status {r.returncode}; stopping", file=sys.stderr)
        return None
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None, help="the other build of libstochquant.so")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--timeout", type=int, default=120, help="seconds per child process")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.reps)
        return 0
    if not a.parent_lib:
        ap.error("--parent-lib is required")
    penv = dict(os.environ, SQ_LIB=os.path.abspath(a.parent_lib))
    rounds = []
    for _ in range(a.rounds):
        runs = []
        for env in (penv, None, penv):
            runs.append(_child(a.reps, a.timeout, env))
            if runs[-1] is None:
                return 1
        rounds.append(dict(zip(("parent", "this", "parent_again"), runs)))
    table = {}
    for k in [k for k in rounds[0]["this"] if k != "build_id" and not k.startswith("flags")]:
        ratio = [r["this"][k] / r["parent"][k] for r in rounds]
        self_ = [r["parent_again"][k] / r["parent"][k] for r in rounds]
        med = statistics.median(ratio)
        table[k] = {"parent_us": statistics.median(r["parent"][k] for r in rounds),
                    "this_us": statistics.median(r["this"][k] for r in rounds),
                    "this_over_parent": [round(x, 4) for x in ratio], "median_this_over_parent": round(med, 4),
                    "parent_again_over_parent": [round(x, 4) for x in self_],
                    "parent_spread": [round(min(self_), 4), round(max(self_), 4)],
                    "inside_parent_spread": bool(min(self_) <= med <= max(self_))}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"rounds": a.rounds, "reps": a.reps, "unit": "us per call (round, fused_x, fused_c: per round)",
                   "parent_build_id": rounds[0]["parent"]["build_id"], "this_build_id": rounds[0]["this"]["build_id"],
                   "table": table, "runs": rounds}, fh, indent=1)
        fh.write("\n")
    for k, v in table.items():
        print(f"{k:16s} parent {v['parent_us']:10.2f} this {v['this_us']:10.2f} median ratio "
              f"{v['median_this_over_parent']:.4f} parent spread {v['parent_spread']} "
              f"{'inside' if v['inside_parent_spread'] else 'OUTSIDE'}")
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
