"""Cost of the φ⁴ ensemble's in-kernel momentum-projected correlators
(Phi4Ensemble.step(momenta=True)), GPU only.

    python scripts/bench_phi4_ens_pcorr.py [--steps 200] [--every 20] [--reps 5] [--out FILE]
                                           [--parent-lib OTHER/libstochquant.so] [--pairs 5]

One child process under `timeout` (this process never opens the GPU) times, at
32³ R = 256, 16³ R = 1024 and 8³ R = 4096, six calls, interleaved round by
round (`reps` rounds after a warm-up round, medians per call), on ensembles of
one seed and start field:

  plain       step(steps)
  sums        step(steps, every=every)                   the four-sums measurement
  corr        step(steps, every=every, correlate=True)   the sums and the zero-momentum correlator
  pcorr M     step(steps, every=every, momenta=True)     the sums and M momenta, M = 1, 4, 8

and reports per shape one step, one zero-momentum measurement ((corr - sums) /
measurements) and, per M, one momentum measurement per momentum ((pcorr M -
sums) / (measurements M)) in µs, with the yardstick "one momentum costs no more
than a zero-momentum measurement plus one step", taken against those two
numbers of the same run.  At 32³ R = 256 the same process also runs the loop
the call replaces: step(every), download(), a NumPy projection on the M = 4
momenta and their correlator, steps / every times.

--parent-lib: raw steps must not move.  step(steps) at 32³ R = 256 with this
build and with another build of the library (SQ_LIB), in interleaved pairs of
child processes, the other build first and then twice in a row as well: the
spread of the other build against itself is the allowance.
Writes profiles/r07/phi4_ens_pcorr/bench.json.
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
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r07", "phi4_ens_pcorr", "bench.json")
CASES = [((32, 32, 32), 256), ((16, 16, 16), 1024), ((8, 8, 8), 4096)]
PARAMS = dict(dtau=0.01, m2=0.5, lam=1.0, C=1.0)
MOMENTA = [(1, 0), (0, 1), (1, 1), (2, 1), (0, 0), (2, 0), (0, 2), (3, 1)]
MS = (1, 4, 8)


def _timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def _host_projection(phi, moms):
    """What a user computes from downloaded fields: g[r][m][t] = Σ_z Re S_p(z) conj S_p(z + t), NumPy."""
    import numpy as np
    R, Lz, Ly, Lx = phi.shape
    x, y = np.arange(Lx), np.arange(Ly)
    W = np.stack([np.exp(2j * np.pi * (nx * x[None, :] / Lx + ny * y[:, None] / Ly)) for nx, ny in moms])
    S = np.einsum("rzyx,myx->rmz", phi.astype(np.float64), W)
    return np.stack([np.sum((S * np.conj(np.roll(S, -t, axis=2))).real, axis=2) for t in range(Lz // 2 + 1)], axis=2)


def worker(steps, every, reps):
    from stochquant_amd import Phi4Ensemble, _lib
    nmeas = steps // every
    for shape, R in CASES:
        ens = {k: Phi4Ensemble(shape, R, seed=7, **PARAMS) for k in ("base",) + MS}
        try:
            for k, e in ens.items():
                e.init_field(0.5)
                if k != "base":
                    e.set_momenta(MOMENTA[:k])
            calls = {"plain": lambda: ens["base"].step(steps), "sums": lambda: ens["base"].step(steps, every=every),
                     "corr": lambda: ens["base"].step(steps, every=every, correlate=True)}
            for M in MS:
                calls[f"pcorr{M}"] = (lambda e: lambda: e.step(steps, every=every, momenta=True))(ens[M])
            ts = {k: [] for k in calls}
            for rnd in range(reps + 1):
                for k, fn in calls.items():
                    t = _timed(fn)
                    if rnd:
                        ts[k].append(t)
            flagged = int(sum(e.flags().sum() for e in ens.values()))
            for M in MS:
                assert int(ens[M].pcorr_sums(count=1)[1][0]) == (reps + 1) * nmeas
            med = {k: statistics.median(v) for k, v in ts.items()}
            step_us = med["plain"] / steps * 1e3
            sums_us = (med["sums"] - med["plain"]) / nmeas * 1e3
            corr_us = (med["corr"] - med["sums"]) / nmeas * 1e3
            yard = corr_us + step_us
            rec = {"kind": "ensemble", "shape": list(shape), "R": R, "steps": steps, "every": every,
                   "ms": {k: round(v, 4) for k, v in med.items()},
                   "ms_all": {k: [round(t, 4) for t in v] for k, v in ts.items()},
                   "step_us": round(step_us, 3), "sums_measurement_us": round(sums_us, 3),
                   "corr_measurement_us": round(corr_us, 3),
                   "yardstick_corr_plus_one_step_us": round(yard, 3), "per_momentum": {},
                   "guard_flags_set": flagged, "build_id": _lib.build_id()}
            for M in MS:
                one = (med[f"pcorr{M}"] - med["sums"]) / (nmeas * M) * 1e3
                rec["per_momentum"][str(M)] = {"momentum_measurement_us": round(one, 3),
                                               "in_steps": round(one / step_us, 3),
                                               "over_corr_measurement": round(one / corr_us, 3) if corr_us > 0 else None,
                                               "yardstick_met": bool(one <= yard),
                                               "call_over_plain_percent":
                                                   round((med[f"pcorr{M}"] / med["plain"] - 1.0) * 100.0, 2)}
            if shape == (32, 32, 32):
                e, moms = ens["base"], MOMENTA[:4]

                def loop():
                    for _ in range(nmeas):
                        e.step(every)
                        _host_projection(e.download(), moms)
                loop()
                one = statistics.median(_timed(loop) for _ in range(reps))
                rec["host_loop_M4_ms"] = round(one, 3)
                rec["speedup_over_host_loop_M4"] = round(one / med["pcorr4"], 2)
        finally:
            for e in ens.values():
                e.close()
        print(json.dumps(rec), flush=True)


def raw_worker(steps, reps):
    import ctypes
    from stochquant_amd import Phi4Ensemble, _lib
    # an older build lacks the newer exports, and the raw step needs none of them
    have = ctypes.CDLL(os.environ.get("SQ_LIB", _lib.LIB_PATH))
    for name in [n for n in _lib.SIGNATURES if not hasattr(have, n)]:
        del _lib.SIGNATURES[name]
    with Phi4Ensemble((32, 32, 32), 256, seed=7, **PARAMS) as ens:
        ens.init_field(0.5)
        ens.step(steps)
        ms = statistics.median(_timed(lambda: ens.step(steps)) for _ in range(reps))
    print(json.dumps({"ms": round(ms, 4), "build_id": _lib.build_id()}), flush=True)


def _child(args, timeout, env=None):
    cmd = ["timeout", "-k", "10", str(timeout), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        sys.stderr.write(r.stderr)
        print(f"bench_phi4_ens_pcorr: a child failed with status {r.returncode}; stopping", file=sys.stderr)
        return None
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--every", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--parent-lib", default=None, help="another build of libstochquant.so for the raw-step A/B")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--raw-worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.steps, a.every, a.reps)
        return 0
    if a.raw_worker:
        raw_worker(a.steps, a.reps)
        return 0
    common = ["--steps", str(a.steps), "--every", str(a.every), "--reps", str(a.reps)]
    records = _child(common + ["--worker"], a.timeout)
    if records is None:
        return 1
    for r in records:
        print(json.dumps(r))
    if a.parent_lib:
        penv = dict(os.environ, SQ_LIB=os.path.abspath(a.parent_lib))
        pairs = []
        for _ in range(a.pairs):   # parent, parent again, this build: two differences per round
            runs = [_child(common + ["--raw-worker"], a.timeout, penv)]
            runs.append(_child(common + ["--raw-worker"], a.timeout, penv) if runs[0] is not None else None)
            runs.append(_child(common + ["--raw-worker"], a.timeout) if runs[1] is not None else None)
            if runs[2] is None:
                return 1
            old, old2, new = (r[0] for r in runs)
            pairs.append({"parent_ms": old["ms"], "parent_again_ms": old2["ms"], "this_ms": new["ms"],
                          "diff_percent": round((new["ms"] / old["ms"] - 1.0) * 100.0, 3),
                          "parent_self_diff_percent": round((old2["ms"] / old["ms"] - 1.0) * 100.0, 3)})
        d = [p["diff_percent"] for p in pairs]
        s = [p["parent_self_diff_percent"] for p in pairs]
        ab = {"kind": "raw_steps_vs_parent", "shape": [32, 32, 32], "R": 256, "steps": a.steps, "pairs": pairs,
              "median_diff_percent": round(statistics.median(d), 3), "min_diff_percent": min(d),
              "max_diff_percent": max(d), "parent_self_median_diff_percent": round(statistics.median(s), 3),
              "parent_self_min_diff_percent": min(s), "parent_self_max_diff_percent": max(s),
              "within_parent_spread": bool(statistics.median(d) <= max(abs(x) for x in s)),
              "parent_build_id": old["build_id"], "this_build_id": new["build_id"]}
        print(json.dumps(ab))
        records.append(ab)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"steps_per_call": a.steps, "every": a.every, "reps": a.reps, "params": PARAMS,
                   "momenta": MOMENTA, "records": records}, fh, indent=1)
        fh.write("\n")
    print(f"wrote {a.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
