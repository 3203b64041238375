"""Cost and use of the φ⁴ ensemble's replica exchange (Phi4Ensemble.exchange,
Phi4Ensemble.step_hmc_exchange), GPU only.

    python scripts/bench_phi4_ens_exchange.py [--reps 5] [--out FILE] [--no-tunnel]
                                              [--parent-lib OTHER/libstochquant.so] [--pairs 5]

One child process under `timeout` (this process never opens the GPU) times, at
32³ R = 256, 16³ R = 1024 and 8³ R = 4096 with ladders of 8 rungs, from fields
thermalised by 1000 Euler steps and 200 rounds of trajectories with exchange,
interleaved round by round (`reps` rounds after a warm-up round, medians):

  round     exchange(200) / 200
  moments   one moments() call over all R                  } the yardstick:
  copy      one device-to-device copy of R x sites floats  } round <= 1.15 (moments + copy)
  fused     step_hmc_exchange(50, ntraj=2, nleap=10)
  separate  step_hmc(100, nleap=10), then exchange(50)     fused <= 1.10 separate
  loop      50 x [step_hmc(2, nleap=10), exchange(1)]: the calls `fused` replaces
  host      per round step_hmc(2, nleap=10), download(), the decision in NumPy
            from the fields' sums, upload(): HOST_ROUNDS rounds, per round

The ladder is geometric, C_i = g^i; g starts at exp(0.765 / sqrt(V)), where the
free field's links accept 0.45, and one pilot rescales ln g towards a link
acceptance of 0.4.  Δτ is bench_phi4_ens_hmc.py's tuned value of the shape.

A second child (skipped with --no-tunnel) measures what the exchange buys, in
the broken phase on 8³: 16 ladders of 16 rungs, C from 1 to 1.6, λ = 1.  m² is
the first of a descending list at which plain step_hmc shows no sign change of
Σφ on any coldest rung in 20,000 trajectories while every hottest rung changes
sign at least 50 times.  Then, for equal trajectory counts, the sign changes of
Σφ on the coldest rungs, the walkers' round trips per 1000 rounds and the wall
time, with and without exchange.

--parent-lib: the existing calls must not move.  step(200) with the Euler, Heun,
MALA and HMC (nleap = 10) schemes and run_frames(50) at 32³ R = 256 with this
build and with another build of the library (SQ_LIB), in interleaved rounds of
child processes, the other build first and then twice in a row as well.
Writes profiles/r07/phi4_ens_exchange/bench.json.
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
DEFAULT_OUT = os.path.join(ROOT, "profiles", "r07", "phi4_ens_exchange", "bench.json")
# shape, replicas, dtau (bench_phi4_ens_hmc.py: acceptance 0.75 at nleap = 10)
CASES = [((32, 32, 32), 256, 0.00106), ((16, 16, 16), 1024, 0.00657), ((8, 8, 8), 4096, 0.0101)]
PARAMS = dict(m2=0.5, lam=1.0)
NLAD = 8
NLEAP = 10
THERMALISE = 1000
ROUNDS = 200
HOST_ROUNDS = 10
FRAMES = 50
TARGET = 0.4
TUNNEL = dict(shape=(8, 8, 8), nlad=16, ladders=16, c_hot=1.6, lam=1.0, dtau=0.008, ntraj=20000,
              m2_list=(-0.3, -0.45, -0.6, -0.8, -1.0, -1.3))


def _timed(fn):
    t0 = time.perf_counter()
    fn()          # every call ends in a stream synchronise
    return (time.perf_counter() - t0) * 1e3


def _spread(acc):
    """s with erfc(s / (2 sqrt 2)) = acc: the spread of a Gaussian Δ of mean s² / 2 accepted at that rate."""
    lo, hi = 0.0, 20.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if math.erfc(mid / (2.0 * math.sqrt(2.0))) > acc else (lo, mid)
    return 0.5 * (lo + hi)


def _ladder(g, nlad, R):
    return [g ** (r % nlad) for r in range(R)]


def _link_acceptance(e, nlad):
    import numpy as np
    st = e.exchange_stats().reshape(-1, nlad, 2)[:, :nlad - 1].sum(axis=0)
    return (st[:, 1] / np.maximum(st[:, 0], 1)).tolist()


def _host_round(e, recs, seeds, oracle_uniform):
    """One exchange round decided on the host: download, the sums and Δ in NumPy, upload."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import phi4_exchange_model as xm
    phi = e.download()
    f = phi.astype(np.float64)
    s2 = (f * f).sum(axis=(1, 2, 3))
    s4 = (f ** 4).sum(axis=(1, 2, 3))
    nn = sum((f * np.roll(f, -1, axis=a)).sum(axis=(1, 2, 3)) for a in (1, 2, 3))
    x = e.exchange_round
    for a, b in xm.pairs(e.R, e.ladder, x):
        d, _ = xm.delta(recs[a], recs[b], (0.0, s2[a], s4[a], nn[a]), (0.0, s2[b], s4[b], nn[b]))
        if xm.verdict(d, oracle_uniform(seeds[a], x)):
            phi[[a, b]] = phi[[b, a]]
    e.upload(phi)
    e.exchange_round = x + 1


def worker(reps):
    import numpy as np
    import torch
    from stochquant_amd import Phi4Ensemble, _lib
    rng = np.random.default_rng(1)
    for shape, R, dtau in CASES:
        V = shape[0] * shape[1] * shape[2]
        g = math.exp(0.765 / math.sqrt(V))
        seeds = [7 + r for r in range(R)]
        with Phi4Ensemble(shape, R, seeds=seeds, dtau=dtau, C=_ladder(g, NLAD, R), **PARAMS) as e:
            e.set_ladder(NLAD)
            e.init_field(0.5)
            e.step(THERMALISE)
            pilots = []
            for _ in range(2):
                e.step_hmc_exchange(ROUNDS, ntraj=2, nleap=NLEAP)
                e.exchange_reset()
                e.step_hmc_exchange(ROUNDS, ntraj=2, nleap=NLEAP)
                acc = _link_acceptance(e, NLAD)
                pilots.append([round(g, 6), [round(a, 3) for a in acc]])
                mean = min(max(statistics.mean(acc), 0.02), 0.98)
                if 0.3 <= mean <= 0.5:
                    break
                g = math.exp(math.log(g) * _spread(TARGET) / _spread(mean))
                e.set_params(C=_ladder(g, NLAD, R))
            e.exchange_reset()
            e.hmc_reset()
            a = torch.zeros(R * V, dtype=torch.float32, device="cuda")
            b = torch.empty_like(a)

            def copy():
                for _ in range(ROUNDS):
                    b.copy_(a)
                torch.cuda.synchronize()

            def moments():
                for _ in range(20):
                    e.moments()

            def separate():
                e.step_hmc(100, nleap=NLEAP)
                e.exchange(50)

            def loop():
                for _ in range(50):
                    e.step_hmc(2, nleap=NLEAP)
                    e.exchange(1)

            p = e.get_params()
            recs = [(float(np.float32(p["dtau"][r])), float(np.float32(p["m2"][r])),
                     float(np.float32(float(np.float32(p["lam"][r])) / 6.0)),
                     float(np.float32(math.sqrt(2.0 * float(np.float32(p["dtau"][r]))) * p["C"][r]))) for r in range(R)]
            uni = {}

            def uniform(seed, x):      # any uniform will do for the timing: the oracle's Philox is not on this path
                return uni.setdefault((seed, x), float(rng.random()))

            def host():
                for _ in range(HOST_ROUNDS):
                    e.step_hmc(2, nleap=NLEAP)
                    _host_round(e, recs, seeds, uniform)

            calls = {"round": lambda: e.exchange(ROUNDS), "moments": moments, "copy": copy,
                     "fused": lambda: e.step_hmc_exchange(50, ntraj=2, nleap=NLEAP), "separate": separate,
                     "loop": loop}
            per = {"round": ROUNDS, "moments": 20, "copy": ROUNDS, "fused": 50, "separate": 50, "loop": 50,
                   "host": HOST_ROUNDS}
            ts = {k: [] for k in list(calls) + ["host"]}
            for rnd in range(reps + 1):
                for k, fn in calls.items():
                    t = _timed(fn)
                    if rnd:
                        ts[k].append(t)
            acc = _link_acceptance(e, NLAD)
            hs = e.hmc_stats()
            for rnd in range(2):      # the host route last: it leaves the labels behind
                t = _timed(host)
                if rnd:
                    ts["host"].append(t)
            flagged = int(e.flags().sum())
            info = Phi4Ensemble.exchange_shape_info(shape)
        us = {k: statistics.median(v) / per[k] * 1e3 for k, v in ts.items()}
        yard = us["moments"] + us["copy"]
        rec = {"kind": "exchange_cost", "shape": list(shape), "R": R, "nlad": NLAD, "dtau": dtau,
               "ladder_ratio": round(g, 6), "ladder_C": [round(g ** i, 5) for i in range(NLAD)], "ladder_pilots": pilots,
               "link_acceptance": [round(a, 4) for a in acc],
               "hmc_acceptance": round(float(hs[:, 1].sum() / max(hs[:, 0].sum(), 1)), 4),
               "K": info["K"], "T": info["T"], "lds_bytes": info["lds_bytes"],
               "ms_all": {k: [round(t, 4) for t in v] for k, v in ts.items()}, "calls_per_timing": per,
               "us": {k: round(v, 3) for k, v in us.items()},
               "yardstick_us": round(yard, 3), "round_over_yardstick": round(us["round"] / yard, 4),
               "round_yardstick_met": bool(us["round"] <= 1.15 * yard),
               "fused_over_separate": round(us["fused"] / us["separate"], 4),
               "fused_yardstick_met": bool(us["fused"] <= 1.10 * us["separate"]),
               "loop_over_fused": round(us["loop"] / us["fused"], 4),
               "host_over_fused": round(us["host"] / us["fused"], 2),
               "field_bytes": 4 * R * V, "round_bandwidth_GBps_read": round(4 * R * V * (NLAD - 1) / NLAD
                                                                            / (us["round"] * 1e-6) / 1e9, 1),
               "guard_flags_set": flagged, "build_id": _lib.build_id()}
        print(json.dumps(rec), flush=True)


def _sign_changes(s1):
    """Sign changes along axis 0 of the series s1[n][k], per column."""
    import numpy as np
    s = np.sign(s1)
    return (s[1:] * s[:-1] < 0).sum(axis=0)


def _round_trips(rungs, top):
    """Completed trips rung 0 -> top -> 0 in the series rungs[n][walkers]."""
    import numpy as np
    trips = np.zeros(rungs.shape[1], dtype=np.int64)
    phase = np.zeros(rungs.shape[1], dtype=np.int8)      # 0: wait for rung 0, 1: left it, on the way up, 2: down
    for row in rungs:
        phase[(phase == 0) & (row == 0)] = 1
        phase[(phase == 1) & (row == top)] = 2
        done = (phase == 2) & (row == 0)
        trips[done] += 1
        phase[done] = 1
    return trips


def tunnel_worker():
    import numpy as np
    from stochquant_amd import Phi4Ensemble, _lib
    T = TUNNEL
    nlad, NL, ntraj = T["nlad"], T["ladders"], T["ntraj"]
    R = nlad * NL
    g = T["c_hot"] ** (1.0 / (nlad - 1))
    cold, hot = np.arange(NL) * nlad, np.arange(NL) * nlad + nlad - 1
    chunk = 2000

    def fresh(m2):
        e = Phi4Ensemble(T["shape"], R, seed=23, dtau=T["dtau"], m2=m2, lam=T["lam"], C=_ladder(g, nlad, R))
        e.init_field(0.5)
        e.step(THERMALISE)
        e.step_hmc(500, nleap=NLEAP, randomize=True)
        return e

    def plain(e):
        parts = []
        t0 = time.perf_counter()
        for _ in range(ntraj // chunk):
            parts.append(e.step_hmc(chunk, nleap=NLEAP, randomize=True, every=1)[:, :, 0].copy())
        return np.concatenate(parts), time.perf_counter() - t0

    scan, chosen = [], None
    for m2 in T["m2_list"]:
        with fresh(m2) as e:
            s1, _ = plain(e)
        ch = _sign_changes(s1)
        scan.append({"m2": m2, "cold_sign_changes": int(ch[cold].sum()), "hot_sign_changes_min": int(ch[hot].min()),
                     "hot_sign_changes_median": float(np.median(ch[hot]))})
        if ch[cold].sum() == 0 and ch[hot].min() >= 50:
            chosen = m2
            break
    out = {"kind": "tunnelling", "shape": list(T["shape"]), "R": R, "nlad": nlad, "ladders": NL, "lam": T["lam"],
           "dtau": T["dtau"], "nleap": NLEAP, "randomize": True, "ladder_C": [round(g ** i, 5) for i in range(nlad)],
           "trajectories": ntraj, "m2_scan": scan, "m2": chosen, "build_id": _lib.build_id()}
    if chosen is not None:
        with fresh(chosen) as e:
            s1, t_plain = plain(e)
            hs = e.hmc_stats().reshape(NL, nlad, 4).sum(axis=0)
        ch = _sign_changes(s1)
        out["plain"] = {"cold_sign_changes": int(ch[cold].sum()), "cold_chains_that_changed_sign": int((ch[cold] > 0).sum()),
                        "hot_sign_changes_median": float(np.median(ch[hot])), "wall_s": round(t_plain, 3),
                        "hmc_acceptance_per_rung": [round(float(a), 3) for a in hs[:, 1] / hs[:, 0]]}
        with fresh(chosen) as e:
            e.set_ladder(nlad)
            e.step_hmc_exchange(500, ntraj=2, nleap=NLEAP, randomize=True)
            e.exchange_reset(walkers=True)
            e.hmc_reset()
            parts, rungs = [], []
            t0 = time.perf_counter()
            for _ in range(ntraj // chunk):
                ser, _, rx = e.step_hmc_exchange(chunk // 2, ntraj=2, nleap=NLEAP, randomize=True, every=1, record=True)
                parts.append(ser[:, :, 0].copy())
                w = rx[:, :, 4].astype(np.int64)                 # label held by each slot after the round
                pos = np.empty_like(w)
                np.put_along_axis(pos, w, np.broadcast_to(np.arange(R) % nlad, w.shape), axis=1)
                rungs.append(pos)                                # rung of every walker after the round
            t_x = time.perf_counter() - t0
            acc = _link_acceptance(e, nlad)
        s1 = np.concatenate(parts)
        ch = _sign_changes(s1)
        trips = _round_trips(np.concatenate(rungs), nlad - 1)
        nrounds = ntraj // 2
        out["exchange"] = {"rounds": nrounds, "ntraj_per_round": 2, "cold_sign_changes": int(ch[cold].sum()),
                           "cold_chains_that_changed_sign": int((ch[cold] > 0).sum()),
                           "hot_sign_changes_median": float(np.median(ch[hot])),
                           "link_acceptance": [round(a, 3) for a in acc],
                           "round_trips_total": int(trips.sum()),
                           "round_trips_per_walker_per_1000_rounds": round(float(trips.mean()) / nrounds * 1e3, 3),
                           "round_trips_per_ladder_per_1000_rounds": round(float(trips.sum()) / NL / nrounds * 1e3, 3),
                           "wall_s": round(t_x, 3)}
        out["wall_ratio_exchange_over_plain"] = round(t_x / t_plain, 3)
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
        print(f"bench_phi4_ens_exchange: a child failed with status {r.returncode}; stopping", file=sys.stderr)
        return None
    return [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="steps per call of the A/B of existing calls")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--parent-lib", default=None, help="another build of libstochquant.so for the A/B of existing calls")
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--no-tunnel", action="store_true", help="skip the broken-phase measurement")
    ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--tunnel-worker", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--raw-worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        worker(a.reps)
        return 0
    if a.tunnel_worker:
        tunnel_worker()
        return 0
    if a.raw_worker:
        raw_worker(a.steps, a.reps)
        return 0
    records = []

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"reps": a.reps, "params": PARAMS, "thermalise": THERMALISE, "nleap": NLEAP,
                       "records": records}, fh, indent=1)
            fh.write("\n")

    got = _child(["--reps", str(a.reps), "--worker"], a.timeout)
    if got is None:
        return 1
    records += got
    save()
    if not a.no_tunnel:
        got = _child(["--tunnel-worker"], a.timeout)
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
