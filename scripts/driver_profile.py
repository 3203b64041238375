"""Summarise rocprofv3 runs of the DRIVER's bench invocation into the record
bench.py's roofline reads (profiles/r0N/driver_profile.json: r05, r06).

Inputs (one rocprofv3 run each, all of `python3 bench.py --steps 20 --warmup 5 --full`,
MI355X_MICROARCH.md §rocprofv3: counters in passes of their own):
  --trace DIR   --kernel-trace --stats  (per-dispatch durations + the stats CSV)
  --fetch DIR   --pmc FETCH_SIZE
  --write DIR   --pmc WRITE_SIZE
  --sq DIR      --pmc SQ_WAVES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAVE_CYCLES ...

For each lattice of the invocation (256^3 = C2, 512^3 = C3) the dominant
kernel is the two-step fused kernel; its launches are told apart by kernel
name and grid size (the hot instance of each lattice, SIZES below).  The
record carries the library's build id (sq_build_id: the hash of the φ⁴
kernels' code object), so bench.py uses it only for that binary.  Per launch:
  * rocprof_avg_us / rocprof_median_us: dispatch durations from the trace
    (every launch of that kernel and grid in the run: settle, warm-up, timed,
    roofline pass);
  * hbm_bytes_per_launch: FETCH_SIZE x 2 (gfx950: wide streaming reads are
    counted at half their bytes) + WRITE_SIZE, KiB x 1024, medians;
  * valu_busy_cycles_per_launch: SQ_ACTIVE_INST_VALU x 4 (quad-cycles), the
    VALU-issue cycles of all waves, median;
  * valu_util_simd = valu_busy_cycles / (1024 SIMDs x 2.4 GHz x rocprof_avg_us):
    the physical roofline fraction bench.py reports as `frac` (its live launch
    time in place of rocprof_avg_us).

    python scripts/driver_profile.py --trace D --fetch D --write D --sq D --out profiles/r06/driver_profile.json
"""
import argparse
import csv
import glob
import json
import os
import statistics

N_SIMD = 1024
CLOCK_MHZ = 2400.0
# the hot instance of each lattice: (template instance, grid in threads or None = its most launched grid)
SIZES = {256: ("phi4_tb2_kernel<true, false, 1, false, true, false>", 512 * 640),
         512: ("phi4_tb2p_kernel<true, true, 6, false, true>", None)}


def _rows(d, pat):
    files = glob.glob(os.path.join(d, "**", pat), recursive=True)
    if not files:
        raise SystemExit(f"no {pat} under {d}")
    for f in files:
        with open(f) as fh:
            yield from csv.DictReader(fh)


def fused_groups(trace_dir):
    """{(kernel, grid): [durations us]} of the fused step kernels in the trace."""
    g = {}
    for r in _rows(trace_dir, "*kernel_trace.csv"):
        k = r["Kernel_Name"]
        if "phi4_tb2" not in k:
            continue
        grid = int(r["Grid_Size_X"]) * int(r["Grid_Size_Y"]) * int(r["Grid_Size_Z"])
        g.setdefault((k, grid), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    return g


def counters(d, kernel, grid):
    vals = {}
    for r in _rows(d, "*counter_collection.csv"):
        if r["Kernel_Name"] == kernel and int(r["Grid_Size"]) == grid:
            vals.setdefault(r["Counter_Name"], []).append(float(r["Counter_Value"]))
            vals.setdefault("_dur_" + r["Counter_Name"], []).append(
                (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    return {k: statistics.median(v[len(v) // 5:] if len(v) >= 10 else v) for k, v in vals.items()}, \
        {k: len(v) for k, v in vals.items() if not k.startswith("_")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", required=True)
    ap.add_argument("--fetch", required=True)
    ap.add_argument("--write", required=True)
    ap.add_argument("--sq", required=True)
    ap.add_argument("--command", default="python3 bench.py --steps 20 --warmup 5 --full")
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    groups = fused_groups(a.trace)
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from stochquant_amd import _lib
    bid = _lib.build_id()
    out = {"command": a.command, "method": __doc__.split("\n\n")[2].strip(), "build_id": bid, "configs": {}}
    picked = {}
    for size, (inst, g0) in SIZES.items():
        cand = [(k, grid, durs) for (k, grid), durs in groups.items()
                if "::" + inst + "(" in k and (g0 is None or grid == g0)]
        if cand:
            picked[size] = max(cand, key=lambda c: len(c[2]))
    for size, (k, grid, durs) in sorted(picked.items()):
        f, nf = counters(a.fetch, k, grid)
        w, nw = counters(a.write, k, grid)
        s, ns = counters(a.sq, k, grid)
        avg = statistics.fmean(durs)
        med = statistics.median(durs)
        rec = {"kernel": k, "grid": grid, "build_id_phi4": bid.get("phi4"), "launches_in_trace": len(durs),
               "rocprof_avg_us": round(avg, 3), "rocprof_median_us": round(med, 3),
               "rocprof_min_us": round(min(durs), 3), "sites": size ** 3, "steps_per_launch": 2,
               "algorithmic_bytes_per_launch": 8 * size ** 3 * 2, "hbm_min_bytes_per_launch": 8 * size ** 3}
        if "FETCH_SIZE" in f and "WRITE_SIZE" in w:
            rd, wr = 2.0 * f["FETCH_SIZE"] * 1024, w["WRITE_SIZE"] * 1024
            rec.update({"FETCH_SIZE_KiB_median": f["FETCH_SIZE"], "WRITE_SIZE_KiB_median": w["WRITE_SIZE"],
                        "read_bytes_per_launch": rd, "write_bytes_per_launch": wr,
                        "hbm_bytes_per_launch": rd + wr, "traffic_over_hbm_min": (rd + wr) / (8 * size ** 3),
                        "pmc_launches": {"FETCH_SIZE": nf.get("FETCH_SIZE"), "WRITE_SIZE": nw.get("WRITE_SIZE")},
                        "hbm_frac_real_at_rocprof_avg": round((rd + wr) / (avg * 1e-6) / 8e12, 4)})
        if "SQ_ACTIVE_INST_VALU" in s:
            cyc = 4.0 * s["SQ_ACTIVE_INST_VALU"]
            rec.update({"SQ_ACTIVE_INST_VALU": s["SQ_ACTIVE_INST_VALU"], "SQ_INSTS_VALU": s.get("SQ_INSTS_VALU"),
                        "SQ_WAVES": s.get("SQ_WAVES"), "SQ_WAVE_CYCLES": s.get("SQ_WAVE_CYCLES"),
                        "valu_busy_cycles_per_launch": cyc,
                        "valu_insts_per_wave": (s["SQ_INSTS_VALU"] / s["SQ_WAVES"]) if s.get("SQ_WAVES") else None,
                        "pmc_sq_kernel_us": round(s["_dur_SQ_ACTIVE_INST_VALU"], 3),
                        "valu_util_simd_at_rocprof_avg": round(cyc / (N_SIMD * CLOCK_MHZ * avg), 4),
                        "valu_util_simd_at_pmc_run": round(cyc / (N_SIMD * CLOCK_MHZ * s["_dur_SQ_ACTIVE_INST_VALU"]), 4)})
            if s.get("SQ_WAVE_CYCLES"):
                rec["avg_resident_waves_per_simd"] = round(4.0 * s["SQ_WAVE_CYCLES"] / (N_SIMD * CLOCK_MHZ * avg), 2)
            for c in ("SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY"):
                if c in s and s.get("SQ_WAVE_CYCLES"):
                    rec[c + "/WAVE_CYCLES"] = round(s[c] / s["SQ_WAVE_CYCLES"], 4)
        out["configs"][str(size)] = rec
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
