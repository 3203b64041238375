"""Records reference_launches.json and reference_cli.json from the reference's
own compiled code (oracle/_ref/, built by oracle/ref/Makefile from the
reference's unmodified sources).  Run by hand where those binaries exist:

    python tests/golden/make_reference_sweep.py

Both files are data only: inputs, and what the reference's binaries gave.
tests/test_reference_parity.py regenerates them in memory and compares.
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import oracle  # noqa: E402
import reference_cases as rc  # noqa: E402

LAUNCH_SEED = 20260421
TARGET_CASES = 60
PER_SIZE = 2          # cases per (N, potID) at the least


def ref_random(seed, gid):
    import ctypes
    s = ctypes.c_uint64(seed)
    xi = oracle.ref_lib().cl_random(ctypes.byref(s), gid)
    return xi, s.value


def record_launch(case):
    """The reference's outputs of one launch, with the derived figures."""
    out = oracle.ref_launch(case)
    out["calls"], out["omega_free"] = rc.derived(case, out["seed"], ref_random, oracle.ref_lib().k_intConst)
    return out


def build_launches():
    """About TARGET_CASES launches at the fixture's sizes, picked from a fixed
    random sequence: a candidate is kept while it adds to a class or a size
    that is still short, then the rest is filled size by size."""
    rng = np.random.default_rng(LAUNCH_SEED)
    need = {s: rc.QUOTA for s in rc.required_slots()}
    size_need = {(n, p): PER_SIZE for n in rc.FIXTURE_N for p in (0, 3)}
    picked = []
    for _ in range(200_000):
        if len(picked) >= TARGET_CASES and not any(need.values()) and not any(size_need.values()):
            break
        case = rc.draw_launch(rng, sizes=rc.FIXTURE_N)
        out = record_launch(case)
        slots = [(k, case["pot"]) for k in rc.classes_of(case, out) if need.get((k, case["pot"]), 0) > 0]
        # the common classes fill by themselves: only a rare one, or a short size, earns a place
        rare = [s for s in slots if s[0] not in ("stable", "c0", "runs_carried")]
        size_key = (case["N"], case["pot"])
        rare_left = any(n > 0 for (k, _), n in need.items() if k not in ("stable", "c0", "runs_carried"))
        nothing_left = not any(need.values()) and not any(size_need.values())
        if not (rare or size_need[size_key] > 0 or (slots and not rare_left) or nothing_left):
            continue
        picked.append((case, out))
        for s in slots:
            need[s] -= 1
        size_need[size_key] = max(0, size_need[size_key] - 1)
    entries = [rc.encode_launch(c, o) for c, o in picked]
    counts = rc.tally([rc.decode_launch(e) for e in entries])
    return entries, counts


def cli_plan():
    """(name, argv, start_from) of every recorded run, in running order."""
    A = rc.cli_argv
    plan = [
        # the three runs of reference_outputs.json, and its resume
        ("appendix_c", ["4", "0.5", "0.01", "2", "0", "1", "2", "1", "0", "5", "0", "END", "12"], None),
        ("dw_all_unstable", ["200", "0.02", "0.002", "3", "3", "1", "2", "1", "0", "10", "0", "END", "40"], None),
        ("dw_stable", ["200", "0.1", "0.002", "5", "3", "1", "2", "1", "0", "200", "0", "END", "40"], None),
        ("dw_stable_resume", ["200", "0.1", "0.002", "5", "3", "1", "2", "1", "0", "200", "START", "END", "40"],
         "dw_stable"),
    ]
    chains = [
        ("n2_pot0", A(2, 0.5, 0.01, 4, 0, 1, 0, 1, 1, 12), 2),
        ("n2_pot3_c0", A(2, 0.1, 0.002, 5, 3, 0, 2, 3, 10, 20), 1),
        ("n3_pot3", A(3, 0.5, 0.05, 6, 3, 1, 0, 1, 10, 40), 2),
        ("n3_pot0_unstable", A(3, 0.1, 0.05, 7, 0, 1, 2, 3, 10, 12), 1),
        ("n4_pot3_dtau_grows", A(4, 0.5, 0.01, 25, 3, 1, 0, 3, 10, 20), 1),
        ("n5_pot3_mixed", A(5, 0.1, 0.01, 30, 3, 1, 2, 1, 10, 12), 2),
        ("n5_pot0_c0_loops1", A(5, 0.5, 0.05, 14, 0, 0, 0, 1, 1, 40), 0),
        ("n10_pot0_unstable", A(10, 0.1, 0.05, 12, 0, 1, 0, 3, 10, 20), 1),
        ("n10_pot3_loops200", A(10, 0.5, 0.02, 3, 3, 1, 2, 1, 200, 12), 0),
        ("n100_pot3", A(100, 0.1, 0.002, 3, 3, 1, 2, 1, 200, 20), 1),
        ("n100_pot0_c0_mixed", A(100, 0.02, 0.0004, 6, 0, 0, 0, 3, 10, 12), 0),
        ("n200_pot0_mixed", A(200, 0.1, 0.01, 6, 0, 1, 0, 3, 10, 12), 1),
    ]
    for name, argv, resumes in chains:
        plan.append((name, argv, None))
        prev = name
        for k in range(resumes):
            nxt = f"{name}_resume{k + 1}"
            plan.append((nxt, rc.resume_of(argv), prev))
            prev = nxt
    # error paths.  One argument too many is ignored by the reference; one too
    # few makes it read past argv (it dies of a signal), recorded as it is.
    plan.append(("one_argument_too_many", A(4, 0.5, 0.01, 2, 0, 1, 0, 1, 5, 12) + ["extra"], None))
    plan.append(("one_argument_too_few", A(4, 0.5, 0.01, 2, 0, 1, 0, 1, 5, 12)[:-1], None))
    plan.append(("missing_start_file", rc.resume_of(A(4, 0.5, 0.01, 2, 0, 1, 0, 1, 5, 12)), None))
    return plan


def check_survey_records(raw):
    """The three runs recorded during the survey must come out as committed."""
    g = json.load(open(os.path.join(HERE, "reference_outputs.json")))
    out, end = raw["appendix_c"][1].decode(), raw["appendix_c"][2].decode()
    a = g["appendix_c_end_file"]
    assert out.split("\n")[0] == a["stdout_first_line"] and out.split("\n")[1].startswith(a["stdout_second_line_prefix"])
    assert end.split("\n")[0] == a["first_line"] and end.split("\n")[4:7] == a["trailer"]
    out, end = raw["dw_all_unstable"][1].decode(), raw["dw_all_unstable"][2].decode()
    u = g["double_well_all_unstable"]
    assert [ln.split("|")[-2].strip() for ln in out.strip().split("\n")] == u["printed_dtau"]
    tail = end.strip().split("\n")[-3:]
    assert abs(float(tail[2].split("|")[0]) / u["end_dtau"] - 1) < 1e-6 and int(tail[1].split("|")[0]) == u["end_N"]
    n_of = lambda name: int(raw[name][2].decode().strip().split("\n")[-2].split("|")[0])
    assert n_of("dw_stable") == g["double_well_stable"]["end_N"]
    assert n_of("dw_stable_resume") == g["resume_double_count"]["resume_end_N"]


def build_cli():
    plan = [dict(name=n, argv=a, start_from=s) for n, a, s in cli_plan()]
    with tempfile.TemporaryDirectory() as root:
        raw = rc.replay_cli(oracle.ref_tauhost, plan, root, terminate=True)
    check_survey_records(raw)
    entries = []
    for e in plan:
        status, out, end = raw[e["name"]]
        entries.append(dict(e, status=status, stdout=rc.blob(out), end=rc.blob(end)))
    return entries


def dump(obj):
    return json.dumps(obj, separators=(",", ":")).replace('},{"', '},\n{"') + "\n"


def main():
    if not oracle.ref_available():
        sys.exit("oracle/_ref/ is not built: python -m stochquant_amd.build where the reference's sources exist")
    launches, counts = build_launches()
    print(f"{len(launches)} launches; cases per (class, potID):")
    for (k, p), n in sorted(counts.items()):
        print(f"  {k:15s} potID {p}: {n}")
    short = [s for s, n in counts.items() if n < rc.QUOTA]
    if short:
        sys.exit(f"refusing to write: short classes {short}")
    cli = build_cli()
    print(f"{len(cli)} tauhost runs")
    for name, obj in (("reference_launches.json", launches), ("reference_cli.json", cli)):
        text = dump(obj)
        with open(os.path.join(HERE, name), "w") as fh:
            fh.write(text)
        print(f"{name}: {len(text)} bytes")


if __name__ == "__main__":
    main()
