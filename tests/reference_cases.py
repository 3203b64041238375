"""Shared by the reference-parity tests and tests/golden/make_reference_sweep.py:
how a time_dev launch and a tauhost run are drawn, stored as data, classified
and compared.  Nothing here runs the product or the reference.

A launch is a dict: N, dt, dtau, pot, C, loops, seed, omega, lrgEl, lrgVl,
runs and the arrays f, x, xx0 (new* start as their copies, as the reference's
host uploads them).  Its record `out` holds every output buffer and scalar of
the reference's own compiled kernel, plus two figures derived from its own
random(): `calls` (the calls of random() the launch made, from the seed it
left) and, for loops = 1, `omega_free` (omega' before the reflection).

Floats are stored as float.hex() strings.  NaNs compare equal whatever their
sign and payload: IEEE 754 leaves those to the implementation, and the hex
form does not keep them.
"""
import functools
import hashlib

import numpy as np

M48 = (1 << 48) - 1
LCG_A, LCG_B = 0x5DEECE66D, 0xB
ARRAYS = ("f", "x", "xx0", "nf", "nx", "nxx0")
FIXTURE_N = (2, 3, 4, 5, 8, 17, 33)


# ---------------------------------------------------------------------------
# Seeds that drive the rare branches of the reference's random()
# (tau_kernel.cl:269-284): the isinf retry (t1 >> 16 == 0, log(0) = -inf) and
# the first arm of the seed update (s < 2^31 and t2 < 2^31 -> s + t2, "case P";
# the common arm is s' = t2 - 2^31, "case Q").
# ---------------------------------------------------------------------------
def lcg_pair(s, g):
    """(t1, t2) of one pass of random() from seed s for work-item g."""
    t1 = ((s + g) * LCG_A + LCG_B) & M48
    return t1, ((t1 + g) * LCG_A + LCG_B) & M48


@functools.lru_cache(maxsize=None)
def case_p_first_call_seeds(count=2):
    """The smallest seeds whose first call (g = 0) takes case P."""
    found = []
    for s in range(1, 3_000_000):
        if lcg_pair(s, 0)[1] < 2 ** 31:
            found.append(s)
            if len(found) == count:
                break
    return tuple(found)


def retry_state(g):
    """A seed from which work-item g's call retries: t1 = 12345, t1 >> 16 == 0."""
    return ((12345 - LCG_B) * pow(LCG_A, -1, 1 << 48) - g) & M48


@functools.lru_cache(maxsize=None)
def case_p_state(g):
    """The smallest seed below 2^31 from which work-item g's call takes case P."""
    return next(s for s in range(1, 1 << 31) if lcg_pair(s, g)[1] < 2 ** 31)


def seed_reaching(s_k, k, N):
    """The seed whose case-Q chain (s' = A^2 s + beta(g)) is s_k before call k
    of a launch with N + 1 work-items: the chain run backwards."""
    alpha = LCG_A * LCG_A & M48
    ainv = pow(alpha, -1, 1 << 48)
    s = s_k
    for j in range(k - 1, -1, -1):
        g = j % (N + 1)
        beta = (LCG_A * LCG_A * g + LCG_A * LCG_B + LCG_A * g + LCG_B - 2 ** 31) & M48
        s = ainv * (s - beta) & M48
    return s


# ---------------------------------------------------------------------------
# Launches
# ---------------------------------------------------------------------------
def draw_launch(rng, sizes=None):
    """One random launch: N in 2..33 (or from `sizes`), potID 0 and 3, C in
    {0, 1, 3}, start amplitudes up to 400, NaN / +-inf sites, omega inside, at
    and outside [0, (N-1) dt], lrgEl / lrgVl carried in, runs up to 1000."""
    N = int(rng.choice(sizes)) if sizes is not None else int(rng.integers(2, 34))
    pot = int(rng.choice([0, 3]))
    C = float(rng.choice([0.0, 1.0, 1.0, 3.0]))
    dt = float(rng.choice([0.02, 0.1, 0.5, 1.0]))
    dtau = float(rng.choice([1e-4, 0.002, 0.01, 0.05]))
    loops = int(rng.choice([1, 1, 2, 3, 5, 7]))
    amp = float(rng.choice([0.01, 0.3, 3.0, 40.0, 400.0]))
    f = amp * rng.standard_normal(N)
    for value in (np.nan, np.inf, -np.inf):
        if rng.random() < 0.1:
            f[int(rng.integers(0, N))] = value
    if rng.random() < 0.5:
        runs, x, xx0 = 0, np.zeros(N), np.zeros(N)
    else:
        runs = int(rng.integers(1, 1001))
        x = 0.5 * rng.standard_normal(N)
        xx0 = 0.5 * rng.standard_normal(N)
    top = (N - 1) * dt
    kind = int(rng.integers(0, 6))
    tiny = float(np.sqrt(2 * dtau)) * 0.3
    omega = [dt * (N // 2), float(rng.uniform(0, top)), tiny * float(rng.random()),
             top - tiny * float(rng.random()), -float(rng.uniform(0, 0.3)) * top,
             top * (1 + float(rng.uniform(0, 0.3)))][kind]
    lrgEl = int(rng.integers(0, N)) if rng.random() < 0.4 else 0
    lrgVl = float(rng.choice([0.0, float(rng.uniform(0, 2.0)), float(rng.uniform(0, 2000.0))]))
    seed = int(rng.integers(0, 2 ** 31)) if rng.random() < 0.5 else int(rng.integers(0, 2 ** 48))
    return dict(N=N, dt=dt, dtau=dtau, pot=pot, C=C, loops=loops, seed=seed, omega=float(omega), lrgEl=lrgEl,
                lrgVl=lrgVl, runs=runs, f=f, x=x, xx0=xx0)


def bits(a):
    """The bit patterns of a float64 array (or scalar), every NaN as one."""
    a = np.array(a, dtype=np.float64, ndmin=1)
    a[np.isnan(a)] = np.nan
    return a.view(np.uint64)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


def launch_mismatch(got, want):
    """Names of the outputs of two launch results that differ in any bit."""
    bad = [k for k in ("stable", "lrgEl", "seed") if int(got[k]) != int(want[k])]
    bad += [k for k in ("omega", "lrgVl") + ARRAYS if not same(got[k], want[k])]
    return bad


def _hx(v):
    return float(v).hex()


def encode_launch(case, out=None):
    e = {k: case[k] for k in ("N", "pot", "loops", "seed", "lrgEl", "runs")}
    e.update({k: _hx(case[k]) for k in ("dt", "dtau", "C", "omega", "lrgVl")})
    e.update({k: [_hx(v) for v in case[k]] for k in ("f", "x", "xx0")})
    if out is not None:
        o = {k: int(out[k]) for k in ("stable", "lrgEl", "seed", "calls")}
        o.update({k: _hx(out[k]) for k in ("omega", "lrgVl")})
        o["omega_free"] = None if out.get("omega_free") is None else _hx(out["omega_free"])
        o.update({k: [_hx(v) for v in out[k]] for k in ARRAYS})
        e["out"] = o
    return e


def decode_launch(e):
    """(case, out) of one stored launch."""
    case = {k: e[k] for k in ("N", "pot", "loops", "seed", "lrgEl", "runs")}
    case.update({k: float.fromhex(e[k]) for k in ("dt", "dtau", "C", "omega", "lrgVl")})
    case.update({k: np.array([float.fromhex(v) for v in e[k]]) for k in ("f", "x", "xx0")})
    o = e["out"]
    out = {k: o[k] for k in ("stable", "lrgEl", "seed", "calls")}
    out.update({k: float.fromhex(o[k]) for k in ("omega", "lrgVl")})
    out["omega_free"] = None if o["omega_free"] is None else float.fromhex(o["omega_free"])
    out.update({k: np.array([float.fromhex(v) for v in o[k]]) for k in ARRAYS})
    return case, out


def derived(case, seed_after, random, intconst):
    """`calls` and `omega_free` of a launch from its input, the seed it left
    and one implementation of random(seed, gid) -> (xi, seed') and intConst.
    Every work-item calls random() once a round, in id order, and a break
    stops the work-items behind the one that found it, so the seed left is
    the seed after `calls` calls: the launch broke in round (calls - 1) //
    (N + 1), or ran all of them.  omega_free = omega + intConst * (C *
    sqrtf(2 dtau) * xi_N), the expression of tau_kernel.cl:105-106, for a
    launch of one round that reached work-item N."""
    s, xi, calls = case["seed"], 0.0, None
    n_items = case["N"] + 1
    for k in range(case["loops"] * n_items):
        xi, s = random(s, k % n_items)
        if s == seed_after:
            calls = k + 1
            break
    assert calls is not None, "the seed left is not a seed of the launch's call sequence"
    free = None
    if case["loops"] == 1 and calls == n_items:
        dw = case["C"] * float(np.sqrt(np.float32(2. * case["dtau"]))) * xi
        free = case["omega"] + intconst(case["pot"]) * dw
    return calls, free


CLASSES = ("stable", "break_round0", "break_later", "clip_pos", "clip_neg", "nan_site", "pinf_site", "ninf_site",
           "omega_lo", "omega_hi", "c0", "runs_carried", "leader_carried")
QUOTA = 2


def classes_of(case, out):
    """The classes a recorded launch belongs to, judged by its input and the
    reference's record alone."""
    c = set()
    f, top = case["f"], (case["N"] - 1) * case["dt"]
    finite = bool(np.all(np.isfinite(f)))
    if out["stable"] == 1:
        c.add("stable")
    else:
        c.add("break_round0" if out["calls"] <= case["N"] + 1 else "break_later")
    if finite and np.any(out["nf"] == 1000.0):
        c.add("clip_pos")
    if finite and np.any(out["nf"] == -1000.0):
        c.add("clip_neg")
    if np.any(np.isnan(f)):
        c.add("nan_site")
    if np.any(np.isposinf(f)):
        c.add("pinf_site")
    if np.any(np.isneginf(f)):
        c.add("ninf_site")
    w = out["omega_free"]
    if w is not None and w < 0 and out["omega"] == -w:
        c.add("omega_lo")
    if w is not None and w > top and out["omega"] == 2 * top - w:
        c.add("omega_hi")
    if case["C"] == 0:
        c.add("c0")
    if case["runs"] > 0 and np.any(case["x"] != 0) and np.any(case["xx0"] != 0):
        c.add("runs_carried")
    if case["lrgEl"] != 0 and out["lrgEl"] != case["lrgEl"] and out["stable"] == 1:
        c.add("leader_carried")
    return c


def required_slots():
    """(class, potID) pairs that need QUOTA cases each.  potID 0 has no omega
    reflection to show: its intConst is 0 and its x_cl ignores omega."""
    return [(k, p) for k in CLASSES for p in (0, 3) if not (p == 0 and k in ("omega_lo", "omega_hi"))]


def tally(entries):
    """{(class, potID): count} over decoded (case, out) pairs."""
    t = {s: 0 for s in required_slots()}
    for case, out in entries:
        for k in classes_of(case, out):
            if (k, case["pot"]) in t:
                t[(k, case["pot"])] += 1
    return t


# ---------------------------------------------------------------------------
# tauhost runs: the 13 arguments, with START / END for the two file names
# ---------------------------------------------------------------------------
CLI_N = (2, 3, 4, 5, 10, 100, 200)
FULL_BYTES = 1500     # longer outputs are stored as a digest


def cli_argv(N, dt, dtau, frames, pot, C, dev, fps, loops, acc, start="0", in_time=0):
    return [str(N), repr(dt), repr(dtau), str(frames), str(pot), str(C), str(dev), str(fps), str(in_time),
            str(loops), start, "END", str(acc)]


def draw_cli(rng):
    """One fresh run's arguments from the fixture's ranges: dtau / dt^2 = 0.2
    (stable), 1 (mixed) or 5 (every frame breaks)."""
    N = int(rng.choice(CLI_N))
    dt = float(rng.choice([0.02, 0.1, 0.5]))
    dtau = float(rng.choice([0.2, 1.0, 5.0])) * dt * dt
    loops = int(rng.choice([1, 10, 200]))
    return cli_argv(N, dt, dtau, int(rng.integers(1, 7)), int(rng.choice([0, 3])), int(rng.choice([0, 1])),
                    int(rng.choice([0, 2])), int(rng.choice([1, 3])), loops, int(rng.choice([12, 20, 40])))


def resume_of(argv):
    a = list(argv)
    a[8], a[10] = "1", "START"
    return a


def blob(data):
    """Output bytes as data: in full when short, else length, head and digest."""
    if data is None:
        return None
    text = data.decode("ascii")
    if len(data) <= FULL_BYTES:
        return {"text": text}
    return {"len": len(data), "head": text[:120], "blake2b": hashlib.blake2b(data, digest_size=16).hexdigest()}


def blob_matches(data, b):
    if b is None or data is None:
        return b is None and data is None
    return blob(data) == b


def terminate_fields(start_bytes, N):
    """The start file with a '|' behind the last field of each of its N site
    lines.  The reference copies a line into a buffer without a terminator
    before it splits it (tauhost.c:116-147), so what it reads for the last
    field, f, depends on the bytes that happen to follow on its stack: a digit
    there lengthens the exponent, and the run differs from one environment to
    the next.  With a delimiter behind it the field ends where the line does,
    which is how the oracle and the product read the plain file."""
    lines = start_bytes.split(b"\n")
    return b"\n".join(ln + b"|" if k < N else ln for k, ln in enumerate(lines))


def run_cli(run, workdir, argv, start_bytes=None):
    """Run one argument list with `run(argv, cwd)` in the empty directory
    `workdir`: START and END become the files start and end; returns
    (status, stdout bytes, end-file bytes or None)."""
    import os
    if start_bytes is not None:
        with open(os.path.join(workdir, "start"), "wb") as fh:
            fh.write(start_bytes)
    a = ["end" if v == "END" else "start" if v == "START" else v for v in argv]
    r = run(a, workdir)
    end = os.path.join(workdir, "end")
    data = None
    if os.path.exists(end):
        with open(end, "rb") as fh:
            data = fh.read()
    return r.returncode, r.stdout, data


def replay_cli(run, entries, root, terminate=False):
    """Run every recorded argument list in order with `run`, each in a fresh
    directory under `root`; a resume starts from the end file that `run` itself
    wrote in the run it continues (for the reference's own program, `terminate`:
    with its fields terminated, see terminate_fields).  {name: (status, stdout,
    end)}."""
    import os
    got = {}
    for e in entries:
        d = os.path.join(str(root), e["name"])
        os.makedirs(d)
        start = got[e["start_from"]][2] if e["start_from"] else None
        if start is not None and terminate:
            start = terminate_fields(start, int(e["argv"][0]))
        got[e["name"]] = run_cli(run, d, e["argv"], start)
    return got


def cli_mismatch(entry, result):
    """What of (status, stdout, end file) differs from the record.  Where the
    reference itself died of a signal (a negative status: it reads past argv
    when an argument is missing) any failure status stands for it."""
    status, out, end = result
    bad = []
    if (status == 0) if entry["status"] < 0 else (status != entry["status"]):
        bad.append(f"status {status} != {entry['status']}")
    if not blob_matches(out, entry["stdout"]):
        bad.append("stdout")
    if not blob_matches(end, entry["end"]):
        bad.append("end file")
    return bad
