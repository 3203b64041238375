"""The phi^4 ensemble checkpoint's format in NumPy, written from the words of include/stochquant.h ("Checkpoints of the
phi^4 ensemble") and not by calling the library: the digest, a writer, and a strict reader.  The CPU tests hand the
writer's files to the library and the library's rules to mutated files; the GPU tests read the library's files here.

A checkpoint `path` is `path` (.npy, float32, (R, Lz, Ly, Lx)), `path`.state (raw sections, 8-byte aligned) and
`path`.json (the metadata, which names sizes, digests and the section table)."""
import json
import os

import numpy as np

FORMAT = "stochquant-phi4-ensemble"
KEYS = ("format", "version", "dims", "R", "loops", "clamp_bits", "clamp", "adapt_dtau", "exchange_round", "cluster_sweep",
        "ladder", "momenta", "flow_levels", "flow_eps_bits", "flow_eps", "flow_m2_bits", "flow_m2", "flow_lambda_bits",
        "flow_lambda", "field_bytes", "state_bytes", "state_digest", "meta_digest", "field_digest", "sections")
INFORMATIVE = ("clamp", "flow_eps", "flow_m2", "flow_lambda")
OPTIONAL = ("frame_records", "mala_stats", "hmc_stats")
MAX_MOMENTA, MAX_FLOW_LEVELS, MAX_FLOW_STEPS, MAX_SITES = 8, 4, 4096, 32768
U64 = (1 << 64) - 1
I32 = (1 << 31) - 1


class Refused(Exception):
    """The files are not a checkpoint of this format."""


# ---- the digest ----
def mix(x):
    x = np.asarray(x, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> np.uint64(30)
        x *= np.uint64(0xBF58476D1CE4E5B9)
        x ^= x >> np.uint64(27)
        x *= np.uint64(0x94D049BB133111EB)
        x ^= x >> np.uint64(31)
    return x


def digest_words(words):
    """sum_i mix(i << 32 | words[i]) mod 2^64 of uint32 words."""
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
    key = (np.arange(w.size, dtype=np.uint64) << np.uint64(32)) | w.astype(np.uint64)
    with np.errstate(over="ignore"):
        return int(np.sum(mix(key), dtype=np.uint64))


def digest_bytes(b):
    b = bytes(b)
    b += b"\0" * (-len(b) % 4)
    return digest_words(np.frombuffer(b, dtype="<u4"))


def field_digest(row):
    """The digest of one replica's field: its float32 values' bit patterns in C order."""
    return digest_words(np.ascontiguousarray(row, dtype=np.float32).view(np.uint32))


def bits(x):
    return int(np.array(x, dtype=np.float64).view(np.uint64))


def from_bits(b):
    return float(np.array(b, dtype=np.uint64).view(np.float64))


# ---- the files' parts ----
def npy_preamble(R, Lz, Ly, Lx):
    hdr = "{'descr': '<f4', 'fortran_order': False, 'shape': (%d, %d, %d, %d), }" % (R, Lz, Ly, Lx)
    hdr += " " * (-(10 + len(hdr) + 1) % 64) + "\n"
    return b"\x93NUMPY\x01\x00" + len(hdr).to_bytes(2, "little") + hdr.encode("ascii")


def section_table(dims, R, loops, M, F, frame_records=True, mala=True, hmc=True):
    """[(name, dtype, shape)] in the writer's order."""
    nt = dims[2] // 2 + 1
    t = [(n, "<u8", (R,)) for n in ("seed", "step")]
    t += [(n, "<f8", (R,)) for n in ("dtau", "m2", "lambda", "C")]
    t += [("flags", "<i4", (R,)), ("frame_dtau", "<f8", (R,)), ("frame_C", "<f8", (R,)), ("frame_T", "<f4", (R,)),
          ("frame_V", "<f4", (R,))]
    t += [(n, "<i4", (R,)) for n in ("frame_init", "frame_cnt", "frame_fired", "frame_flag", "frame_exec")]
    if frame_records and loops >= 1:
        t += [("frame_records", "<f4", (R, 3, loops))]
    t += [("corr_G", "<f8", (R, nt)), ("corr_S1", "<f8", (R,)), ("corr_nmeas", "<i8", (R,))]
    if M > 0:
        t += [("pcorr_G", "<f8", (R, M, nt))]
    t += [("pcorr_nmeas", "<i8", (R,))]
    if F > 0:
        t += [("flow_G", "<f8", (R, F, nt)), ("flow_S1", "<f8", (R, F)), ("flow_nmeas", "<i8", (R, F))]
    if mala:
        t += [("mala_stats", "<i8", (R, 3))]
    if hmc:
        t += [("hmc_stats", "<i8", (R, 4))]
    t += [("exchange_stats", "<i8", (R, 2)), ("walkers", "<i4", (R,)), ("cluster_stats", "<i8", (R, 5))]
    return t


def default_state(dims, R, loops, M=0, F=0, frame_records=False, mala=False, hmc=False):
    """The sections of a fresh handle with plain parameters: {name: array}."""
    st = {n: np.zeros(s, dtype=d) for n, d, s in section_table(dims, R, loops, M, F, frame_records, mala, hmc)}
    st["seed"][:] = 0x5EED + np.arange(R, dtype=np.uint64)
    st["dtau"][:] = st["frame_dtau"][:] = 0.01
    st["m2"][:] = st["lambda"][:] = st["C"][:] = st["frame_C"][:] = 1.0
    st["frame_fired"][:] = -1
    st["walkers"][:] = np.arange(R)
    return st


def meta_digest(m):
    w = [m["version"], *m["dims"], m["R"], m["loops"], m["clamp_bits"], m["adapt_dtau"], m["exchange_round"],
         m["cluster_sweep"], m["ladder"], len(m["momenta"])]
    w += [n for p in m["momenta"] for n in p]
    w += [len(m["flow_levels"]), *m["flow_levels"]]
    w += [m["flow_eps_bits"], m["flow_m2_bits"], m["flow_lambda_bits"], m["field_bytes"], m["state_bytes"], m["state_digest"]]
    w += list(m["field_digest"])
    w += [len(m["sections"])] + [s["offset"] for s in m["sections"]]
    return digest_bytes(np.array([x & U64 for x in w], dtype="<u8").tobytes())


def _dec(x):
    return x if np.isfinite(x) else None


def write(path, fields, state, loops=100, clamp=1000.0, adapt_dtau=True, exchange_round=0, cluster_sweep=0, ladder=0,
          momenta=(), flow_levels=(), flow_eps=0.0, flow_m2=float("nan"), flow_lambda=float("nan")):
    """Write the three files; fields (R, Lz, Ly, Lx) float32, state {name: array} in file order.  Returns the
    metadata as a dict."""
    path = os.fspath(path)
    fields = np.ascontiguousarray(fields, dtype=np.float32)
    R, Lz, Ly, Lx = fields.shape
    blob, sections = b"", []
    for name, a in state.items():
        a = np.ascontiguousarray(a)
        sections.append({"name": name, "dtype": a.dtype.newbyteorder("<").str, "shape": list(a.shape), "offset": len(blob)})
        blob += a.tobytes()
        blob += b"\0" * (-len(blob) % 8)
    pre = npy_preamble(R, Lz, Ly, Lx)
    m = {"format": FORMAT, "version": 1, "dims": [Lx, Ly, Lz], "R": R, "loops": int(loops), "clamp_bits": bits(clamp),
         "clamp": _dec(clamp), "adapt_dtau": 1 if adapt_dtau else 0, "exchange_round": int(exchange_round),
         "cluster_sweep": int(cluster_sweep), "ladder": int(ladder), "momenta": [list(p) for p in momenta],
         "flow_levels": list(flow_levels), "flow_eps_bits": bits(flow_eps), "flow_eps": _dec(flow_eps),
         "flow_m2_bits": bits(flow_m2), "flow_m2": _dec(flow_m2), "flow_lambda_bits": bits(flow_lambda),
         "flow_lambda": _dec(flow_lambda), "field_bytes": len(pre) + fields.nbytes, "state_bytes": len(blob),
         "state_digest": digest_bytes(blob), "field_digest": [field_digest(fields[r]) for r in range(R)],
         "sections": sections}
    m["meta_digest"] = meta_digest(m)
    with open(path, "wb") as fh:
        fh.write(pre + fields.tobytes())
    with open(path + ".state", "wb") as fh:
        fh.write(blob)
    write_meta(path, m)
    return m


def write_meta(path, m):
    with open(os.fspath(path) + ".json", "w") as fh:
        fh.write(json.dumps(m))  # nothing behind the closing brace


# ---- the strict reader ----
def _no(why):
    raise Refused(why)


def _pairs(p):
    d = dict(p)
    if len(d) != len(p):
        _no("a key appears twice")
    return d


def _int(v, lo, hi, what):
    if type(v) is not int or not lo <= v <= hi:
        _no(f"{what} is not an integer in [{lo}, {hi}]")
    return v


def _ints(v, n_max, lo, hi, what):
    if type(v) is not list or len(v) > n_max:
        _no(f"{what} is not a list of at most {n_max}")
    return [_int(x, lo, hi, what) for x in v]


def parse_meta(text):
    """The metadata of `text` (bytes), everything checked that the metadata alone can show."""
    if b"\\" in text:
        _no("an escape")
    try:
        m = json.loads(text.decode("ascii"), object_pairs_hook=_pairs, parse_constant=lambda c: _no("not JSON: " + c))
    except Refused:
        raise
    except Exception as e:  # not JSON, not ASCII
        _no(f"not complete JSON: {e}")
    if type(m) is not dict or set(m) != set(KEYS):
        _no("not an object of exactly the format's keys")
    if m["format"] != FORMAT:
        _no("wrong format name")
    if _int(m["version"], 0, 1 << 30, "version") != 1:
        _no("unknown version")
    d = _ints(m["dims"], 3, 0, 1 << 30, "dims")
    if len(d) != 3:
        _no("dims")
    Lx, Ly, Lz = d
    if Lx not in (8, 16, 32, 64) or Ly < 2 or Lz < 2 or max(Ly, Lz) > MAX_SITES or Lx * Ly * Lz > MAX_SITES:
        _no("an illegal lattice shape")
    R = _int(m["R"], 1, I32, "R")
    loops = _int(m["loops"], -I32 - 1, I32, "loops")
    _int(m["adapt_dtau"], 0, 1, "adapt_dtau")
    for k in ("clamp_bits", "exchange_round", "cluster_sweep", "flow_eps_bits", "flow_m2_bits", "flow_lambda_bits",
              "field_bytes", "state_bytes", "state_digest", "meta_digest"):
        _int(m[k], 0, U64, k)
    for k in INFORMATIVE:
        if type(m[k]) not in (int, float, type(None)):
            _no(k)
    lad = _int(m["ladder"], 0, I32, "ladder")
    if lad != 0 and (lad < 2 or lad > R or R % lad):
        _no("ladder does not divide R")
    if type(m["momenta"]) is not list or len(m["momenta"]) > MAX_MOMENTA:
        _no("momenta")
    for p in m["momenta"]:
        p = _ints(p, 2, -I32, I32, "a momentum")
        if len(p) != 2 or not (0 <= p[0] < Lx and 0 <= p[1] < Ly):
            _no("a momentum outside the lattice")
    lev = _ints(m["flow_levels"], MAX_FLOW_LEVELS, -I32, I32, "flow_levels")
    for i, n in enumerate(lev):
        if n < (lev[i - 1] + 1 if i else 0) or n > MAX_FLOW_STEPS:
            _no("flow levels do not ascend")
    if type(m["field_digest"]) is not list or len(m["field_digest"]) != R:
        _no("field_digest is not R digests")
    for x in m["field_digest"]:
        _int(x, 0, U64, "a field digest")
    if m["field_bytes"] != len(npy_preamble(R, Lz, Ly, Lx)) + 4 * R * Lx * Ly * Lz:
        _no("field_bytes is not the size of the shape's .npy")
    known = {n: (dt, list(s)) for n, dt, s in section_table((Lx, Ly, Lz), R, loops, len(m["momenta"]), len(lev))}
    if type(m["sections"]) is not list or len(m["sections"]) > len(known):
        _no("sections")
    seen, spans = set(), []
    for s in m["sections"]:
        if type(s) is not dict or set(s) != {"name", "dtype", "shape", "offset"}:
            _no("a section is not {name, dtype, shape, offset}")
        if type(s["name"]) is not str or s["name"] not in known:
            _no(f"unknown section {s['name']!r}")
        if s["name"] in seen:
            _no("a section appears twice")
        seen.add(s["name"])
        dt, shape = known[s["name"]]
        if s["dtype"] != dt or _ints(s["shape"], 4, 0, I32, "shape") != shape:
            _no(f"section {s['name']} has another dtype or shape")
        off = _int(s["offset"], 0, U64, "offset")
        n = int(np.prod(shape, dtype=object)) * int(dt[2])
        if off % 8 or off > m["state_bytes"] or n > m["state_bytes"] - off:
            _no(f"section {s['name']} is misaligned or reaches past the end")
        spans.append((off, off + n))
    if [n for n in known if n not in OPTIONAL and n not in seen]:
        _no("a required section is missing")
    spans.sort()
    if any(a[1] > b[0] for a, b in zip(spans, spans[1:])):
        _no("sections overlap")
    if m["meta_digest"] != meta_digest(m):
        _no("meta_digest")
    return m


def meaning(m):
    """The metadata without its informative copies."""
    return {k: v for k, v in m.items() if k not in INFORMATIVE}


def read(path, verify=True):
    """(metadata, fields (R, Lz, Ly, Lx), {section: array}) of checkpoint `path`; Refused for anything a load refuses
    without a handle's knowledge."""
    path = os.fspath(path)
    try:
        with open(path + ".json", "rb") as fh:
            m = parse_meta(fh.read())
        with open(path + ".state", "rb") as fh:
            blob = fh.read()
        with open(path, "rb") as fh:
            f = fh.read()
    except OSError as e:
        _no(f"missing file: {e}")
    Lx, Ly, Lz = m["dims"]
    R = m["R"]
    pre = npy_preamble(R, Lz, Ly, Lx)
    if verify:
        if len(blob) != m["state_bytes"] or digest_bytes(blob) != m["state_digest"]:
            _no("the state file's size or digest")
        if len(f) != m["field_bytes"] or f[:len(pre)] != pre:
            _no("the field file's size or .npy header")
    fields = np.frombuffer(f, dtype="<f4", offset=len(pre)).reshape(R, Lz, Ly, Lx)
    if verify and [field_digest(fields[r]) for r in range(R)] != m["field_digest"]:
        _no("a field digest")
    state = {s["name"]: np.frombuffer(blob, dtype=s["dtype"], count=int(np.prod(s["shape"])), offset=s["offset"])
             .reshape(s["shape"]) for s in m["sections"]}
    return m, fields, state
