"""Gradient-flow measurements inside the frames kernels (Euler and Heun) and inside the Heun step kernel of
the phi^4 lattice ensemble on the GPU: sq_phi4_ens_run_frames_flow, sq_phi4_ens_step_flow_heun;
Phi4Ensemble.run_frames_flow, run_frames(flow=True), step_flow(scheme="heun").

Every reference is a composition of calls that are pinned to the oracle elsewhere: a twin ensemble with the
same seeds, parameters and start fields runs the same frames (or Heun steps) one call at a time WITHOUT the flow
and takes flowed() of its stored fields between the calls; the correlator accumulators are summed on the host
from the twin's g and S in frame order, one addition each.  Tolerances: bit for bit everywhere.

The four replica columns (test_gpu_phi4_ens_heun_frames.py) give stable frames, rule-only firings and guard
trips; that every shape case shows all three is asserted from the twin's results alone.
"""
import ctypes

import numpy as np
import pytest

from test_gpu_phi4_ens_heun_frames import AMP, CN, DTAU, LAM, LOOPS, M2, SEEDS, SHAPES, STEP0
from test_phi4_ens_shapes import assert_shape

pytestmark = pytest.mark.gpu

CLAMP = 1000.0
EPS = 0.05
LEVELS = (0, 1, 3, 6)
ODD_LEVELS = (0, 2, 5)           # an odd last level: with two images the flow ends in the other one
SCHEMES = ("euler", "heun")
NFR = 8
# the smallest shape of each K, and K = 8 with either image count
PER_K = [(8, 2, 2), (64, 16, 8), (64, 3, 43), (8, 50, 51), (64, 11, 29)]

_cache = {}


def _ens(shape, cols=(0, 1, 2, 3), adapt=True, loops=LOOPS, dtau=None):
    from stochquant_amd import Phi4Ensemble
    c = list(cols)
    return Phi4Ensemble(shape, len(c), dtau=[DTAU[i] for i in c] if dtau is None else dtau, m2=[M2[i] for i in c],
                        lam=[LAM[i] for i in c], C=[CN[i] for i in c], seeds=[SEEDS[i] for i in c], clamp=CLAMP,
                        loops=loops, adapt_dtau=adapt)


def _start(shape):
    """The four columns' start fields, init_field(AMP[r]) of replica r's seed: once per shape, read-only."""
    key = ("start", shape)
    if key not in _cache:
        with _ens(shape) as E:
            out = None
            for amp in sorted(set(AMP)):
                E.init_field(amp)
                f = E.download()
                out = f.copy() if out is None else out
                for r in range(4):
                    if AMP[r] == amp:
                        out[r] = f[r]
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def _fresh(shape, levels=LEVELS, cols=(0, 1, 2, 3), flow_kw=None, **kw):
    E = _ens(shape, cols, **kw)
    E.upload(_start(shape)[list(cols)])
    E.step_counter = [STEP0[i] for i in cols]
    if levels is not None:
        E.set_flow(EPS, levels, **(flow_kw or {}))
    return E


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _sim_state(E, records=True):
    """Everything the flow must leave alone."""
    s = E.stability(n=LOOPS if records else 0)     # n given: a frames call through ctypes does not tell the wrapper
    out = {"field": E.download(), "step": E.step_counter, "flags": E.flags(), "dtau": E.dtau,
           "T": s["T"], "V": s["V"], "fired": s["fired"], "perf_steps": np.array(E.perf()["steps"])}
    if records:
        for r in range(E.R):
            n = LOOPS if s["fired"][r] < 0 else s["fired"][r] + 1
            for k in ("M", "D", "A"):
                out[f"{k}{r}"] = s[k][r][:n].copy()
    G, S1, N = E.corr_sums()
    out.update(cG=G, cS1=S1, cN=N)
    return out


def _assert_same_sim(a, b, tag):
    assert a.keys() == b.keys(), tag
    for k in a:
        assert _eq(a[k], b[k]), (tag, k, a[k], b[k])


def _s1_host(S):
    s = 0.0
    for v in S:
        s = s + float(v)
    return s


def _compose(shape, scheme, levels=LEVELS, flow_kw=None, n=NFR):
    """The twin's route, once per case: n times run_frames(1, measure=True) then flowed()."""
    key = ("compose", shape, scheme, levels, tuple(sorted((flow_kw or {}).items())), n)
    if key in _cache:
        return _cache[key]
    F = len(levels)
    with _fresh(shape, levels, flow_kw=flow_kw) as B:
        R, nt = B.R, B.nt
        st, dt, plain = [], [], []
        ser = np.zeros((n, F, R, 4))
        G, S1, N = np.zeros((R, F, nt)), np.zeros((R, F)), np.zeros(R, dtype=np.int64)
        kinds = set()
        for f in range(n):
            s, d, m = B.run_frames(1, measure=True, scheme=scheme)
            st.append(s[0])
            dt.append(d[0])
            plain.append(m[0])
            stab = B.stability()
            for r in range(R):
                k = LOOPS if stab["fired"][r] < 0 else stab["fired"][r] + 1
                guard = bool((stab["A"][r][:k] >= CLAMP).any())
                assert bool(s[0, r]) == (stab["fired"][r] < 0 and not guard)
                kinds.add("stable" if s[0, r] else ("guard" if guard else "rule"))
            sums, S, g = B.flowed()
            ser[f] = sums.transpose(1, 0, 2)
            for r in range(R):
                if s[0, r]:
                    for l in range(F):
                        G[r, l] = G[r, l] + g[r, l]
                        S1[r, l] = S1[r, l] + _s1_host(S[r, l])
                    N[r] += 1
        out = dict(st=np.array(st), dt=np.array(dt), plain=np.array(plain), ser=ser, G=G, S1=S1, N=N, kinds=kinds,
                   sim=_sim_state(B))
    _cache[key] = out
    return out


def _assert_telling(ref):
    """From the twin alone: a stable frame, a rule-only firing and a guard trip among the case's replicas."""
    assert ref["kinds"] == {"stable", "rule", "guard"}, ref["kinds"]


def _check_composition(shape, scheme, levels=LEVELS, flow_kw=None):
    ref = _compose(shape, scheme, levels, flow_kw)
    _assert_telling(ref)
    with _fresh(shape, levels, flow_kw=flow_kw) as A:
        st, dt, ser = A.run_frames_flow(NFR, correlate=True, scheme=scheme)
        assert A.perf()["kernel_launches"] == 1
        assert ser.shape == (NFR, len(levels), A.R, 4)
        assert _eq(st, ref["st"]) and _eq(dt, ref["dt"]), (st, ref["st"])
        for f in range(NFR):
            assert _eq(ser[f], ref["ser"][f]), (f, np.argwhere(ser[f] != ref["ser"][f])[:4])
        G, S1, N = A.fcorr_sums()
        assert list(N) == list(ref["N"]) == list(ref["st"].sum(axis=0))
        assert _eq(G, ref["G"]) and _eq(S1, ref["S1"])
        sim = _sim_state(A)
        assert not sim["cN"].any() and not sim["cG"].any() and not sim["cS1"].any()   # the plain accumulators rest
        _assert_same_sim(sim, ref["sim"], (shape, scheme))     # perf's step count too: the early exits agree
    return ref


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", SHAPES)
def test_composition(gpu, shape, scheme):
    assert_shape(shape)
    ref = _check_composition(shape, scheme)
    if LEVELS[0] == 0:
        assert _eq(ref["ser"][:, 0], ref["plain"])


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", [(16, 4, 31), (8, 50, 51)])
def test_composition_odd_last_level(gpu, shape, scheme):
    _check_composition(shape, scheme, ODD_LEVELS)


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", [(8, 2, 2), (64, 16, 8), (8, 2, 2048)])
def test_level_zero_row_is_the_measured_series(gpu, shape, scheme):
    n = 4
    with _fresh(shape) as A, _fresh(shape, None) as B:
        sa, da, ser = A.run_frames(n, flow=True, scheme=scheme)
        sb, db, plain = B.run_frames(n, measure=True, scheme=scheme)
        assert ser.shape == (n, len(LEVELS), A.R, 4) and plain.shape == (n, A.R, 4)
        assert _eq(sa, sb) and _eq(da, db)
        assert _eq(ser[:, 0], plain)
        assert not sa.all() and sa.any()
        # measure is ignored with flow=True: the series comes back either way
        assert len(A.run_frames(1, measure=False, flow=True, scheme=scheme)) == 3


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", PER_K)
def test_flow_leaves_the_run_alone(gpu, shape, scheme):
    """One call with the flow against one call without it: verdicts, dtau, fields, counters, flags, T, V, the
    controller (through the dtau of later frames), the step records, the plain accumulators."""
    n = 6
    with _fresh(shape) as A, _fresh(shape, None) as B:
        sa, da, _ = A.run_frames_flow(n, correlate=True, scheme=scheme)
        sb, db = B.run_frames(n, scheme=scheme)
        assert _eq(sa, sb) and _eq(da, db)
        _assert_same_sim(_sim_state(A), _sim_state(B), (shape, scheme))
        # the controller's count is part of the state: the next frames agree as well
        s2a, d2a = A.run_frames(7, scheme=scheme)
        s2b, d2b = B.run_frames(7, scheme=scheme)
        assert _eq(s2a, s2b) and _eq(d2a, d2b)


def _raw_frames_flow(E, n, series, correlate, scheme):
    from stochquant_amd import _lib
    st = np.zeros((n, E.R), dtype=np.int32)
    dt = np.zeros((n, E.R))
    ser = np.zeros((n, len(E.flow["levels"]), E.R, 4)) if series else None
    rc = _lib.load().sq_phi4_ens_run_frames_flow(
        E._h, n, st.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), dt.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
        None if ser is None else ser.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 1 if correlate else 0,
        SCHEMES.index(scheme))
    return rc, st != 0, dt, ser


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", [(16, 4, 31), (64, 11, 29)])
def test_series_only_correlate_only_neither(gpu, shape, scheme):
    ref = _compose(shape, scheme)
    # correlate only (series = NULL): the accumulators of the full call
    with _fresh(shape) as A:
        rc, st, dt, _ = _raw_frames_flow(A, NFR, False, True, scheme)
        assert rc == 0 and _eq(st, ref["st"]) and _eq(dt, ref["dt"])
        G, S1, N = A.fcorr_sums()
        assert list(N) == list(ref["N"]) and _eq(G, ref["G"]) and _eq(S1, ref["S1"])
        _assert_same_sim(_sim_state(A), ref["sim"], (shape, scheme, "correlate only"))
    # series only: the rows, and the accumulators at rest
    with _fresh(shape) as A:
        rc, st, dt, ser = _raw_frames_flow(A, NFR, True, False, scheme)
        assert rc == 0 and _eq(st, ref["st"]) and _eq(ser, ref["ser"])
        G, S1, N = A.fcorr_sums()
        assert not N.any() and not G.any() and not S1.any()
        _assert_same_sim(_sim_state(A), ref["sim"], (shape, scheme, "series only"))
    # neither: the plain frames call
    with _fresh(shape) as A:
        rc, st, dt, _ = _raw_frames_flow(A, NFR, False, False, scheme)
        assert rc == 0 and _eq(st, ref["st"]) and _eq(dt, ref["dt"])
        assert not A.fcorr_sums()[2].any()
        _assert_same_sim(_sim_state(A), ref["sim"], (shape, scheme, "neither"))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_unstable_frames_measure_no_correlator(gpu, scheme):
    shape = (16, 4, 31)
    with _fresh(shape, adapt=False, dtau=3.0) as A:
        start = A.download()
        st, dt, ser = A.run_frames_flow(3, correlate=True, scheme=scheme)
        assert not st.any() and np.all(dt == 3.0)
        G, S1, N = A.fcorr_sums()
        assert not N.any() and not G.any() and not S1.any()
        assert _eq(A.download(), start)
        sums = A.flowed()[0].transpose(1, 0, 2)
        for f in range(3):                       # every rolled-back frame repeats the start field's rows
            assert _eq(ser[f], sums), f


@pytest.mark.parametrize("shape", SHAPES)
def test_heun_steps_with_flow(gpu, shape):
    assert_shape(shape)
    n, k = 7, 3
    counters = [0, 2 ** 32 - 2, 0, 2 ** 32 - 2]
    F = len(LEVELS)
    with _fresh(shape) as A, _fresh(shape) as B:
        for E in (A, B):
            E.step_counter = counters
        ser = A.step_flow(n, k, correlate=True, scheme="heun")
        assert ser.shape == (n // k, F, A.R, 4) and A.perf()["kernel_launches"] == 1
        G, S1 = np.zeros((B.R, F, B.nt)), np.zeros((B.R, F))
        for m in range(n // k):
            B.step(k, scheme="heun")
            sums, S, g = B.flowed()
            assert _eq(ser[m], sums.transpose(1, 0, 2)), m
            for r in range(B.R):
                for l in range(F):
                    G[r, l] = G[r, l] + g[r, l]
                    S1[r, l] = S1[r, l] + _s1_host(S[r, l])
        B.step(n % k, scheme="heun")             # the incomplete tail: stepped, not measured
        aG, aS1, aN = A.fcorr_sums()
        assert list(aN) == [n // k] * A.R and _eq(aG, G) and _eq(aS1, S1)
        _assert_same_sim(_sim_state(A, records=False), _sim_state(B, records=False), shape)
        assert list(A.step_counter) == [c + n for c in counters]


def test_heun_step_flow_tail_and_alternation(gpu):
    shape = (16, 4, 31)
    F = len(LEVELS)
    with _fresh(shape) as A, _fresh(shape) as B:
        # an incomplete tail measures nothing and still steps
        ser = A.step_flow(2, 3, correlate=True, scheme="heun")
        B.step(2, scheme="heun")
        assert ser.shape == (0, F, A.R, 4) and not A.fcorr_sums()[2].any()
        assert _eq(A.download(), B.download())
        # neither series nor correlate: the plain Heun call
        from stochquant_amd import _lib
        assert _lib.load().sq_phi4_ens_step_flow_heun(A._h, 3, 1, None, 0) == 0
        B.step(3, scheme="heun")
        assert _eq(A.download(), B.download()) and not A.fcorr_sums()[2].any()
        # Heun and Euler flow calls alternate on one handle
        G, S1 = np.zeros((B.R, F, B.nt)), np.zeros((B.R, F))
        for scheme in ("heun", "euler", "heun", "euler"):
            ser = A.step_flow(3, 3, correlate=True, scheme=scheme)
            B.step(3, scheme=scheme)
            sums, S, g = B.flowed()
            assert _eq(ser[0], sums.transpose(1, 0, 2)), scheme
            for r in range(B.R):
                for l in range(F):
                    G[r, l] = G[r, l] + g[r, l]
                    S1[r, l] = S1[r, l] + _s1_host(S[r, l])
        aG, aS1, aN = A.fcorr_sums()
        assert list(aN) == [4] * A.R and _eq(aG, G) and _eq(aS1, S1)
        _assert_same_sim(_sim_state(A, records=False), _sim_state(B, records=False), "alternation")


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", [(16, 4, 31), (64, 11, 29)])
def test_split_calls(gpu, shape, scheme):
    with _fresh(shape) as A, _fresh(shape) as B:
        sa, da, ra = A.run_frames_flow(5, correlate=True, scheme=scheme)
        s1, d1, r1 = B.run_frames_flow(2, correlate=True, scheme=scheme)
        s2, d2, r2 = B.run_frames_flow(3, correlate=True, scheme=scheme)
        s0, d0, r0 = B.run_frames_flow(0, correlate=True, scheme=scheme)
        assert s0.shape == d0.shape == (0, B.R) and r0.shape == (0, len(LEVELS), B.R, 4)
        assert _eq(sa, np.concatenate([s1, s2])) and _eq(da, np.concatenate([d1, d2]))
        assert _eq(ra, np.concatenate([r1, r2]))
        for x, y in zip(A.fcorr_sums(), B.fcorr_sums()):
            assert _eq(x, y)
        _assert_same_sim(_sim_state(A), _sim_state(B), (shape, scheme))


@pytest.mark.parametrize("scheme", SCHEMES)
def test_independent_of_replica_count_and_position(gpu, scheme):
    shape, n = (16, 4, 31), 5
    cols7 = (3, 0, 1, 2, 3, 1, 0)
    with _fresh(shape, cols=cols7) as A:
        sa, da, ra = A.run_frames_flow(n, correlate=True, scheme=scheme)
        Ga, S1a, Na = A.fcorr_sums()
        fa = A.download()
    ref4 = None
    for cols in ((0, 1, 2, 3), (0,), (1,), (2,), (3,)):
        with _fresh(shape, cols=cols) as B:
            sb, db, rb = B.run_frames_flow(n, correlate=True, scheme=scheme)
            Gb, S1b, Nb = B.fcorr_sums()
            fb = B.download()
        if len(cols) == 4:
            ref4 = (sb, db, rb, Gb, S1b, Nb, fb)
        for j, c in enumerate(cols):
            for i in [i for i, ci in enumerate(cols7) if ci == c]:        # R = 7 against R = 4 and R = 1
                assert _eq(sa[:, i], sb[:, j]) and _eq(da[:, i], db[:, j]), (cols, c, i)
                assert _eq(ra[:, :, i], rb[:, :, j]), (cols, c, i)
                assert _eq(Ga[i], Gb[j]) and _eq(S1a[i], S1b[j]) and Na[i] == Nb[j], (cols, c, i)
                assert _eq(fa[i], fb[j])
    assert ref4 is not None and ref4[5].any()


@pytest.mark.parametrize("scheme", SCHEMES)
@pytest.mark.parametrize("shape", PER_K)
def test_shared_flow_coefficients(gpu, shape, scheme):
    """The flow's own m2 = lambda = 0 for all replicas (the heat equation); each replica's own m2 / lambda is
    test_composition's case."""
    _check_composition(shape, scheme, LEVELS, dict(m2=0.0, lam=0.0))


def test_arguments(gpu):
    from stochquant_amd import StochQuantError, _lib
    lib = _lib.load()
    shape = (8, 2, 2)
    R = 4
    st = (ctypes.c_int * (4 * R))()
    dt = (ctypes.c_double * (4 * R))()
    ser = (ctypes.c_double * (4 * 4 * R * 4))()

    def state(E):
        return (E.flow, [a.copy() for a in E.fcorr_sums()] if E.flow else None, _sim_state(E, records=False))

    def same(a, b):
        assert a[0] == b[0]
        if a[1] is not None:
            assert all(_eq(x, y) for x, y in zip(a[1], b[1]))
        _assert_same_sim(a[2], b[2], "refused call")

    with _fresh(shape, None) as E:
        before = state(E)
        for scheme in (0, 1):                   # no flow set
            assert lib.sq_phi4_ens_run_frames_flow(E._h, 2, st, dt, ser, 1, scheme) == -4
        assert lib.sq_phi4_ens_step_flow_heun(E._h, 4, 2, ser, 1) == -4
        with pytest.raises(StochQuantError) as ei:
            E.run_frames(2, flow=True)
        assert ei.value.code == -4
        same(before, state(E))
        E.set_flow(EPS, LEVELS)
        E.run_frames_flow(2, correlate=True)
        before = state(E)
        assert lib.sq_phi4_ens_run_frames_flow(E._h, 2, st, dt, ser, 1, 2) == -1        # scheme
        assert lib.sq_phi4_ens_run_frames_flow(E._h, 2, st, dt, ser, 1, -1) == -1
        assert lib.sq_phi4_ens_run_frames_flow(E._h, -1, st, dt, ser, 1, 0) == -1       # nframes < 0
        assert lib.sq_phi4_ens_run_frames_flow(E._h, 2, None, dt, ser, 1, 0) == -1      # sq_phi4_ens_run_frames' rule
        assert lib.sq_phi4_ens_run_frames_flow(E._h, 2, st, None, ser, 1, 1) == -1
        assert lib.sq_phi4_ens_step_flow_heun(E._h, 4, 0, ser, 1) == -1                  # every < 1
        assert lib.sq_phi4_ens_step_flow_heun(E._h, -1, 2, ser, 1) == -1
        same(before, state(E))
        for scheme in (0, 1):                   # nframes = 0 succeeds with null outputs
            assert lib.sq_phi4_ens_run_frames_flow(E._h, 0, None, None, None, 1, scheme) == 0
        assert lib.sq_phi4_ens_step_flow_heun(E._h, 0, 2, None, 1) == 0
        same(before, state(E))
    # loops < 1: as run_frames handles it
    with _fresh(shape, loops=0) as E:
        before = state(E)
        assert lib.sq_phi4_ens_run_frames(E._h, 2, st, dt, None) == -1
        for scheme in (0, 1):
            assert lib.sq_phi4_ens_run_frames_flow(E._h, 2, st, dt, ser, 1, scheme) == -1
        same(before, state(E))
