"""Frames of the phi^4 lattice ensemble on the GPU (sq_phi4_ens_run_frames,
Phi4Ensemble.run_frames): per replica `loops` steps, the stability rule, the
rollback and the Δτ controller, all decided inside the one launch of the call.

Replica r must be bit for bit the single context (Phi4Lattice.run_frames) of
its seed, parameters, `loops`, step counter and start field: verdicts, the Δτ
after every frame, the field, the carried T / V, the firing step, the records
M / D / A through the firing step (the ensemble skips the rest of a frame whose
rule has fired; the context runs them, without effect on anything it keeps)
and the step counter.  The base recipe is test_run_frames_match_host_frames':
init_field(0.3), m² = λ = C = 1, loops = 12, 40 frames, Δτ₀ = 0.19 (above the
Euler limit: rolled-back frames by the rule and by the guard, then stable
ones and a Δτ / 0.95), seed 99.

Tolerances: bitwise everywhere, except the in-flight sums against the exactly
rounded sums of the downloaded field, where the bound is the ensemble suite's
2 n u Σ|t| (u = 2^-53: n double additions in any order, one more rounding per
phi^4 term; see test_gpu_phi4_ens.py).
"""
import math

import numpy as np
import pytest

from test_phi4_ens_shapes import assert_shape

pytestmark = pytest.mark.gpu

LOOPS, NFR = 12, 40
SEEDS = [99, 1234, 0xDEADBEEF12345]
DTAU0 = [0.19, 0.01, 0.19]
STEP0 = [0, 0, 2 ** 32 - 100]      # replica 2's counter carries into the high word during the run
SHAPES = [(8, 2, 2), (16, 4, 31), (64, 16, 8), (32, 32, 32), (64, 16, 32),
          # K >= 2 with owned quads that do not exist (lanes that carry -inf quads and mp = 0 through the record),
          # K = 4, K = 8 with two images at the LDS limit, the first one-image lattice, Ly = 2 at K = 8
          (8, 17, 31), (64, 3, 43), (16, 32, 32), (8, 50, 51), (64, 11, 29), (32, 2, 321),
          # the other ways the last j can end, per K and image count: inside a wave with every wave still holding
          # a quad, and on a wave boundary with whole waves empty (test_phi4_ens_shapes.py)
          (8, 20, 28), (8, 16, 34), (32, 4, 71), (16, 20, 28), (32, 12, 47), (16, 16, 71), (64, 12, 29)]
MEASURED = [(64, 3, 43), (16, 32, 32), (8, 50, 51), (32, 2, 321)]

_cache = {}


def _ens(shape, R, **kw):
    from stochquant_amd import Phi4Ensemble
    kw.setdefault("m2", 1.0)
    kw.setdefault("lam", 1.0)
    kw.setdefault("C", 1.0)
    kw.setdefault("loops", LOOPS)
    return Phi4Ensemble(shape, R, **kw)


def _lat(shape, **kw):
    from stochquant_amd import Phi4Lattice
    kw.setdefault("m2", 1.0)
    kw.setdefault("lam", 1.0)
    kw.setdefault("C", 1.0)
    kw.setdefault("loops", LOOPS)
    return Phi4Lattice(shape, **kw)


def _state(L, st, dt):
    return {"stable": np.array(st, dtype=bool), "dtau": np.array(dt, dtype=np.float64), "field": L.download(),
            "stab": L.stability(), "step": int(L.step_counter)}


def _ref(shape, r, adapt=True, nfr=NFR):
    """Phi4Lattice.run_frames of replica r's recipe (one run per shape, replica and mode, shared)."""
    key = (shape, r, adapt, nfr)
    if key not in _cache:
        with _lat(shape, dtau=DTAU0[r], seed=SEEDS[r], adapt_dtau=adapt) as L:
            L.init_field(0.3)
            L.step_counter = STEP0[r]
            st, dt = L.run_frames(nfr)
            _cache[key] = _state(L, st, dt)
        _cache[key]["field"].setflags(write=False)
    return _cache[key]


def _recipe(shape, **kw):
    E = _ens(shape, 3, dtau=DTAU0, seeds=SEEDS, **kw)
    E.init_field(0.3)
    E.step_counter = STEP0
    return E


def _check(E, st, dt, r, ref, tag=""):
    """Replica r of E after frames with verdicts st[:, r] and Δτ dt[:, r] against a single context's state."""
    tag = f"{tag} replica {r}"
    assert np.array_equal(st[:, r], ref["stable"]), tag
    assert np.array_equal(dt[:, r], ref["dtau"]), tag                 # the same doubles, not approximately
    assert np.array_equal(E.download(first=r, count=1)[0], ref["field"]), tag
    s, rs = E.stability(first=r, count=1), ref["stab"]
    assert s["T"][0] == rs["T"] and s["V"][0] == rs["V"] and s["fired"][0] == rs["fired"], (tag, s, rs)
    n = LOOPS if rs["fired"] < 0 else rs["fired"] + 1
    for k in ("M", "D", "A"):
        assert np.array_equal(s[k][0][:n], rs[k][:n]), (tag, k)
    assert int(E.step_counter[r]) == ref["step"], tag
    assert E.get_params(first=r, count=1)["dtau"][0] == ref["dtau"][-1], tag


@pytest.mark.parametrize("shape", SHAPES)
def test_frames_bitwise_vs_single_context(gpu, shape):
    """One wave; K = 1 with a partial wave and two images; K = 2; K = 8 with one
    image, where the rollback rewrites the image behind the two-barrier step;
    the work-group shapes of test_phi4_ens_shapes.GPU_SHAPES beyond those."""
    assert_shape(shape)
    refs = [_ref(shape, r) for r in range(3)]
    assert refs[0]["stable"].any() and not refs[0]["stable"].all(), refs[0]["stable"]
    assert refs[1]["stable"].all()            # Δτ₀ = 0.01 never rolls back: three Δτ / 0.95 in 40 frames
    assert refs[1]["dtau"][-1] == 0.01 / 0.950 / 0.950 / 0.950
    with _recipe(shape) as E:
        st, dt = E.run_frames(NFR)
        assert st.shape == dt.shape == (NFR, 3) and st.dtype == bool
        for r in range(3):
            _check(E, st, dt, r, refs[r], str(shape))
            assert int(E.step_counter[r]) == STEP0[r] + NFR * LOOPS
        # executed steps: every frame of the never-failing replica in full, of the others at least one step each
        p = E.perf()
        assert p["kernel_launches"] == 1
        assert NFR * LOOPS + 2 * NFR <= p["steps"] <= 3 * NFR * LOOPS


@pytest.mark.parametrize("shape", [(16, 4, 31), (32, 32, 32), (64, 3, 43), (64, 11, 29)])
def test_split_calls_and_raw_steps_between(gpu, shape):
    assert_shape(shape)
    refs = [_ref(shape, r) for r in range(3)]
    assert refs[0]["stable"].any() and not refs[0]["stable"].all()
    with _recipe(shape) as E:
        st, dt = E.run_frames(7)
        parts_s, parts_d = [st], [dt]
        for _ in range(3):
            ok = E.run_frame()
            assert ok.shape == (3,) and ok.dtype == bool
            parts_s.append(ok[None, :])
            parts_d.append(E.dtau[None, :])
        s2, d2 = E.run_frames(0)
        assert s2.shape == (0, 3) and d2.shape == (0, 3)
        s3, d3 = E.run_frames(30)
        st, dt = np.concatenate(parts_s + [s3]), np.concatenate(parts_d + [d3])
        for r in range(3):
            _check(E, st, dt, r, refs[r], f"{shape} split")
    # raw steps at the adapted Δτ between two frames calls
    with _recipe(shape) as E:
        sa, da = E.run_frames(9)
        E.step(5)
        sb, db = E.run_frames(9)
        st, dt = np.concatenate([sa, sb]), np.concatenate([da, db])
        for r in range(3):
            with _lat(shape, dtau=DTAU0[r], seed=SEEDS[r]) as L:
                L.init_field(0.3)
                L.step_counter = STEP0[r]
                ra, rda = L.run_frames(9)
                L.step(5)
                rb, rdb = L.run_frames(9)
                ref = _state(L, np.concatenate([ra, rb]), np.concatenate([rda, rdb]))
            assert ref["step"] == STEP0[r] + 18 * LOOPS + 5
            _check(E, st, dt, r, ref, f"{shape} step between")


@pytest.mark.parametrize("shape", [(8, 8, 8), (32, 32, 32)])
def test_rule_only_rollback_vs_oracle(gpu, oracle_mod, shape):
    """test_stability_rule_rolls_back_diverging_unclamped_field's recipe: C = 0,
    Δτ = 0.2 above the Euler limit diverges as an oscillation far below the
    clamp, so only the rule can reject the frame; a stable replica (Δτ = 0.01)
    beside it in the same launch runs its 12 steps."""
    h = 0.2
    p = oracle_mod.phi4_params(shape, h, 1.0, 1.0, 1234, C=0.0)
    phi0 = oracle_mod.phi4_init(p, 0.05)
    T0, V0 = float(phi0.max()), float(np.abs(phi0).max())
    out, M, D, A, fired, T1, V1 = oracle_mod.phi4_frame_stab(p, phi0, LOOPS, 0, T0, V0)
    assert fired >= 0 and np.abs(out).max() < 1000            # diverging, never clamped
    q = oracle_mod.phi4_params(shape, 0.01, 1.0, 1.0, 1234, C=0.0)
    quiet = phi0
    for s in range(LOOPS):
        quiet = oracle_mod.phi4_step(q, quiet, s)
    with _ens(shape, 2, dtau=[h, 0.01], C=0.0, seeds=[1234, 1234]) as E:
        E.upload(phi0)
        ok = E.run_frame()
        assert list(ok) == [False, True]
        st = E.stability()
        n = fired + 1
        assert st["fired"][0] == fired and st["T"][0] == T1 and st["V"][0] == V1
        assert np.array_equal(st["M"][0][:n], M[:n]) and np.array_equal(st["D"][0][:n], D[:n])
        assert np.array_equal(st["A"][0][:n], A[:n])
        assert st["fired"][1] == -1
        got = E.download()
        assert np.array_equal(got[0], phi0)                   # rolled back
        assert np.array_equal(got[1], quiet)
        dt = E.dtau
        assert dt[0] == h * 0.950 and dt[1] == 0.01
        assert list(E.step_counter) == [LOOPS, LOOPS]         # a retried frame draws fresh noise
        assert not E.flags().any()
        assert E.perf()["steps"] == n + LOOPS                 # the rejected frame stopped at the firing step


@pytest.mark.parametrize("shape", [(16, 4, 31), (8, 17, 31), (64, 3, 43)])
def test_negative_maximum_vs_oracle(gpu, oracle_mod, shape):
    """A field whose maximum is negative: the step's record takes atomic maxima
    of ordered keys over LDS words that start at 0, the wave's running maximum
    starts at -inf, and a lane without a quad carries mp = 0, above every site
    here.  K = 1 with a partial wave, K = 2 and K = 4 with waves that have such
    lanes.  C = 0, so the oracle's frame (oracle.phi4_frame_stab) is the
    reference bit for bit: two frames, the second from the carried negative T;
    a mixed-sign replica beside it in the same launch is checked the same way."""
    assert_shape(shape)
    h = 0.01
    p = [oracle_mod.phi4_params(shape, h, 1.0, 1.0, s, C=0.0) for s in (1234, 99)]
    phi = [-2.0 - np.abs(oracle_mod.phi4_init(p[0], 0.3)), oracle_mod.phi4_init(p[1], 0.3)]
    assert phi[0].dtype == np.float32 and phi[0].max() < 0 and phi[1].max() > 0 > phi[1].min()
    T = [float(f.max()) for f in phi]                         # a replica's first frame takes T, V from its start field
    V = [float(np.abs(f).max()) for f in phi]
    with _ens(shape, 2, dtau=h, C=0.0, seeds=[1234, 99]) as E:
        E.upload(np.stack(phi))
        for frame in range(2):
            ok = E.run_frame()
            st = E.stability()
            got = E.download()
            assert list(E.dtau) == [h, h] and not E.flags().any()
            for r in range(2):
                out, M, D, A, fired, T1, V1 = oracle_mod.phi4_frame_stab(p[r], phi[r], LOOPS, frame * LOOPS, T[r], V[r])
                tag = (shape, frame, r)
                assert fired < 0, tag                         # Δτ = 0.01 is far below the Euler limit
                if r == 0:
                    assert np.all(M < 0) and T1 < 0 and out.max() < 0, tag      # negative through all 12 steps
                assert bool(ok[r]) and st["fired"][r] == -1, tag
                assert st["T"][r] == T1 and st["V"][r] == V1, (tag, st["T"][r], T1, st["V"][r], V1)
                for k, ref in (("M", M), ("D", D), ("A", A)):
                    assert np.array_equal(st[k][r], ref), (tag, k, st[k][r], ref)
                assert np.array_equal(got[r], out), tag
                phi[r], T[r], V[r] = out, T1, V1
        assert list(E.step_counter) == [2 * LOOPS, 2 * LOOPS]


def test_adapt_dtau_off(gpu):
    shape, nfr = (16, 4, 31), 20
    refs = [_ref(shape, r, adapt=False, nfr=nfr) for r in range(3)]
    assert not refs[0]["stable"].all()
    with _recipe(shape, adapt_dtau=False) as E:
        st, dt = E.run_frames(nfr)
        assert np.array_equal(dt, np.broadcast_to(np.array(DTAU0), (nfr, 3)))
        for r in range(3):
            _check(E, st, dt, r, refs[r], "adapt off")


def test_set_stability_round_trip_and_guard_only_rollback(gpu):
    shape = (8, 8, 8)
    big = 1e30
    with _recipe(shape) as E:
        before = E.stability(n=0)
        assert before["M"].shape == (3, 0) and list(before["fired"]) == [-1, -1, -1]
        E.set_stability([1.5, 2.5, 3.5], [4.0, 5.0, 6.0])
        st = E.stability(n=0)
        assert list(st["T"]) == [1.5, 2.5, 3.5] and list(st["V"]) == [4.0, 5.0, 6.0]
        E.set_stability(7.0, 8.0, first=1, count=1)
        st = E.stability(n=0)
        assert list(st["T"]) == [1.5, 7.0, 3.5] and list(st["V"]) == [4.0, 8.0, 6.0]
        # T and V so large that the rule never fires: only the guard rejects frames
        E.set_stability(big, big)
        ok, dt = E.run_frames(NFR)
        fired = E.stability()["fired"]
        assert list(fired) == [-1, -1, -1]
        for r in range(3):
            with _lat(shape, dtau=DTAU0[r], seed=SEEDS[r]) as L:
                L.init_field(0.3)
                L.step_counter = STEP0[r]
                L.set_stability(big, big)
                rs, rd = L.run_frames(NFR)
                assert L.stability()["fired"] == -1
                assert np.array_equal(ok[:, r], rs) and np.array_equal(dt[:, r], rd), r
                assert np.array_equal(E.download(first=r, count=1)[0], L.download()), r
    # a guard-only rollback from an uploaded field with a NaN and a site far above the clamp
    with _ens(shape, 2, dtau=0.01, seeds=[5, 6]) as E:
        E.init_field(0.3)
        phi0 = E.download()
        phi0[1, 6, 1, 2] = np.float32("nan")
        phi0[1, 3, 4, 5] = np.float32(1e6)
        E.upload(phi0)
        E.set_stability(big, big)
        ok = E.run_frame()
        assert list(ok) == [True, False]
        got = E.download()
        assert np.array_equal(got[1].view(np.uint32), phi0[1].view(np.uint32))    # restored, the NaN included
        assert not np.array_equal(got[0], phi0[0])
        assert list(E.flags()) == [False, True]
        assert list(E.stability()["fired"]) == [-1, -1]
        assert list(E.dtau) == [0.01, 0.01 * 0.950]


def _exact_sums(phi):
    """Exactly rounded S1, S2, S4, NN of one lattice and per sum the bound 2 n u sum |terms|."""
    a = phi.astype(np.float64)
    a2 = a * a                                     # exact: 24-bit factors
    links = np.concatenate([(a * np.roll(a, -1, axis=ax)).ravel() for ax in (2, 1, 0)])   # exact
    terms = [a.ravel(), a2.ravel(), (a2 * a2).ravel(), links]
    u = 2.0 ** -53
    return (np.array([math.fsum(t) for t in terms]),
            np.array([2 * t.size * u * math.fsum(np.abs(t)) for t in terms]))


@pytest.mark.parametrize("shape", [(16, 4, 31), (32, 32, 32)] + MEASURED)
def test_measure_rows(gpu, shape):
    assert_shape(shape)
    names = ("S1", "S2", "S4", "NN")
    with _recipe(shape) as E, _recipe(shape) as Tw:
        st, dt, ser = E.run_frames(NFR, measure=True)
        assert ser.shape == (NFR, 3, 4)
        m = Tw.moments()
        prev = np.stack([m[k] for k in names], axis=1)
        rolled = 0
        for f in range(NFR):
            ok = Tw.run_frame()
            assert np.array_equal(ok, st[f])
            m = Tw.moments()
            row = np.stack([m[k] for k in names], axis=1)
            assert np.array_equal(ser[f], row), f            # the same code on the same field
            for r in range(3):
                if not st[f, r]:
                    rolled += 1
                    assert np.array_equal(ser[f, r], prev[r]), (f, r)
            prev = row
        assert rolled > 0
        field = E.download()
        assert np.array_equal(field, Tw.download())          # measuring changes nothing
        for r in range(3):
            s, b = _exact_sums(field[r])
            assert np.all(np.abs(ser[-1, r] - s) <= b), (r, ser[-1, r], s, b)
    for r in range(3):
        assert np.array_equal(st[:, r], _ref(shape, r)["stable"])


def test_independent_of_replica_count_and_position(gpu):
    """More work-groups than CUs, some leaving frames early while others run on."""
    shape, R, nfr = (8, 8, 8), 300, 20
    seeds = [1000 + 7 * i for i in range(R)]
    seeds[299] = 99
    with _ens(shape, R, dtau=0.19, seeds=seeds) as A, _ens(shape, 1, dtau=0.19, seeds=[99]) as B:
        for E in (A, B):
            E.init_field(0.3)
        sa, da = A.run_frames(nfr)
        sb, db = B.run_frames(nfr)
        assert sb[:, 0].any() and not sb[:, 0].all()
        assert (sa.any(axis=1) & ~sa.all(axis=1)).any()        # some frame is stable for some replicas only
        assert np.array_equal(sa[:, 299], sb[:, 0]) and np.array_equal(da[:, 299], db[:, 0])
        assert np.array_equal(A.download(first=299, count=1), B.download())
        x, y = A.stability(first=299, count=1), B.stability()
        for k in ("T", "V", "fired"):
            assert x[k][0] == y[k][0], k
        n = LOOPS if y["fired"][0] < 0 else y["fired"][0] + 1
        for k in ("M", "D", "A"):
            assert np.array_equal(x[k][0][:n], y[k][0][:n]), k
        assert A.perf()["steps"] < R * nfr * LOOPS             # some frame somewhere exited early


def test_argument_errors(gpu):
    from stochquant_amd import StochQuantError
    with _ens((8, 8, 8), 2, dtau=0.01, loops=0) as E:         # accepted at creation, refused by the frames call
        E.init_field(0.3)
        with pytest.raises(StochQuantError) as ei:
            E.run_frames(1)
        assert ei.value.code == -1
        E.step(1)
    with _ens((8, 8, 8), 2, dtau=0.01, loops=4) as E:
        with pytest.raises(StochQuantError):
            E.run_frames(-1)
        with pytest.raises(StochQuantError):
            E.stability(n=1)                                   # no frame has run
        E.init_field(0.3)
        assert E.run_frame().all()
        with pytest.raises(StochQuantError):
            E.stability(n=5)
        with pytest.raises(StochQuantError):
            E.stability(first=1, count=2)
        with pytest.raises(StochQuantError):
            E.set_stability(1.0, 1.0, first=2, count=1)
        assert E.stability(n=2)["M"].shape == (2, 2)
