"""Heun frames of the phi^4 lattice ensemble on the GPU (phi4_ens_heun_frames_kernel,
sq_phi4_ens_run_frames_heun, Phi4Ensemble.run_frames(scheme="heun")).

The reference is composed here from entries the oracle already has, in device-transcendental
mode: oracle.phi4_heun_step for phi' and the three guarded maxima; orc_normals4_q and
orc_phi4_sigq (through ctypes) for the normal and the amplitude at the sites attaining the
step's maximum; libm's fmaf (through ctypes) for the record's one fused operation;
orc_phi4_stab_rule for the rule; and a Python restatement of the controller (frame_decide)
and of phi4_base_args' float conversions.  The record of a Heun step, as the header states it:
M = max phi', D = the largest over the sites attaining M of |fmaf(-sigq, xi, phi' - phi)| with
phi the step's input, A = max(max |p|, max |e|, max |phi'|).

Tolerances: bit for bit everywhere (fields, verdicts, the doubles of dtau, T, V, the firing
step, the records through it, counters, accumulators, measured rows).
"""
import ctypes
import ctypes.util

import numpy as np
import pytest

from test_oracle import same_bits
from test_phi4_ens_shapes import assert_shape

pytestmark = pytest.mark.gpu

CLAMP = 1000.0
# one replica each: always stable; noise off and far above the linear limit, where the Heun amplification
# 1 - x + x^2 / 2 of the fastest mode exceeds 2 and the increment at the maximum outgrows every earlier |phi|
# within a few steps, long before the clamp (the rule alone fires); so large that stage 2's cubic term passes
# the clamp in the first step (a guard trip); noise on near the limit
DTAU = [0.01, 0.3, 3.0, 0.19]
M2 = [1.0, 0.5, 1.0, 0.8]
LAM = [1.0, 0.8, 1.0, 1.3]
CN = [1.0, 0.0, 1.0, 0.7]
SEEDS = [99, 1234, 0xDEADBEEF12345, 7]
STEP0 = [0, 2 ** 32 - 2, 5, 2 ** 40 + 5]      # replica 1's counter carries into the high word in its first frame
AMP = [0.3, 0.05, 0.3, 0.3]
R = 4
LOOPS, NFR = 5, 3
# every work-group class that differs in code: one wave with lanes that own no quad; a partial wave; K = 2;
# K = 4 with empty waves; K = 8 with two images; K = 8 with one image and missing quads; a plane of four quads
SHAPES = [(8, 2, 2), (16, 4, 31), (64, 16, 8), (64, 3, 43), (8, 50, 51), (64, 11, 29), (8, 2, 2048)]

_cache = {}
_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float] * 3


def _ens(shape, adapt=True, loops=LOOPS, **kw):
    from stochquant_amd import Phi4Ensemble
    kw.setdefault("dtau", DTAU)
    return Phi4Ensemble(shape, R, m2=M2, lam=LAM, C=CN, seeds=SEEDS, clamp=CLAMP, loops=loops,
                        adapt_dtau=adapt, **kw)


class Replica:
    """One replica of the composed oracle: its snapshot, counter, dtau and the rule's carried state."""

    def __init__(self, o, shape, r, dtau=None, adapt=True, loops=LOOPS):
        self.o, self.shape, self.r, self.adapt, self.loops = o, shape, r, adapt, loops
        self.dtau = float(DTAU[r] if dtau is None else dtau)
        self.step, self.cnt = STEP0[r], 0
        self.T = self.V = None                      # taken from the start field at the first frame
        self.fired, self.flag, self.sticky, self.executed = -1, 0, False, 0
        self.rec = None
        L = o.lib()
        L.orc_normals4_q.restype = None
        L.orc_normals4_q.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_uint64,
                                     ctypes.POINTER(ctypes.c_float)]
        L.orc_phi4_sigq.restype = ctypes.c_float
        L.orc_phi4_sigq.argtypes = [ctypes.c_float, ctypes.c_double]
        self.phi = o.phi4_init(self._params(), AMP[r])

    def _params(self):
        # phi4_base_args: h = (float)dtau; the oracle derives lam6, sig and sigq from the floats as the product does
        return self.o.phi4_params(self.shape, np.float32(self.dtau), M2[self.r], LAM[self.r], SEEDS[self.r],
                                  clamp=CLAMP, C=CN[self.r])

    def _record(self, p, phi, out, mx, step):
        L = self.o.lib()
        sigq = L.orc_phi4_sigq(p.h, p.C)
        a, b = out.ravel(), phi.ravel()
        M = a.max()
        D = np.float32(0.0)
        xi = (ctypes.c_float * 4)()
        for s in np.flatnonzero(a == M):
            L.orc_normals4_q(p.seed, 0, int(s) >> 2, step, xi)
            d = np.float32(abs(_libm.fmaf(-sigq, xi[int(s) & 3], np.float32(a[s] - b[s]))))
            D = max(D, d)
        return np.float32(M), np.float32(D), np.float32(max(mx))

    def heun_steps(self, n):
        """n raw Heun steps (Phi4Ensemble.step(n, scheme="heun")): the rule's state stays."""
        p = self._params()
        for k in range(n):
            self.phi, mx = self.o.phi4_heun_step(p, self.phi, self.step + k)
            self.sticky = self.sticky or max(mx) >= CLAMP
        self.step += n

    def euler_steps(self, n):
        p = self._params()
        for k in range(n):
            self.phi = self.o.phi4_step(p, self.phi, self.step + k)
            self.sticky = self.sticky or np.abs(self.phi).max() >= CLAMP     # some site was clamped
        self.step += n

    def frame(self):
        """One Heun frame; returns the verdict."""
        o, n = self.o, self.loops
        if self.T is None:
            self.T, self.V = np.float32(self.phi.max()), np.float32(np.abs(self.phi).max())
        p = self._params()
        T, V = (np.array([x], np.float32) for x in (self.T, self.V))
        rec = np.zeros((3, n), np.float32)
        cur, fired, flag, ex = self.phi, -1, 0, 0
        fp = ctypes.POINTER(ctypes.c_float)
        for t in range(n):
            out, mx = o.phi4_heun_step(p, cur, self.step + t)
            rec[:, t] = self._record(p, cur, out, mx, self.step + t)
            cur, ex = out, ex + 1
            if rec[2, t] >= CLAMP:
                flag = 1
            if o.lib().orc_phi4_stab_rule(T.ctypes.data_as(fp), V.ctypes.data_as(fp), rec[0, t:].ctypes.data_as(fp),
                                          rec[1, t:].ctypes.data_as(fp), rec[2, t:].ctypes.data_as(fp), 1) == 0:
                fired = t
                break
        self.T, self.V = T[0], V[0]
        stable = flag == 0 and fired < 0
        if self.adapt:                              # frame_decide
            if stable:
                if self.cnt > 10:
                    self.cnt = 0
                    self.dtau /= 0.950
                self.cnt += 1
            else:
                self.dtau *= 0.950
                self.cnt = 0
        if stable:
            self.phi = cur
        self.step += n
        self.fired, self.flag, self.rec = fired, flag, rec
        self.sticky = self.sticky or bool(flag)
        self.executed += ex
        return stable


def _oracle_frames(o, shape):
    """NFR frames of the R replicas on the composed oracle, once per shape: per frame and replica the verdict,
    dtau, field, T, V, firing step, guard flag and records; and what the case must show."""
    key = ("frames", shape)
    if key not in _cache:
        reps = [Replica(o, shape, r) for r in range(R)]
        start = np.stack([x.phi for x in reps])
        log = []
        for f in range(NFR):
            row = []
            for x in reps:
                st = x.frame()
                row.append(dict(stable=st, dtau=x.dtau, phi=x.phi, T=x.T, V=x.V, fired=x.fired, flag=x.flag,
                                rec=x.rec, n=LOOPS if x.fired < 0 else x.fired + 1))
            log.append(row)
        start.setflags(write=False)
        _cache[key] = (start, log, [x.executed for x in reps], [x.sticky for x in reps])
    return _cache[key]


def _assert_case_is_telling(log):
    """On the oracle's output alone: a stable frame, a rule-only firing before the last step and a guard trip."""
    rows = [e for row in log for e in row]
    assert any(e["stable"] for e in rows)
    assert any(0 <= e["fired"] < LOOPS - 1 and e["flag"] == 0 for e in rows), [(e["fired"], e["flag"]) for e in rows]
    assert any(e["flag"] == 1 for e in rows)


def _check_state(E, row, tag):
    s = E.stability()
    got = E.download()
    for r, e in enumerate(row):
        t = (tag, r)
        assert same_bits(got[r], e["phi"]), (t, int(np.count_nonzero(got[r] != e["phi"])))
        assert np.float32(s["T"][r]) == e["T"] and np.float32(s["V"][r]) == e["V"], (t, s["T"][r], e["T"], s["V"][r], e["V"])
        assert s["fired"][r] == e["fired"], (t, s["fired"][r], e["fired"])
        for k, name in enumerate(("M", "D", "A")):
            a, b = s[name][r][:e["n"]], e["rec"][k][:e["n"]]
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (t, name, a, b)


@pytest.mark.parametrize("shape", SHAPES)
def test_frames_bitwise_against_the_composed_oracle(gpu, dev_oracle, shape):
    assert_shape(shape)
    start, log, executed, sticky = _oracle_frames(dev_oracle, shape)
    _assert_case_is_telling(log)
    want_st = np.array([[e["stable"] for e in row] for row in log])
    want_dt = np.array([[e["dtau"] for e in row] for row in log])
    # one launch for the three frames
    with _ens(shape) as E:
        E.upload(start)
        E.step_counter = STEP0
        st, dt = E.run_frames(NFR, scheme="heun")
        assert st.shape == dt.shape == (NFR, R) and st.dtype == bool
        assert np.array_equal(st, want_st), (st, want_st)
        assert np.array_equal(dt.view(np.uint64), want_dt.view(np.uint64)), (dt, want_dt)
        _check_state(E, log[-1], (shape, "one launch"))
        assert [int(s) for s in E.step_counter] == [s + NFR * LOOPS for s in STEP0]   # whatever the verdicts
        assert list(E.flags()) == sticky
        assert np.array_equal(E.dtau.view(np.uint64), want_dt[-1].view(np.uint64))
        p = E.perf()
        assert p["kernel_launches"] == 1 and p["steps"] == sum(executed), (p, executed)   # exec, through the exits
    # frame by frame: the records, T, V and the field after every frame
    with _ens(shape) as E:
        E.upload(start)
        E.step_counter = STEP0
        for f in range(NFR):
            ok = E.run_frame(scheme="heun")
            assert np.array_equal(ok, want_st[f]), (f, ok)
            assert np.array_equal(E.dtau.view(np.uint64), want_dt[f].view(np.uint64)), f
            _check_state(E, log[f], (shape, f))


def test_adapt_off_all_stable_equals_raw_heun_steps(gpu):
    """adapt_dtau = 0 and every frame stable: run_frames(n, heun) leaves the bits and counters of step(n loops, heun)."""
    shape, n = (16, 4, 31), 4
    assert_shape(shape)
    with _ens(shape, adapt=False, dtau=[0.01, 0.02, 0.015, 0.01]) as A, \
            _ens(shape, adapt=False, dtau=[0.01, 0.02, 0.015, 0.01]) as B:
        for E in (A, B):
            E.init_field(0.3)
            E.step_counter = STEP0
        st, dt = A.run_frames(n, scheme="heun")
        assert st.all() and np.array_equal(dt, np.broadcast_to([0.01, 0.02, 0.015, 0.01], (n, R)))
        B.step(n * LOOPS, scheme="heun")
        assert same_bits(A.download(), B.download())
        assert list(A.step_counter) == list(B.step_counter) == [s + n * LOOPS for s in STEP0]
        assert not A.flags().any() and not B.flags().any()
        assert A.perf()["steps"] == B.perf()["steps"] == R * n * LOOPS


@pytest.mark.parametrize("shape", [(16, 4, 31), (64, 11, 29)])
def test_split_calls(gpu, shape):
    """2 + 1 frames against 3 in one launch: verdicts, dtau, fields, the carried state and the last records."""
    assert_shape(shape)
    with _ens(shape) as A, _ens(shape) as B:
        for E in (A, B):
            E.init_field(0.3)
            E.step_counter = STEP0
        sa, da = A.run_frames(3, scheme="heun")
        s1, d1 = B.run_frames(2, scheme="heun")
        s2, d2 = B.run_frames(1, scheme="heun")
        s0, d0 = B.run_frames(0, scheme="heun")
        assert s0.shape == d0.shape == (0, R)
        assert np.array_equal(sa, np.concatenate([s1, s2])) and np.array_equal(da, np.concatenate([d1, d2]))
        assert not sa.all() and sa.any()
        assert same_bits(A.download(), B.download())
        x, y = A.stability(), B.stability()
        for k in ("T", "V", "fired"):
            assert np.array_equal(x[k], y[k]), k
        for r in range(R):
            n = LOOPS if y["fired"][r] < 0 else y["fired"][r] + 1
            for k in ("M", "D", "A"):
                assert np.array_equal(x[k][r][:n].view(np.uint32), y[k][r][:n].view(np.uint32)), (r, k)
        assert list(A.step_counter) == list(B.step_counter)
        assert list(A.flags()) == list(B.flags())


def test_schemes_interleaved_on_one_handle(gpu, dev_oracle):
    """Heun frame, Euler frame, raw Heun steps, raw Euler steps, Heun frame on one handle against the same
    sequence on the oracle: T, V, the controller's count and dtau are shared.  The Euler frame's reference is
    the oracle's own (phi4_frame_stab) under the same controller."""
    shape = (16, 4, 31)
    assert_shape(shape)
    o = dev_oracle
    reps = [Replica(o, shape, r) for r in range(R)]
    start = np.stack([x.phi for x in reps])

    def euler_frame(x):
        p = x._params()
        out, M, D, A, fired, T1, V1 = o.phi4_frame_stab(p, x.phi, LOOPS, x.step, x.T, x.V)
        n = LOOPS if fired < 0 else fired + 1
        flag = bool(np.any(A[:n] >= CLAMP))
        stable = fired < 0 and not flag
        x.T, x.V = np.float32(T1), np.float32(V1)   # frozen at the firing step by the rule itself
        if stable:
            if x.cnt > 10:
                x.cnt = 0
                x.dtau /= 0.950
            x.cnt += 1
            x.phi = out
        else:
            x.dtau *= 0.950
            x.cnt = 0
        x.step += LOOPS
        x.fired = fired
        x.sticky = x.sticky or flag
        return stable

    with _ens(shape) as E:
        E.upload(start)
        E.step_counter = STEP0
        want = []
        got = [E.run_frame(scheme="heun")]
        want.append([x.frame() for x in reps])
        got.append(E.run_frame())
        want.append([euler_frame(x) for x in reps])
        E.step(2, scheme="heun")
        E.step(3)
        for x in reps:
            x.heun_steps(2)
            x.euler_steps(3)
        got.append(E.run_frame(scheme="heun"))
        want.append([x.frame() for x in reps])
        assert [list(g) for g in got] == want, (got, want)
        assert np.array_equal(E.dtau.view(np.uint64), np.array([x.dtau for x in reps]).view(np.uint64))
        f = E.download()
        for r, x in enumerate(reps):
            assert same_bits(f[r], x.phi), r
        s = E.stability()
        assert [np.float32(t) for t in s["T"]] == [x.T for x in reps]
        assert [np.float32(v) for v in s["V"]] == [x.V for x in reps]
        assert list(s["fired"]) == [x.fired for x in reps]
        assert [int(c) for c in E.step_counter] == [x.step for x in reps]
        assert list(E.flags()) == [x.sticky for x in reps]


def test_set_stability_and_guard_only_rollback(gpu):
    shape, big = (8, 8, 8), 1e30
    with _ens(shape) as E:
        E.init_field(0.3)
        E.set_stability([1.5, 2.5, 3.5, 4.5], [4.0, 5.0, 6.0, 7.0])
        st = E.stability(n=0)
        assert list(st["T"]) == [1.5, 2.5, 3.5, 4.5] and list(st["V"]) == [4.0, 5.0, 6.0, 7.0]
        # T and V so large that the rule never fires: the frames run all their steps, only the guard rejects
        E.set_stability(big, big)
        ok, dt = E.run_frames(2, scheme="heun")
        assert list(E.stability()["fired"]) == [-1] * R
        assert list(ok[:, 0]) == [True, True] and list(ok[:, 2]) == [False, False]      # dtau = 0.01; dtau = 3
        assert E.perf()["steps"] == 2 * R * LOOPS
    # one over-range site: an unstable frame, the field restored bit for bit, dtau cut
    with _ens(shape, dtau=0.01) as E:
        E.init_field(0.3)
        phi0 = E.download()
        phi0[1, 3, 4, 5] = np.float32(1e6)
        E.upload(phi0)
        E.set_stability(big, big)
        ok = E.run_frame(scheme="heun")
        assert list(ok) == [True, False, True, True]
        got = E.download()
        assert same_bits(got[1], phi0[1])
        for r in (0, 2, 3):
            assert not np.array_equal(got[r], phi0[r])
        assert list(E.flags()) == [False, True, False, False]
        assert list(E.stability()["fired"]) == [-1] * R
        assert list(E.dtau) == [0.01, 0.01 * 0.950, 0.01, 0.01]
        assert [int(s) for s in E.step_counter] == [LOOPS] * R


def test_independent_of_replica_count_and_position(gpu):
    """R = 300 at 8^3, more work-groups than CUs, some leaving frames early: three picked replicas against R = 1 runs."""
    from stochquant_amd import Phi4Ensemble
    shape, n, nfr = (8, 8, 8), 300, 6
    seeds = [1000 + 7 * i for i in range(n)]
    dtau = [0.19 if i % 3 else 0.01 for i in range(n)]
    with Phi4Ensemble(shape, n, dtau=dtau, seeds=seeds, loops=LOOPS) as A:
        A.init_field(0.3)
        sa, da = A.run_frames(nfr, scheme="heun")
        assert (sa.any(axis=1) & ~sa.all(axis=1)).any()
        assert A.perf()["steps"] < n * nfr * LOOPS                # some frame somewhere exited early
        for i in (0, 157, 299):
            with Phi4Ensemble(shape, 1, dtau=dtau[i], seeds=[seeds[i]], loops=LOOPS) as B:
                B.init_field(0.3)
                sb, db = B.run_frames(nfr, scheme="heun")
                assert np.array_equal(sa[:, i], sb[:, 0]) and np.array_equal(da[:, i], db[:, 0]), i
                assert same_bits(A.download(first=i, count=1), B.download()), i
                x, y = A.stability(first=i, count=1), B.stability()
                for k in ("T", "V", "fired"):
                    assert x[k][0] == y[k][0], (i, k)
                m = LOOPS if y["fired"][0] < 0 else y["fired"][0] + 1
                for k in ("M", "D", "A"):
                    assert np.array_equal(x[k][0][:m].view(np.uint32), y[k][0][:m].view(np.uint32)), (i, k)


MODES = {"correlate": (True, False), "momenta": (False, True), "both": (True, True)}
MOMS = [(0, 0), (1, 0), (1, 1)]
# K = 1; K = 4; K = 8 with two images in every launch; K = 8 with one; and 8 x 2 x 2048, K = 8 with one image,
# whose LDS cannot hold the momentum projections: its momentum modes assert the refusal
MEASURED = [(16, 4, 31), (64, 3, 43), (32, 24, 24), (64, 11, 29), (8, 2, 2048)]


@pytest.mark.parametrize("shape", [(16, 4, 31), (64, 11, 29)])
def test_measure_rows(gpu, shape):
    """measure=True rows bit for bit moments() of the adopted fields; a rolled-back frame repeats the row before."""
    assert_shape(shape)
    names = ("S1", "S2", "S4", "NN")
    with _ens(shape) as E, _ens(shape) as Tw:
        for X in (E, Tw):
            X.init_field(0.3)
        st, dt, ser = E.run_frames(NFR, measure=True, scheme="heun")
        assert ser.shape == (NFR, R, 4)
        m = Tw.moments()
        prev = np.stack([m[k] for k in names], axis=1)
        for f in range(NFR):
            assert np.array_equal(Tw.run_frame(scheme="heun"), st[f])
            m = Tw.moments()
            row = np.stack([m[k] for k in names], axis=1)
            assert np.array_equal(ser[f].view(np.uint64), row.view(np.uint64)), f
            for r in range(R):
                if not st[f, r]:
                    assert np.array_equal(ser[f, r], prev[r]), (f, r)
            prev = row
        assert not st.all() and st.any()
        assert same_bits(E.download(), Tw.download())               # measuring changes nothing


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", MEASURED)
def test_correlators_after_stable_frames_only(gpu, shape, mode):
    """The accumulators bit for bit the sums of slices() / pslices() taken after the same frames on a twin that
    measures nothing in flight, over the stable frames only: nmeas equals the count of stable verdicts."""
    from stochquant_amd import Phi4Ensemble, StochQuantError
    assert_shape(shape)
    corr, mom = MODES[mode]
    mask = Phi4Ensemble.heun_frames_shape_info(shape)["measure_mask"]
    with _ens(shape) as E, _ens(shape) as Tw:
        for X in (E, Tw):
            X.init_field(0.3)
        if not (mask >> (int(corr) | 2 * int(mom))) & 1:
            assert mom                                               # only momenta can be refused: no LDS for them
            with pytest.raises(StochQuantError):
                E.set_momenta(MOMS)
            with pytest.raises(StochQuantError):
                E.run_frames(1, correlate=corr, momenta=True, scheme="heun")
            return
        if mask & 4:                                                 # the shape can hold momenta
            for X in (E, Tw):
                X.set_momenta(MOMS)
        nt = E.nt
        st, dt = E.run_frames(NFR, correlate=corr, momenta=mom, scheme="heun")
        G, S1, Gp = np.zeros((R, nt)), np.zeros(R), np.zeros((R, len(MOMS), nt))
        for f in range(NFR):
            assert np.array_equal(Tw.run_frame(scheme="heun"), st[f])
            S, g = Tw.slices()
            gp = Tw.pslices()[1] if mom else None
            for r in range(R):
                if st[f, r]:
                    if corr:
                        G[r] = G[r] + g[r]
                        s1 = 0.0
                        for z in range(shape[2]):
                            s1 = s1 + S[r, z]
                        S1[r] = S1[r] + s1
                    if mom:
                        Gp[r] = Gp[r] + gp[r]
        assert not st.all() and st.any()
        aG, aS1, aN = E.corr_sums()
        aGp, aNp = E.pcorr_sums()
        if not mask & 4:
            Gp = Gp[:, :0]                                           # no momenta set: empty rows
        nst = st.sum(axis=0)
        assert list(aN) == list(nst * int(corr)) and list(aNp) == list(nst * int(mom))
        assert np.array_equal(aG.view(np.uint64), G.view(np.uint64))
        assert np.array_equal(aS1.view(np.uint64), S1.view(np.uint64))
        assert np.array_equal(aGp.view(np.uint64), Gp.view(np.uint64))
        assert same_bits(E.download(), Tw.download())


def test_euler_path_untouched(gpu):
    shape = (16, 4, 31)
    with _ens(shape) as A, _ens(shape) as B, _ens(shape) as H:
        for E in (A, B, H):
            E.init_field(0.3)
        sa, da = A.run_frames(3)
        sb, db = B.run_frames(3, scheme="euler")
        assert np.array_equal(sa, sb) and np.array_equal(da.view(np.uint64), db.view(np.uint64))
        assert same_bits(A.download(), B.download())
        H.run_frames(3, scheme="heun")
        assert not np.array_equal(A.download()[0], H.download()[0])  # the scheme reaches the kernel
