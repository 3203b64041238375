"""The phi^4 ensemble's Heun step (phi4_ens_heun_kernel, Phi4Ensemble.step(scheme="heun"),
sq_phi4_ens_step_heun) against the CPU oracle's Heun entry (oracle.phi4_heun_step,
orc_phi4_heun_step), which is written from the header's definition and shares no code with
the kernels, and at the kernel's edges:

  * every work-group shape with per-replica counters that differ, one of them above 2^32
    from the start;
  * the guard flag's three sources one at a time (max |p|, max |e|, max |phi'|);
  * every instance of the in-flight measurements (series only, correlator, momenta, both;
    series present or absent) at the K = 1 .. 8, one- and two-image shapes that have owned
    quads which do not exist;
  * Heun steps between two frames calls, at the adapted, per-replica step sizes;
  * the integrator's order on the interacting drift against a float64 solution.

Tolerances: fields, flags, counters, accumulators and verdicts bit for bit.  The series rows
against the oracle's field: the ensemble suite's 2 n u sum |t| (test_gpu_phi4_ens.py).  The
order test's bounds are derived at the test.
"""
import numpy as np
import pytest

from test_gpu_phi4_ens import _exact_sums
from test_gpu_phi4_ens_heun import C, CLAMP, DT, LAM, M2, SEEDS, _ens
from test_oracle import (HEUN_GUARD_IDS, HEUN_GUARD_PARAMS, ODE_LAM, ODE_M2, ODE_SHAPES, ODE_T, assert_heun_guard_maxima,
                         assert_ode_orders, heun_guard_field, ode_start_and_reference, same_bits)
from test_phi4_ens_shapes import GPU_SHAPES, assert_shape

pytestmark = pytest.mark.gpu

SHAPES = list(GPU_SHAPES)
COUNTERS = [0, 2 ** 32 - 2, 2 ** 40 + 5]      # one crosses into the high word during the call, one starts above it
NAMES = ("S1", "S2", "S4", "NN")

_cache = {}


def _gate(shape, want=None):
    """assert_shape for a shape of GPU_SHAPES; for another, `want` = (K, T, images, frames images) stated here."""
    if want is None:
        return assert_shape(shape)
    from stochquant_amd import Phi4Ensemble
    i = Phi4Ensemble.shape_info(shape)
    assert (i["K"], i["T"], i["images"], i["frames_images"]) == want, (shape, i)
    return i


def _params(o, shape, r):
    return o.phi4_params(shape, DT[r], M2[r], LAM[r], SEEDS[r], clamp=CLAMP, C=C[r])


def _starts(o, shape, amp=0.5):
    key = ("start", shape, amp)
    if key not in _cache:
        _cache[key] = np.stack([o.phi4_init(_params(o, shape, r), amp) for r in range(3)])
        _cache[key].setflags(write=False)
    return _cache[key]


def _oracle_heun(o, p, phi, s0, n):
    """n Heun steps of the oracle from counter s0: (the field after each step, the guard flag)."""
    fields, hit = [], False
    for k in range(n):
        phi, mx = o.phi4_heun_step(p, phi, s0 + k)
        hit = hit or any(m >= p.clampv for m in mx)
        fields.append(phi)
    return fields, hit


@pytest.mark.parametrize("shape", SHAPES)
def test_bitwise_against_the_oracle(gpu, dev_oracle, shape):
    assert_shape(shape)
    phi0 = _starts(dev_oracle, shape)
    with _ens(shape) as E:
        E.upload(phi0)
        E.step_counter = COUNTERS
        assert E.step(3, scheme="heun") is None
        got = E.download()
        assert [int(s) for s in E.step_counter] == [s + 3 for s in COUNTERS]
        flags = E.flags()
    for r in range(3):
        fields, hit = _oracle_heun(dev_oracle, _params(dev_oracle, shape, r), phi0[r], COUNTERS[r], 3)
        assert same_bits(got[r], fields[-1]), f"replica {r}: {np.count_nonzero(got[r] != fields[-1])} sites " \
                                              f"differ, max {np.max(np.abs(got[r] - fields[-1]))}"
        assert bool(flags[r]) == hit and not hit, (r, flags)


@pytest.mark.parametrize("case,shape", HEUN_GUARD_PARAMS, ids=HEUN_GUARD_IDS)
def test_guard_flag_stage_by_stage(gpu, oracle_mod, case, shape):
    """One Heun step of test_oracle.HEUN_GUARD_CASES in replica 0 (C = 0, clamp 1000): no maximum at the clamp,
    max |e| alone, max |p| and max |e|, max |p| alone.  A quiet replica 1 in the same launch keeps flag 0."""
    from stochquant_amd import Phi4Ensemble
    assert_shape(shape)
    dt, m2, lam = case[3]
    ps = [oracle_mod.phi4_params(shape, dt, m2, lam, s, clamp=CLAMP, C=0.0) for s in (1, 2)]
    phi0 = np.stack([heun_guard_field(case, shape), oracle_mod.phi4_init(ps[1], 0.5)])
    with Phi4Ensemble(shape, 2, dtau=dt, m2=m2, lam=lam, C=0.0, seeds=[1, 2], clamp=CLAMP) as E:
        E.upload(phi0)
        E.step(1, scheme="heun")
        got = E.download()
        flags = E.flags()
        assert list(E.step_counter) == [1, 1]
    ref = [oracle_mod.phi4_heun_step(ps[r], phi0[r], 0) for r in range(2)]
    assert_heun_guard_maxima(case, ref[0][1])
    assert max(ref[1][1]) < 10.0
    for r in range(2):
        assert same_bits(got[r], ref[r][0]), (case[0], r)
    assert list(flags) == [case[5], False], (case[0], flags, ref[0][1])


def _oracle_measured(o, shape):
    """6 Heun steps of the three replicas from _starts at counter 0 (device normals): the fields after steps 2, 4
    and 6 with their exactly rounded sums and bounds.  Once per shape."""
    key = ("measured", shape)
    if key not in _cache:
        phi0 = _starts(o, shape)
        recs = []
        for r in range(3):
            fields, hit = _oracle_heun(o, _params(o, shape, r), phi0[r], 0, 6)
            assert not hit
            recs.append([(fields[k],) + _exact_sums(fields[k])[:2] for k in (1, 3, 5)])
        _cache[key] = recs
    return _cache[key]


MODES = {"series": (False, False), "correlate": (True, False), "momenta": (False, True), "both": (True, True)}


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("shape", [(8, 3, 5), (64, 3, 43), (16, 32, 32), (8, 50, 51), (64, 11, 29), (32, 2, 321)])
def test_measurements_in_flight_each_instance(gpu, sqlib, dev_oracle, shape, mode):
    """step(6, every=2, heun) with the mode's measurements against a second ensemble that takes two unmeasured
    Heun steps and measures its stored field (moments / slices / pslices), three times: rows bit for bit, the
    accumulators the sequential sums, those the mode does not name zero with no measurement counted.  A third
    ensemble makes the mode's call without a series (the C entry; the instance's other branch) and must reach
    the same accumulators.  The rows and the final field also against the oracle's Heun fields."""
    _gate(shape, (1, 64, 2, 2) if shape == (8, 3, 5) else None)      # 8 x 3 x 5: one wave, 30 quads
    corr, mom = MODES[mode]
    moms = [(0, 0), (1, 0), (1, 1)]
    phi0 = _starts(dev_oracle, shape)
    recs = _oracle_measured(dev_oracle, shape)
    with _ens(shape) as A, _ens(shape) as B, _ens(shape) as N:
        for E in (A, B, N):
            E.upload(phi0)
            E.set_momenta(moms)
        nt = A.nt
        ser = A.step(6, every=2, correlate=corr, momenta=mom, scheme="heun")
        assert ser.shape == (3, 3, 4)
        G, S1, Gp = np.zeros((3, nt)), np.zeros(3), np.zeros((3, len(moms), nt))
        for m in range(3):
            B.step(2, scheme="heun")
            mo = B.moments()
            row = np.stack([mo[k] for k in NAMES], axis=1)
            assert np.array_equal(ser[m].view(np.uint64), row.view(np.uint64)), f"record {m}"
            for r in range(3):
                _, exact, bound = recs[r][m]
                err = np.abs(ser[m, r] - exact)
                assert np.all(err <= bound), (m, r, err, bound)
            if corr:
                S, g = B.slices()
                G = G + g
                s1 = np.zeros(3)
                for z in range(shape[2]):
                    s1 = s1 + S[:, z]
                S1 = S1 + s1
            if mom:
                Gp = Gp + B.pslices()[1]
        want_n, want_np = [3 * int(corr)] * 3, [3 * int(mom)] * 3

        def sums(E):
            aG, aS1, aN = E.corr_sums()
            aGp, aNp = E.pcorr_sums()
            assert np.array_equal(aG.view(np.uint64), G.view(np.uint64))
            assert np.array_equal(aS1.view(np.uint64), S1.view(np.uint64))
            assert np.array_equal(aGp.view(np.uint64), Gp.view(np.uint64))
            assert list(aN) == want_n and list(aNp) == want_np

        sums(A)
        if corr or mom:
            assert sqlib.sq_phi4_ens_step_heun(N._h, 6, 2, None, int(corr) | 2 * int(mom)) == 0
        else:
            assert N.step(6, scheme="heun") is None
        sums(N)
        fa = A.download()
        assert same_bits(fa, B.download()) and same_bits(fa, N.download())
        for r in range(3):
            assert same_bits(fa[r], recs[r][2][0]), f"replica {r} against the oracle"
        assert list(A.step_counter) == list(B.step_counter) == list(N.step_counter) == [6, 6, 6]
        assert not A.flags().any() and not N.flags().any()


@pytest.mark.parametrize("shape", [(16, 4, 31), (64, 3, 43), (64, 11, 29)])
def test_heun_steps_between_frames_calls(gpu, dev_oracle, shape):
    """run_frames(9), step(3, heun), run_frames(9) on the frames suite's recipe (loops 12, dtau0 = [0.19, 0.01,
    0.19], a counter near 2^32): the Heun call runs every replica at its own adapted dtau and counter, leaves
    the rule's carried T, V and firing step alone, and the second frames call goes on from its field exactly as
    from the oracle's Heun result uploaded into an ensemble that took the same first frames."""
    from test_gpu_phi4_ens_frames import SEEDS as FSEEDS, _recipe
    assert_shape(shape)

    def carried(E):
        s = E.stability()
        return [list(s[k]) for k in ("T", "V", "fired")]

    with _recipe(shape) as A, _recipe(shape) as B:
        sa, da = A.run_frames(9)
        sb, db = B.run_frames(9)
        assert np.array_equal(sa, sb) and np.array_equal(da, db)
        par = A.get_params()
        cnt = [int(s) for s in A.step_counter]
        # the case exercises what it claims: the replicas' step sizes and counters differ
        assert len(set(par["dtau"])) > 1 and len(set(cnt)) > 1, (par["dtau"], cnt)
        assert par["dtau"][0] != 0.19 or par["dtau"][2] != 0.19     # a controller has acted
        start = A.download()
        assert same_bits(start, B.download())
        before = carried(A)
        assert A.step(3, scheme="heun") is None
        got = A.download()
        assert carried(A) == before
        assert [int(s) for s in A.step_counter] == [c + 3 for c in cnt]
        want = []
        for r in range(3):
            p = dev_oracle.phi4_params(shape, par["dtau"][r], par["m2"][r], par["lam"][r], FSEEDS[r], clamp=1000.0,
                                       C=par["C"][r])
            assert p.h == np.float32(par["dtau"][r])               # h = float32(dtau), as the kernel's record
            fields, _ = _oracle_heun(dev_oracle, p, start[r], cnt[r], 3)
            want.append(fields[-1])
            assert same_bits(got[r], fields[-1]), f"replica {r}: {np.count_nonzero(got[r] != fields[-1])} sites differ"
        B.upload(np.stack(want))
        B.step_counter = np.array(cnt, dtype=np.uint64) + np.uint64(3)
        assert carried(B) == before                                # upload and set_step touch none of it
        sa2, da2 = A.run_frames(9)
        sb2, db2 = B.run_frames(9)
        assert np.array_equal(sa2, sb2)
        assert np.array_equal(da2, db2)                            # the same doubles
        assert same_bits(A.download(), B.download())
        assert carried(A) == carried(B)
        assert list(A.step_counter) == list(B.step_counter) == [c + 3 + 9 * 12 for c in cnt]
        assert np.array_equal(A.get_params()["dtau"], B.get_params()["dtau"])


@pytest.mark.parametrize("shape", ODE_SHAPES)
def test_order_of_convergence_against_float64(gpu, oracle_mod, shape):
    """Noise off (C = 0), m2 = 0.5, lam = 1, from phi4_init(seed 5, amp 0.8) to T = 0.8 in n = 16 and n = 32
    steps against the float64 RK4 solution (4000 steps) of dphi/dtau = lap phi - phi (m2 + lam phi^2 / 6):
    err_n = max |phi_n - reference|, order = log2(err_16 / err_32).

    Asserted on the GPU's fields: Heun order in [1.8, 2.5], Euler order in [0.8, 1.2], Heun err_32 < Euler
    err_32 / 10.  The nearest wrong answers are order 1 (a Heun step without its second stage or its average)
    and order 3.  Heun's err_32 is more than 100 x the accumulated fp32 rounding (32 steps of some 1e-7), so
    the order measured is the scheme's.

    Measured, 8x2x2 / 8x8x8 / 32x8x13:
      CPU oracle  Heun order 2.145 / 2.156 / 2.170, err_32 2.42e-4 / 3.40e-4 / 4.40e-4
                  Euler order 0.965 / 0.970 / 0.963, err_32 6.12e-3 / 9.42e-3 / 1.09e-2
      MI355X      Heun order 2.145 / 2.156 / 2.170, err_32 2.4235e-4 / 3.4038e-4 / 4.3983e-4
                  Euler order 0.965 / 0.970 / 0.963, err_32 6.1228e-3 / 9.4219e-3 / 1.0874e-2
                  (with the noise off the GPU's fields are the oracle's bit for bit, hence the same figures)
    """
    from stochquant_amd import Phi4Ensemble
    assert_shape(shape)
    phi0, ref = ode_start_and_reference(oracle_mod, shape)
    err = {"heun": {}, "euler": {}}
    for n in (16, 32):
        for scheme in ("heun", "euler"):
            with Phi4Ensemble(shape, 1, dtau=ODE_T / n, m2=ODE_M2, lam=ODE_LAM, C=0.0, seeds=[5], clamp=CLAMP) as E:
                E.upload(phi0)
                E.step(n, scheme=scheme)
                got = E.download()[0]
                assert not E.flags().any()
            err[scheme][n] = float(np.max(np.abs(got - ref)))
    assert_ode_orders("gpu", shape, err)
