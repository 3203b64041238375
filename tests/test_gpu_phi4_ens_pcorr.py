"""The phi^4 ensemble's momentum-projected time-slice correlators on the GPU
(sq_phi4_ens_set_momenta / _step_pcorr / _run_frames_pcorr / _pcorr_sums /
_pcorr_reset / _pslices / _pcorrelator; Phi4Ensemble.set_momenta,
step(momenta=True), run_frames(momenta=True), pcorr_sums, pcorr_reset, pslices,
pcorrelator).

Definitions (include/stochquant.h): for momentum m = (nx, ny) the projections
A_m(z) + i B_m(z) = sum_{x,y} phi (cx[x] + i sx[x]) (cy[y] + i sy[y]) with the
tables of sq_phi4_ens_momentum_table, in double in a fixed order; g_m(t) =
sum_z [A(z) A(zt) + B(z) B(zt)], zt = (z + t) mod Lz, as acc = (acc + A A) + B B
with z ascending; accumulators Gp[m][t] += g_m(t), nmeas_p += 1.

Tolerances: the projections against math.fsum of independently built terms
within (Lx Ly + 6) 2^-53 sum|phi| (derived at test_projections_...); everything
else bit for bit, restated on the host from the device's own A and B in float64
with separate multiplies and adds; the free field's exact stationary law within
4 standard errors of the replica mean.
"""
import ctypes
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (8,2,2): one wave, a four-quad slice; (8,3,5): odd Ly; (16,4,31): 16-quad slices, odd Lz; (32,8,13): exactly 64
# quads per slice; (64,16,8): 16 quads per row, K = 2; (32,32,32): K = 8, one image, four quads per lane and slice;
# (8,2,2000): K = 8, a column close to the longest the LDS rule admits (2040), nt = 1001 on 1024 lanes, M = 2
SHAPES = [(8, 2, 2), (8, 3, 5), (16, 4, 31), (32, 8, 13), (64, 16, 8), (32, 32, 32), (8, 2, 2000)]
DTAU, M2, LAM = 0.02, 0.5, 1.0
SEEDS = [1234, 99, 0xDEADBEEF12345]
U = 2.0 ** -53

_cache = {}


def _momenta(shape):
    Lx, Ly, Lz = shape
    if Lz == 2000:
        return [(0, 0), (1, 1)]
    return [(0, 0), (1, 0), (0, 1), (1, 1), (Lx - 1, Ly - 1), (Lx // 2, 1), (1, 1)]


def _ens(shape, R, momenta=None, **kw):
    from stochquant_amd import Phi4Ensemble
    kw.setdefault("dtau", DTAU)
    kw.setdefault("m2", M2)
    kw.setdefault("lam", LAM)
    E = Phi4Ensemble(shape, R, **kw)
    E.set_momenta(_momenta(shape) if momenta is None else momenta)
    return E


def _starts(oracle_mod, shape, amp=0.9, seeds=(77, 78, 79)):
    """Distinct start fields, one per replica (computed once per shape)."""
    key = ("start", shape)
    if key not in _cache:
        _cache[key] = np.stack([oracle_mod.phi4_init(oracle_mod.phi4_params(shape, DTAU, M2, LAM, s), amp)
                                for s in seeds])
        _cache[key].setflags(write=False)
    return _cache[key]


def _measured(oracle_mod, shape):
    """Noisy fields after three steps and their pslices(), slices() (one GPU run per shape)."""
    key = ("meas", shape)
    if key not in _cache:
        with _ens(shape, 3, seeds=SEEDS) as E:
            E.upload(_starts(oracle_mod, shape))
            E.step(3)
            phi = E.download()
            AB, g = E.pslices()
            S, g0 = E.slices()
            assert E.momenta == _momenta(shape)
        for a in (phi, AB, g, S, g0):
            a.setflags(write=False)
        _cache[key] = (phi, AB, g, S, g0)
    return _cache[key]


def _weights(shape, m):
    """Re and Im of e^{i (px x + py y)} on one slice, indexed [y, x] like the field's rows: the table values
    combined as cos(a + b) = cos a cos b - sin a sin b, sin(a + b) = cos a sin b + sin a cos b."""
    from stochquant_amd import Phi4Ensemble
    Lx, Ly, _ = shape
    cx, sx = Phi4Ensemble.momentum_table(Lx, m[0])
    cy, sy = Phi4Ensemble.momentum_table(Ly, m[1])
    wa = np.empty((Ly, Lx))
    wb = np.empty((Ly, Lx))
    for y in range(Ly):
        for x in range(Lx):
            wa[y, x] = cx[x] * cy[y] - sx[x] * sy[y]
            wb[y, x] = cx[x] * sy[y] + sx[x] * cy[y]
    return wa, wb


def _g_host(A, B):
    """g_m(t), t = 0 .. Lz // 2, from one momentum's projections: z ascending with the wrap, acc = (acc + A(z)
    A(zt)) + B(z) B(zt), one float64 rounding per product and per sum (NumPy's elementwise ops; no fused
    multiply-add)."""
    Lz = len(A)
    nt = Lz // 2 + 1
    t = np.arange(nt)
    acc = np.zeros(nt)
    for z in range(Lz):
        zt = (z + t) % Lz
        acc = (acc + A[z] * A[zt]) + B[z] * B[zt]
    return acc


def _follow(E, rounds, k):
    """Stand-alone restatement: `rounds` times step(k) then pslices(), accumulated in float64 in order."""
    G = np.zeros((E.R, len(E.momenta), E.nt))
    for _ in range(rounds):
        E.step(k)
        G = G + E.pslices()[1]
    return G


@pytest.mark.parametrize("shape", SHAPES)
def test_projections_against_an_independent_evaluation(gpu, oracle_mod, shape):
    """A_m(z), B_m(z) of noisy fields against math.fsum over the 2-D products phi[y, x] w[y, x], w built from the
    same tables with x and y indexed independently of the kernel's quad arithmetic.

    Bound.  Both sides evaluate sum over the n = Lx Ly sites of phi (cx cy - sx sy) (A; B alike) from the same
    table values, so only roundings differ.  Device: a site's two terms phi cx cy and phi sx sy each pass two
    product roundings (phi cx, then re cy) and the additions on their way to lane 63: two inside the quad, the
    subtraction, one per quad of the lane (at most ceil(n / 256)) and six of the scan -- never more than n - 1
    for n >= 16, the smallest slice.  So each term carries a relative error of at most (1 + u)^(n + 1) - 1, u =
    2^-53, and sum |terms| = sum |phi| (|cx cy| + |sx sy|) <= sum |phi| (Cauchy-Schwarz on unit vectors).
    Reference: w has three roundings of quantities <= 1 in magnitude, absolute error <= 3 u; phi w one more
    (relative u); math.fsum rounds the exact sum of those once: at most 5 u sum |phi| together.  With the
    second-order terms ((n + 6) u < 3e-13 here) the difference is within (n + 6) u sum|phi| per slice."""
    phi, AB, g, S, g0 = _measured(oracle_mod, shape)
    Lx, Ly, Lz = shape
    moms = _momenta(shape)
    assert AB.shape == (3, len(moms), Lz, 2) and g.shape == (3, len(moms), Lz // 2 + 1)
    n = Lx * Ly
    f64 = phi.astype(np.float64)
    ref = np.zeros(AB.shape)
    bound = np.zeros((3, Lz))
    for r in range(3):
        for z in range(Lz):
            bound[r, z] = (n + 6) * U * float(np.sum(np.abs(f64[r, z])))
    worst = 0.0
    for mi, m in enumerate(moms):
        wa, wb = _weights(shape, m)
        for r in range(3):
            for z in range(Lz):
                ref[r, mi, z, 0] = math.fsum((f64[r, z] * wa).ravel())
                ref[r, mi, z, 1] = math.fsum((f64[r, z] * wb).ravel())
        err = np.abs(AB[:, mi] - ref[:, mi]).max(axis=-1)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (m, float(np.max(err / bound)))
    print(f"pcorr projections {shape}: worst |AB - fsum| / bound = {worst:.3g}")
    if (1, 0) in moms and (0, 1) in moms:
        # the reference itself tells the axes apart: every slice's (1, 0) and (0, 1) projections differ by far
        # more than the bound, so swapped axes (or a conjugated momentum: B changes sign) cannot pass above
        d = np.abs(ref[:, moms.index((1, 0))] - ref[:, moms.index((0, 1))]).max(axis=-1)
        assert np.all(d > bound), float(np.min(d / bound))
        i11 = moms.index((1, 1))
        assert np.all(np.abs(ref[:, i11, :, 1]).max(axis=-1) > bound.max(axis=-1))


@pytest.mark.parametrize("shape", SHAPES)
def test_g_is_the_stated_arithmetic(gpu, oracle_mod, shape):
    phi, AB, g, S, g0 = _measured(oracle_mod, shape)
    for r in range(3):
        for mi in range(AB.shape[1]):
            ref = _g_host(AB[r, mi, :, 0], AB[r, mi, :, 1])
            assert np.array_equal(g[r, mi], ref), (r, mi, np.max(np.abs(g[r, mi] - ref)))


@pytest.mark.parametrize("shape", SHAPES)
def test_zero_momentum_is_the_existing_correlator(gpu, oracle_mod, shape):
    phi, AB, g, S, g0 = _measured(oracle_mod, shape)
    moms = _momenta(shape)
    assert moms[0] == (0, 0)
    assert np.array_equal(AB[:, 0, :, 0], S)
    assert not AB[:, 0, :, 1].any() and not np.signbit(AB[:, 0, :, 1]).any()      # B = +0.0
    assert np.array_equal(g[:, 0], g0)
    dup = [i for i, m in enumerate(moms) if m == (1, 1)]
    if len(dup) == 2:
        assert np.array_equal(AB[:, dup[0]], AB[:, dup[1]]) and np.array_equal(g[:, dup[0]], g[:, dup[1]])
    with _ens(shape, 3, seeds=SEEDS) as E:
        E.upload(_starts(oracle_mod, shape))
        E.step(12, every=4, correlate=True, momenta=True)
        Gp, nmp = E.pcorr_sums()
        G, S1, nm = E.corr_sums()
        assert list(nmp) == list(nm) == [3, 3, 3]
        assert np.array_equal(Gp[:, 0], G)
        if len(dup) == 2:
            assert np.array_equal(Gp[:, dup[0]], Gp[:, dup[1]])


@pytest.mark.parametrize("shape", SHAPES)
def test_nothing_else_moves(gpu, oracle_mod, shape):
    from stochquant_amd import _lib
    phi0 = _starts(oracle_mod, shape)

    def fresh():
        E = _ens(shape, 3, seeds=SEEDS)
        E.upload(phi0)
        return E

    with fresh() as A, fresh() as A2, fresh() as P, fresh() as P2:
        # A, P: the C calls without a series; A2, P2: the Python calls, which ask for one
        _lib.call("sq_phi4_ens_step_pcorr", A._h, 12, 4, None, 1)
        _lib.call("sq_phi4_ens_step_corr", P._h, 12, 4, None)
        serA = A2.step(12, every=4, correlate=True, momenta=True)
        serP = P2.step(12, every=4, correlate=True)
        assert serA.shape == (3, 3, 4) and np.array_equal(serA, serP)
        ref_field = P.download()
        GP, S1P, nP = P.corr_sums()
        assert list(nP) == [3, 3, 3]
        for E in (A, A2, P2):
            assert np.array_equal(E.download(), ref_field)
            assert list(E.step_counter) == [12, 12, 12]
            assert np.array_equal(E.flags(), P.flags())
            G, S1, nm = E.corr_sums()
            assert np.array_equal(G, GP) and np.array_equal(S1, S1P) and list(nm) == [3, 3, 3]
        assert np.array_equal(A.pcorr_sums()[0], A2.pcorr_sums()[0])
        # the calls without momenta measure none; momenta without correlate leave G, S1, nmeas alone
        assert not P.pcorr_sums()[0].any() and not P.pcorr_sums()[1].any()
        P.step(4, every=4, momenta=True)
        G, S1, nm = P.corr_sums()
        assert np.array_equal(G, GP) and np.array_equal(S1, S1P) and list(nm) == [3, 3, 3]
        assert list(P.pcorr_sums()[1]) == [1, 1, 1]


@pytest.mark.parametrize("shape", SHAPES)
def test_in_flight_equals_stand_alone(gpu, oracle_mod, shape):
    phi0 = _starts(oracle_mod, shape)

    def fresh():
        E = _ens(shape, 3, seeds=SEEDS)
        E.upload(phi0)
        return E

    with fresh() as A, fresh() as B, fresh() as C:
        A.step(12, every=4, momenta=True)
        GB = _follow(B, 3, 4)
        G, nm = A.pcorr_sums()
        assert list(nm) == [3, 3, 3]
        assert np.array_equal(G, GB), np.max(np.abs(G - GB))
        assert np.array_equal(A.download(), B.download())
        # split calls add up to the same bits
        C.step(8, every=4, momenta=True)
        C.step(4, every=4, momenta=True)
        GC, nC = C.pcorr_sums()
        assert np.array_equal(GC, G) and list(nC) == [3, 3, 3]


@pytest.mark.parametrize("shape", [(8, 3, 5), (32, 32, 32)])
def test_tail_reset_persistence_and_set_momenta(gpu, oracle_mod, shape):
    phi0 = _starts(oracle_mod, shape)
    with _ens(shape, 3, seeds=SEEDS) as A, _ens(shape, 3, seeds=SEEDS) as C:
        for E in (A, C):
            E.upload(phi0)
        A.step(12, every=4, momenta=True)
        GA, nA = A.pcorr_sums()
        C.step(11, every=4, momenta=True)            # an incomplete tail measures nothing
        assert list(C.pcorr_sums()[1]) == [2, 2, 2]
        assert C.step(3, every=4, momenta=True).shape == (0, 3, 4)
        assert list(C.pcorr_sums()[1]) == [2, 2, 2]
        # ranges
        G1, n1 = A.pcorr_sums(first=1, count=2)
        assert np.array_equal(G1, GA[1:]) and list(n1) == [3, 3]
        # uploads, setters and the zero-momentum reset leave the accumulators alone
        A.upload(phi0)
        A.set_params(dtau=0.01, m2=0.25)
        A.step_counter = [5, 6, 7]
        A.set_stability(1.0, 2.0)
        A.corr_reset()
        G2, n2 = A.pcorr_sums()
        assert np.array_equal(G2, GA) and list(n2) == [3, 3, 3]
        # reset zeroes its range only
        A.pcorr_reset(first=1, count=1)
        G3, n3 = A.pcorr_sums()
        assert not G3[1].any() and list(n3) == [3, 0, 3]
        assert np.array_equal(G3[[0, 2]], GA[[0, 2]])
        # set_momenta clears everything, with the same list too, and a shorter list changes the layout
        A.set_momenta(_momenta(shape))
        G4, n4 = A.pcorr_sums()
        assert G4.shape == GA.shape and not G4.any() and not n4.any()
        A.step(4, every=4, momenta=True)
        A.set_momenta([(1, 1), (0, 1)])
        assert A.momenta == [(1, 1), (0, 1)]
        G5, n5 = A.pcorr_sums()
        assert G5.shape == (3, 2, A.nt) and not G5.any() and not n5.any()
    # a momentum's row does not depend on the list it stands in
    with _ens(shape, 3, seeds=SEEDS) as F, _ens(shape, 3, momenta=[(1, 1), (0, 1)], seeds=SEEDS) as H:
        for E in (F, H):
            E.upload(phi0)
            E.step(8, every=4, momenta=True)
        assert np.array_equal(H.pcorr_sums()[0], F.pcorr_sums()[0][:, [3, 2]])


def test_independent_of_R_and_position(gpu):
    shape = (8, 8, 8)
    with _ens(shape, 300, seed=5000) as E, _ens(shape, 2, seeds=[5001, 5007]) as O:
        for X in (E, O):
            X.init_field(0.5)
            X.step(8, every=2, momenta=True)
        G, nm = E.pcorr_sums(first=7, count=1)
        Go, no = O.pcorr_sums(first=1, count=1)
        assert list(nm) == list(no) == [4]
        assert np.array_equal(G, Go)
        assert np.array_equal(E.download(first=7, count=1), O.download(first=1, count=1))
        assert list(E.pcorr_sums()[1]) == [4] * 300
        assert np.array_equal(E.pcorr_sums(first=1, count=1)[0], O.pcorr_sums(first=0, count=1)[0])


LOOPS = 12
FR_SEEDS = [99, 1234, 0xDEADBEEF12345, 7]
FR_DTAU = [0.19, 0.01, 0.19, 0.01]


def _frames_ens(shape, adapt):
    E = _ens(shape, 4, dtau=FR_DTAU, m2=1.0, lam=1.0, C=1.0, seeds=FR_SEEDS, loops=LOOPS, adapt_dtau=adapt)
    E.init_field(0.3)
    return E


@pytest.mark.parametrize("adapt", [True, False], ids=["adapt", "fixed"])
@pytest.mark.parametrize("shape", [(8, 8, 8), (32, 8, 13), (32, 32, 32)])
def test_frames(gpu, shape, adapt):
    nfr = 6
    with _frames_ens(shape, adapt) as A, _frames_ens(shape, adapt) as P, _frames_ens(shape, adapt) as B, \
            _frames_ens(shape, adapt) as Z:
        st, dt, ser = A.run_frames(nfr, measure=True, momenta=True)
        stP, dtP, serP = P.run_frames(nfr, measure=True)
        stZ, dtZ = Z.run_frames(nfr, correlate=True, momenta=True)
        print(f"pcorr frames {shape} adapt={adapt}: stable frames per replica {st.sum(axis=0)}")
        assert st.any() and not st.all()             # Δτ = 0.19 is above the Euler limit, 0.01 well below
        assert np.array_equal(st, stP) and np.array_equal(dt, dtP) and np.array_equal(ser, serP)
        assert np.array_equal(st, stZ) and np.array_equal(dt, dtZ)
        for E in (A, Z):
            assert np.array_equal(E.download(), P.download())
            assert np.array_equal(E.step_counter, P.step_counter)
            assert np.array_equal(E.flags(), P.flags())
        sa, sp = A.stability(), P.stability()
        assert np.array_equal(sa["T"], sp["T"]) and np.array_equal(sa["V"], sp["V"])
        assert np.array_equal(sa["fired"], sp["fired"])
        G, nm = A.pcorr_sums()
        assert list(nm) == list(st.sum(axis=0))
        assert not P.pcorr_sums()[1].any() and not A.corr_sums()[2].any()
        # the twin, frame by frame: pslices() of the adopted field after each stable frame
        GB = np.zeros_like(G)
        for f in range(nfr):
            ok = B.run_frame()
            assert np.array_equal(ok, st[f])
            g = B.pslices()[1]
            for r in range(4):
                if ok[r]:
                    GB[r] = GB[r] + g[r]
        assert np.array_equal(G, GB)
        for r in range(4):
            if nm[r] == 0:
                assert not G[r].any()
        # with correlate: the same momentum sums, and the zero-momentum accumulators beside them
        GZ, nZ = Z.pcorr_sums()
        assert np.array_equal(GZ, G) and list(nZ) == list(nm)
        G0, S10, n0 = Z.corr_sums()
        assert list(n0) == list(nm) and np.array_equal(G0, G[:, 0])


def _pcorrelator_host(G, nm, shape, n):
    """sq_phi4_ens_pcorrelator restated: per momentum, replicas in index order, sequential float64 sums."""
    V = float(shape[0] * shape[1] * shape[2])
    rows = [r for r in range(len(nm)) if nm[r] > 0]
    u = len(rows)
    M = G.shape[1]
    mean, err = np.zeros((M, n)), np.zeros((M, n))
    for m in range(M):
        for t in range(n):
            c = [float(G[r, m, t]) / (float(nm[r]) * V) for r in rows]
            s = 0.0
            for v in c:
                s = s + v
            mu = s / float(u)
            q = 0.0
            for v in c:
                q = q + (v - mu) * (v - mu)
            mean[m, t] = mu
            err[m, t] = math.sqrt(q / (float(u) * float(u - 1))) if u > 1 else 0.0
    return mean, err, u


def test_pcorrelator_statistics(gpu, oracle_mod):
    from stochquant_amd import StochQuantError
    shape = (8, 3, 5)
    with _ens(shape, 4, seeds=SEEDS + [5]) as E:
        with pytest.raises(StochQuantError) as ei:
            E.pcorrelator()
        assert ei.value.code == -4                    # SQ_E_STATE: nothing measured yet
        E.upload(_starts(oracle_mod, shape)[0])
        E.step(10, every=2, momenta=True)
        E.step(3, every=3, momenta=True)
        E.pcorr_reset(first=2, count=1)               # replica 2 drops out
        G, nm = E.pcorr_sums()
        assert list(nm) == [6, 6, 0, 6]
        for n in (E.nt, 1):
            mean, err, used = E.pcorrelator(n=n)
            rm, re, ru = _pcorrelator_host(G, nm, shape, n)
            assert used == ru == 3 and mean.shape == (7, n)
            assert np.array_equal(mean, rm), (n, mean, rm)
            assert np.array_equal(err, re), (n, err, re)
            assert np.all(err > 0)
        E.pcorr_reset(first=0, count=2)               # one replica left: no error bar
        mean, err, used = E.pcorrelator()
        assert used == 1 and not err.any() and mean.any()
        with pytest.raises(StochQuantError):
            E.pcorrelator(n=E.nt + 1)


def test_free_field_exact_law(gpu):
    """λ = 0: the Euler scheme's stationary two-point function in closed form, E[c(m, t)] = (1/Lz) Σ_k
    cos(2πkt/Lz) / (ω² (1 − Δτ ω² / 2)), ω² = m² + (2 − 2 cos(2π nx / Lx)) + (2 − 2 cos(2π ny / Ly)) + 2 − 2
    cos(2πk/Lz).  (1, 0) and (0, 1) differ by 30 % at t = 0 with a 0.4 % error bar: a swapped axis, a wrong
    normalisation or a wrong wrap misses by tens of standard errors.  The same run with the mathematical noise
    of the repository's oracle on the CPU stayed within 2.4 standard errors at all 35 points; the seeds are
    fixed.  The 4 sigma cap is test_gpu_phi4_ens_corr.py's."""
    shape, R, dtau, m2 = (8, 4, 8), 128, 0.05, 1.0
    Lx, Ly, Lz = shape
    moms = [(0, 0), (1, 0), (0, 1), (1, 1), (3, 2), (7, 3), (4, 2)]
    k = np.arange(Lz)
    nt = Lz // 2 + 1
    exact = np.zeros((len(moms), nt))
    for mi, (nx, ny) in enumerate(moms):
        w2 = (m2 + (2.0 - 2.0 * np.cos(2.0 * np.pi * nx / Lx)) + (2.0 - 2.0 * np.cos(2.0 * np.pi * ny / Ly))
              + 2.0 - 2.0 * np.cos(2.0 * np.pi * k / Lz))
        for t in range(nt):
            exact[mi, t] = np.sum(np.cos(2.0 * np.pi * k * t / Lz) / (w2 * (1.0 - dtau * w2 / 2.0))) / Lz
    assert np.allclose(exact[:, 0], [0.474686, 0.363550, 0.246838, 0.220845, 0.131721, 0.220845, 0.127015], atol=1e-6)
    with _ens(shape, R, momenta=moms, dtau=dtau, m2=m2, lam=0.0, C=1.0, seeds=[1000 + r for r in range(R)]) as E:
        E.step(200)
        E.pcorr_reset()
        E.step(1600, every=20, momenta=True)
        mean, err, used = E.pcorrelator()
        assert used == R and not E.flags().any()
        assert list(E.pcorr_sums()[1]) == [80] * R
    ratio = (mean - exact) / err
    for mi, m in enumerate(moms):
        print(f"pcorr free field {m}: (mean - exact) / err =", " ".join(f"{x:+.2f}" for x in ratio[mi]),
              " err =", " ".join(f"{x:.4f}" for x in err[mi]))
    assert mean.shape == (7, nt)
    assert np.all(np.abs(mean - exact) <= 4.0 * err), (mean, exact, err)


def test_errors(gpu):
    from stochquant_amd import Phi4Ensemble, StochQuantError, _lib

    def code(fn):
        with pytest.raises(StochQuantError) as ei:
            fn()
        return ei.value.code

    with Phi4Ensemble((8, 4, 8), 2, dtau=DTAU, m2=M2, lam=LAM) as E:
        assert E.momenta == []
        assert code(lambda: E.step(4, every=2, momenta=True)) == -4          # SQ_E_STATE before set_momenta
        assert code(lambda: E.run_frames(1, momenta=True)) == -4
        E.set_momenta([(1, 1)])
        E.step(4, every=2, momenta=True)
        E.set_momenta([])
        assert E.momenta == [] and E.pcorr_sums()[0].shape == (2, 0, 5) and not E.pcorr_sums()[1].any()
        assert code(lambda: E.step(4, every=2, momenta=True)) == -4          # ... and after set_momenta([])
        assert code(lambda: E.pslices()) == -4 and code(lambda: E.pcorrelator()) == -4
        E.set_momenta([(1, 1), (2, 3)])
        assert code(lambda: E.set_momenta([(0, 0)] * 9)) == -1               # SQ_E_ARG: M = 9
        assert code(lambda: E.set_momenta([(8, 0)])) == -1                   # nx = Lx
        assert code(lambda: E.set_momenta([(0, 4)])) == -1                   # ny = Ly
        assert code(lambda: E.set_momenta([(0, -1)])) == -1                  # ny = -1
        assert code(lambda: E.set_momenta([(-1, 0)])) == -1
        assert E.momenta == [(1, 1), (2, 3)]                                 # a refused list changes nothing
        assert code(lambda: _lib.call("sq_phi4_ens_step_pcorr", E._h, 4, 0, None, 0)) == -1      # every = 0
        assert code(lambda: _lib.call("sq_phi4_ens_step_pcorr", E._h, -1, 2, None, 0)) == -1
        M = ctypes.c_int(-1)
        assert code(lambda: _lib.call("sq_phi4_ens_get_momenta", E._h, None, None)) == -1
        _lib.call("sq_phi4_ens_get_momenta", E._h, ctypes.byref(M), None)
        assert M.value == 2
        assert list(E.step_counter) == [4, 4]
    with Phi4Ensemble((8, 2, 2048), 1, dtau=DTAU, m2=M2, lam=LAM) as E:      # no LDS for 2 Lz doubles
        assert code(lambda: E.set_momenta([(0, 0)])) == -1
        assert E.momenta == []
        E.step(2, every=1, correlate=True)                                   # the zero-momentum one still fits
        assert list(E.corr_sums()[2]) == [2]
