"""The phi^4 ensemble's in-kernel time-slice correlator on the GPU
(sq_phi4_ens_step_corr / _run_frames_corr / _corr_sums / _corr_reset / _slices /
_correlator; Phi4Ensemble.step(correlate=True), run_frames(correlate=True),
corr_sums, corr_reset, slices, correlator).

Definitions (include/stochquant.h): S(z) = sum_{x,y} phi in double in a fixed
order, g(t) = sum_z S(z) S((z + t) mod Lz) with z ascending and one rounding
per product and per sum, accumulators G += g, S1 += sum_z S(z), nmeas += 1.

Tolerances: the slice sums against the exactly rounded sum (math.fsum) within
2 n u sum|phi| (n = Lx Ly terms, u = 2^-53: any order of n double additions is
within (n - 1) u sum|t| of the exact sum; the bound test_gpu_phi4_ens.py uses
for the in-flight sums); everything else bit for bit, restated on the host from
the device's own S in float64 with separate multiplies and adds; the free
field's exact stationary law within 4 standard errors of the replica mean.
"""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# (8,2,2): one wave, nt = 2, the wrap double-counts; (8,3,5): 6 quads per slice, odd Lz, 30 quads in a wave;
# (16,4,31): 16-quad slices, odd Lz; (32,8,13): exactly 64 quads per slice; (64,16,8): K = 2, more waves than
# slices; (32,32,32): K = 8, one image; (8,2,2048): K = 8, Lz at its maximum, nt = 1025 > 1024 lanes
SHAPES = [(8, 2, 2), (8, 3, 5), (16, 4, 31), (32, 8, 13), (64, 16, 8), (32, 32, 32), (8, 2, 2048)]
DTAU, M2, LAM = 0.02, 0.5, 1.0
SEEDS = [1234, 99, 0xDEADBEEF12345]
U = 2.0 ** -53

_cache = {}


def _ens(shape, R, **kw):
    from stochquant_amd import Phi4Ensemble
    kw.setdefault("dtau", DTAU)
    kw.setdefault("m2", M2)
    kw.setdefault("lam", LAM)
    return Phi4Ensemble(shape, R, **kw)


def _starts(oracle_mod, shape, amp=0.9, seeds=(77, 78, 79)):
    """Distinct start fields, one per replica (computed once per shape)."""
    key = ("start", shape)
    if key not in _cache:
        _cache[key] = np.stack([oracle_mod.phi4_init(oracle_mod.phi4_params(shape, DTAU, M2, LAM, s), amp)
                                for s in seeds])
        _cache[key].setflags(write=False)
    return _cache[key]


def _measured(oracle_mod, shape):
    """slices() and moments() of the start fields (one GPU run per shape)."""
    key = ("meas", shape)
    if key not in _cache:
        with _ens(shape, 3, seeds=SEEDS) as E:
            E.upload(_starts(oracle_mod, shape))
            S, g = E.slices()
            _cache[key] = (S, g, E.moments()["S1"])
    return _cache[key]


def _g_host(S):
    """g(t), t = 0 .. Lz // 2, of one replica's slice sums: z ascending with the wrap, one float64 multiply and one
    float64 add per term (NumPy's elementwise ops round each once; no fused multiply-add)."""
    Lz = len(S)
    nt = Lz // 2 + 1
    t = np.arange(nt)
    acc = np.zeros(nt)
    for z in range(Lz):
        acc = acc + S[z] * S[(z + t) % Lz]
    return acc


def _s1_host(S):
    s = 0.0
    for v in S:
        s = s + float(v)
    return s


def _follow(E, rounds, steps_per_round):
    """Stand-alone restatement: `rounds` times step(k) then slices(), accumulated in float64 in order."""
    G = np.zeros((E.R, E.nt))
    S1 = np.zeros(E.R)
    for _ in range(rounds):
        E.step(steps_per_round)
        S, g = E.slices()
        G = G + g
        S1 = S1 + np.array([_s1_host(S[r]) for r in range(E.R)])
    return G, S1


@pytest.mark.parametrize("shape", SHAPES)
def test_slice_sums_against_exact_sum(gpu, oracle_mod, shape):
    phi = _starts(oracle_mod, shape).astype(np.float64)
    S, g, mS1 = _measured(oracle_mod, shape)
    Lx, Ly, Lz = shape
    assert S.shape == (3, Lz) and g.shape == (3, Lz // 2 + 1)
    n = Lx * Ly
    worst = 0.0
    for r in range(3):
        tot_bound = 0.0
        for z in range(Lz):
            sl = phi[r, z].ravel()
            bound = 2 * n * U * float(np.sum(np.abs(sl)))
            err = abs(S[r, z] - math.fsum(sl))
            worst = max(worst, err / bound)
            assert err <= bound, (r, z, err, bound)
            tot_bound += bound
        mom_bound = 2 * (n * Lz) * U * float(np.sum(np.abs(phi[r])))
        assert abs(math.fsum(S[r]) - mS1[r]) <= tot_bound + mom_bound, (r, math.fsum(S[r]), mS1[r])
    print(f"corr slices {shape}: worst |S - fsum| / bound = {worst:.3g}")


@pytest.mark.parametrize("shape", SHAPES)
def test_g_is_the_stated_arithmetic(gpu, oracle_mod, shape):
    S, g, _ = _measured(oracle_mod, shape)
    for r in range(3):
        ref = _g_host(S[r])
        assert np.array_equal(g[r], ref), (r, np.max(np.abs(g[r] - ref)))
        # the wrap: g(t) counts every pair at distance t once per z, so g(0) = sum S^2 >= |g(t)|
        assert np.all(np.abs(g[r]) <= g[r][0] * (1 + 1e-12))


@pytest.mark.parametrize("shape", SHAPES)
def test_in_flight_equals_stand_alone(gpu, oracle_mod, shape):
    from stochquant_amd import _lib
    phi0 = _starts(oracle_mod, shape)

    def fresh():
        E = _ens(shape, 3, seeds=SEEDS)
        E.upload(phi0)
        return E

    with fresh() as A, fresh() as A2, fresh() as B, fresh() as P, fresh() as P2:
        # A: the C call without a series; A2: the Python call, which asks for one
        _lib.call("sq_phi4_ens_step_corr", A._h, 12, 4, None)
        ser2 = A2.step(12, every=4, correlate=True)
        GB, S1B = _follow(B, 3, 4)
        P.step(12)
        serP = P2.step(12, every=4)
        ref_field = P.download()
        for E in (A, A2):
            G, S1, nm = E.corr_sums()
            assert list(nm) == [3, 3, 3]
            assert np.array_equal(G, GB), np.max(np.abs(G - GB))
            assert np.array_equal(S1, S1B)
        for E in (A, A2, B, P2):
            assert np.array_equal(E.download(), ref_field)
            assert list(E.step_counter) == [12, 12, 12]
            assert np.array_equal(E.flags(), P.flags())
        assert ser2.shape == (3, 3, 4) and np.array_equal(ser2, serP)
        # plain calls measure nothing
        for E in (B, P, P2):
            G, S1, nm = E.corr_sums()
            assert not G.any() and not S1.any() and not nm.any()


@pytest.mark.parametrize("shape", [(8, 3, 5), (32, 32, 32)])
def test_additive_tail_reset_and_persistence(gpu, oracle_mod, shape):
    phi0 = _starts(oracle_mod, shape)
    with _ens(shape, 3, seeds=SEEDS) as A, _ens(shape, 3, seeds=SEEDS) as B, _ens(shape, 3, seeds=SEEDS) as C:
        for E in (A, B, C):
            E.upload(phi0)
        A.step(12, every=4, correlate=True)
        B.step(8, every=4, correlate=True)
        B.step(4, every=4, correlate=True)
        GA, SA, nA = A.corr_sums()
        GB, SB, nB = B.corr_sums()
        assert np.array_equal(GA, GB) and np.array_equal(SA, SB) and list(nA) == list(nB) == [3, 3, 3]
        C.step(11, every=4, correlate=True)          # an incomplete tail measures nothing
        assert list(C.corr_sums()[2]) == [2, 2, 2]
        assert C.step(3, every=4, correlate=True).shape == (0, 3, 4)
        assert list(C.corr_sums()[2]) == [2, 2, 2]
        # ranges
        G1, S1, n1 = A.corr_sums(first=1, count=2)
        assert np.array_equal(G1, GA[1:]) and np.array_equal(S1, SA[1:]) and list(n1) == [3, 3]
        # uploads and setters leave the accumulators alone
        A.upload(phi0)
        A.set_params(dtau=0.01, m2=0.25)
        A.step_counter = [5, 6, 7]
        A.set_stability(1.0, 2.0)
        G2, S2, n2 = A.corr_sums()
        assert np.array_equal(G2, GA) and np.array_equal(S2, SA) and list(n2) == [3, 3, 3]
        # reset zeroes its range only
        A.corr_reset(first=1, count=1)
        G3, S3, n3 = A.corr_sums()
        assert not G3[1].any() and S3[1] == 0.0 and list(n3) == [3, 0, 3]
        assert np.array_equal(G3[[0, 2]], GA[[0, 2]]) and np.array_equal(S3[[0, 2]], SA[[0, 2]])
        A.corr_reset()
        assert not A.corr_sums()[0].any() and not A.corr_sums()[2].any()


def test_independent_of_R_and_position(gpu):
    shape = (8, 8, 8)
    with _ens(shape, 300, seed=5000) as E, _ens(shape, 1, seeds=[5007]) as O:
        for X in (E, O):
            X.init_field(0.5)
            X.step(8, every=2, correlate=True)
        G, S1, nm = E.corr_sums(first=7, count=1)
        Go, So, no = O.corr_sums()
        assert list(nm) == list(no) == [4]
        assert np.array_equal(G, Go) and np.array_equal(S1, So)
        assert np.array_equal(E.download(first=7, count=1), O.download())
        assert list(E.corr_sums()[2]) == [4] * 300


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
    from stochquant_amd import StochQuantError
    nfr = 6
    with _frames_ens(shape, adapt) as A, _frames_ens(shape, adapt) as P, _frames_ens(shape, adapt) as B:
        st, dt, ser = A.run_frames(nfr, measure=True, correlate=True)
        stP, dtP, serP = P.run_frames(nfr, measure=True)
        print(f"corr frames {shape} adapt={adapt}: stable frames per replica {st.sum(axis=0)}")
        assert st.any() and not st.all()             # Δτ = 0.19 is above the Euler limit, 0.01 well below
        assert np.array_equal(st, stP) and np.array_equal(dt, dtP) and np.array_equal(ser, serP)
        assert np.array_equal(A.download(), P.download())
        assert np.array_equal(A.step_counter, P.step_counter)
        assert np.array_equal(A.flags(), P.flags())
        sa, sp = A.stability(), P.stability()
        assert np.array_equal(sa["T"], sp["T"]) and np.array_equal(sa["V"], sp["V"])
        assert np.array_equal(sa["fired"], sp["fired"])
        for r in range(4):
            n = LOOPS if sa["fired"][r] < 0 else sa["fired"][r] + 1
            for k in ("M", "D", "A"):
                assert np.array_equal(sa[k][r][:n], sp[k][r][:n]), (r, k)
        G, S1, nm = A.corr_sums()
        assert list(nm) == list(st.sum(axis=0))
        assert not P.corr_sums()[2].any()
        # the twin, frame by frame: slices() of the adopted field after each stable frame
        GB, S1B = np.zeros_like(G), np.zeros_like(S1)
        for f in range(nfr):
            ok = B.run_frame()
            assert np.array_equal(ok, st[f])
            S, g = B.slices()
            for r in range(4):
                if ok[r]:
                    GB[r] = GB[r] + g[r]
                    S1B[r] = S1B[r] + _s1_host(S[r])
        assert np.array_equal(G, GB) and np.array_equal(S1, S1B)
        mean, err, used = A.correlator()
        assert used == int((nm > 0).sum())
        for r in range(4):
            if nm[r] == 0:
                assert not G[r].any() and S1[r] == 0.0
        with pytest.raises(StochQuantError) as ei:
            P.correlator()
        assert ei.value.code == -4


def _correlator_host(G, S1, nm, shape, n, connected):
    """sq_phi4_ens_correlator restated: replicas in index order, sequential float64 sums."""
    V = float(shape[0] * shape[1] * shape[2])
    Lz = float(shape[2])
    rows = [r for r in range(len(nm)) if nm[r] > 0]
    u = len(rows)
    mean, err = np.zeros(n), np.zeros(n)
    for t in range(n):
        c = []
        for r in rows:
            k = float(nm[r])
            v = float(G[r, t]) / (k * V)
            if connected:
                sb = float(S1[r]) / k
                v = v - sb * sb / (Lz * V)
            c.append(v)
        s = 0.0
        for v in c:
            s = s + v
        m = s / float(u)
        q = 0.0
        for v in c:
            q = q + (v - m) * (v - m)
        mean[t] = m
        err[t] = math.sqrt(q / (float(u) * float(u - 1))) if u > 1 else 0.0
    return mean, err, u


def test_correlator_statistics(gpu, oracle_mod):
    from stochquant_amd import StochQuantError
    shape = (8, 3, 5)
    with _ens(shape, 4, seeds=SEEDS + [5]) as E:
        with pytest.raises(StochQuantError) as ei:
            E.correlator()
        assert ei.value.code == -4                    # SQ_E_STATE: nothing measured yet
        E.upload(_starts(oracle_mod, shape)[0])
        E.step(10, every=2, correlate=True)
        E.step(3, every=3, correlate=True)
        E.corr_reset(first=2, count=1)                # replica 2 drops out
        G, S1, nm = E.corr_sums()
        assert list(nm) == [6, 6, 0, 6]
        for connected in (True, False):
            for n in (E.nt, 1):
                mean, err, used = E.correlator(n=n, connected=connected)
                rm, re, ru = _correlator_host(G, S1, nm, shape, n, connected)
                assert used == ru == 3
                assert np.array_equal(mean, rm), (connected, n, mean, rm)
                assert np.array_equal(err, re), (connected, n, err, re)
                assert np.all(err > 0)
        E.corr_reset(first=0, count=2)                # one replica left: no error bar
        mean, err, used = E.correlator()
        assert used == 1 and not err.any()
        with pytest.raises(StochQuantError):
            E.correlator(n=E.nt + 1)


def test_free_field_exact_law(gpu):
    """λ = 0: the Euler scheme's stationary two-point function is known in closed
    form, E[c(t)] = (1/Lz) Σ_k cos(2πkt/Lz) / (ω_k² (1 − Δτ ω_k² / 2)), ω_k² = m² + 2 − 2 cos(2πk/Lz)
    for the unconnected zero-momentum correlator.  A wrong normalisation or a wrong wrap misses it by
    many standard errors; the seeds are fixed."""
    shape, R, dtau, m2 = (8, 8, 8), 128, 0.05, 1.0
    Lz = shape[2]
    k = np.arange(Lz)
    w2 = m2 + 2.0 - 2.0 * np.cos(2.0 * np.pi * k / Lz)
    exact = np.array([np.sum(np.cos(2.0 * np.pi * k * t / Lz) / (w2 * (1.0 - dtau * w2 / 2.0))) / Lz
                      for t in range(5)])
    assert np.allclose(exact, [0.474686, 0.170697, 0.066686, 0.028571, 0.019048], atol=1e-6)
    with _ens(shape, R, dtau=dtau, m2=m2, lam=0.0, C=1.0, seeds=[1000 + r for r in range(R)]) as E:
        E.step(200)
        E.corr_reset()
        E.step(1600, every=20, correlate=True)
        mean, err, used = E.correlator(connected=False)
        assert used == R and not E.flags().any()
        assert list(E.corr_sums()[2]) == [80] * R
    ratio = (mean - exact) / err
    print("corr free field: (mean - exact) / err =", " ".join(f"{x:+.2f}" for x in ratio),
          " err =", " ".join(f"{x:.4f}" for x in err))
    assert np.all(np.abs(mean - exact) <= 4.0 * err), (mean, exact, err)
