"""Swendsen-Wang cluster sweeps of the phi^4 ensemble on the GPU (sq_phi4_ens_cluster, sq_phi4_ens_step_hmc_cluster)
against the NumPy statement of the header's definition (phi4_cluster_model.py).  The oracle tests' fields are made in
NumPy and uploaded; test_phi4_cluster_model.py asserts their properties without a GPU.

Tolerances.  Bond bits, labels, fields, counters and statistics: exact.  A bond with |exp(-2βt) - u| < 1e-12 could
not be decided across two exp implementations; the CPU test shows the inputs have none, and a test here fails if it
meets one.  The two statistical tests take their bounds from the CPU tests and from
test_gpu_phi4_ens_sampler_edges.py; both are derived there."""
import math

import numpy as np
import pytest

import phi4_cluster_model as cm
import test_gpu_phi4_ens_hmc as hmc
from test_gpu_phi4_ens_heun import CLAMP
from test_gpu_phi4_ens_hmc import CLASS_SHAPES
from test_gpu_phi4_ens_mala import THERM
from test_gpu_phi4_ens_sampler_edges import LAW_DTAU, _metropolis
from test_oracle import same_bits
from test_phi4_ens_shapes import GPU_SHAPES, assert_shape

pytestmark = pytest.mark.gpu

SHAPES = list(GPU_SHAPES)
M2, LAM = 0.5, 1.0
SIGN = np.uint32(0x80000000)


def _ens(shape, R=4, C=None, seeds=None, **kw):
    from stochquant_amd import Phi4Ensemble
    kw.setdefault("dtau", cm.ORACLE_DTAU)
    kw.setdefault("m2", M2)
    kw.setdefault("lam", LAM)
    kw.setdefault("clamp", CLAMP)
    return Phi4Ensemble(shape, R, C=list(np.resize(cm.ORACLE_C, R)) if C is None else C,
                        seeds=cm.oracle_seeds(R) if seeds is None else seeds, **kw)


def _lat(E, flat):
    return np.ascontiguousarray(flat).reshape((-1,) + E.lattice_shape)


def _flat(E, f):
    return np.ascontiguousarray(f).reshape(f.shape[0], -1)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _betas(E):
    p = E.get_params()
    return [cm.beta(cm.record(p["dtau"][r], p["m2"][r], p["lam"][r], p["C"][r])) for r in range(E.R)]


def _others(E):
    """Everything a sweep must leave alone."""
    G, S1, n = E.corr_sums()
    p = E.get_params()
    return {"steps": np.asarray(E.step_counter), "flags": np.asarray(E.flags()), "hmc": E.hmc_stats(),
            "mala": E.mala_stats(), "xstat": E.exchange_stats(), "walkers": E.walkers(),
            "round": np.asarray(E.exchange_round), "ladder": np.asarray(E.ladder), "G": _bits(G), "S1": _bits(S1),
            "nmeas": np.asarray(n), "psteps": np.asarray(E.perf()["steps"]),
            **{"par_" + k: np.asarray(v) for k, v in p.items()}}


def _state(E):
    s = _others(E)
    s.update(field=E.download().view(np.uint32), cstat=E.cluster_stats(), sweep=np.asarray(E.cluster_sweep),
             launches=np.asarray(E.perf()["kernel_launches"]))
    return s


def _same(a, b, skip=()):
    for k in a:
        if k not in skip:
            assert np.array_equal(a[k], b[k]), k


def check_sweeps(E, seeds, nsweeps):
    """Run cluster(nsweeps, record=True) on E from the state it is in and check the records, the fields, the
    statistics and the counters against the model."""
    R, shape, c0 = E.R, E.shape, E.cluster_sweep
    sites = shape[0] * shape[1] * shape[2]
    betas = _betas(E)
    phi = _flat(E, E.download())
    stats = E.cluster_stats().copy()
    others, launches = _others(E), E.perf()["kernel_launches"]
    bonds, labels = E.cluster(nsweeps, record=True)
    assert bonds.shape == labels.shape == (nsweeps, R, sites) and bonds.dtype == np.uint8 and labels.dtype == np.int32
    for i in range(nsweeps):
        res = cm.sweep(phi, betas, seeds, c0 + i, shape)
        assert res["margin"] >= 1e-12, ("a bond within 1e-12 of a tie: another input, not another bound", res["margin"])
        assert np.array_equal(bonds[i], res["bits"]), (shape, c0 + i, np.argwhere(bonds[i] != res["bits"])[:8])
        # the labels are the components of the kernel's own bonds (the model's, the bits being equal)
        assert np.array_equal(labels[i], res["labels"]), (shape, c0 + i, np.argwhere(labels[i] != res["labels"])[:8])
        odd = (cm.blocks(seeds, c0 + i, sites)[:, :, 3] & 1).astype(bool)
        flip = np.take_along_axis(odd, labels[i].astype(np.int64), axis=1)
        root = labels[i] == np.arange(sites)[None, :]
        phi = (phi.view(np.uint32) ^ (flip.astype(np.uint32) << np.uint32(31))).view(np.float32)
        inc = np.stack([root.sum(axis=1), (root & odd).sum(axis=1), flip.sum(axis=1)], axis=1)
        assert np.array_equal(inc, res["stats"])
        stats[:, 0] += 1
        stats[:, 1:4] += inc
    assert same_bits(E.download(), _lat(E, phi)), "sign bits toggled exactly on the clusters whose root word is odd"
    got = E.cluster_stats()
    assert np.array_equal(got, stats), (got, stats)
    assert not got[:, 4].any(), "the pass bound was reached"
    assert E.cluster_sweep == c0 + nsweeps
    assert E.perf()["kernel_launches"] == launches + nsweeps, "one launch per sweep"
    _same(others, _others(E))
    return bonds, labels


@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_model(gpu, shape):
    assert_shape(shape)
    seeds = cm.oracle_seeds(4)
    with _ens(shape) as E:
        assert E.cluster_sweep == 0 and not E.cluster_stats().any()
        E.upload(_lat(E, cm.oracle_fields(shape)))
        first = None
        for c in cm.ORACLE_SWEEPS:
            E.cluster_sweep = c
            bonds, labels = check_sweeps(E, seeds, 2)
            first = (bonds[0], labels[0]) if first is None else first
        st = E.cluster_stats()
        assert st[:, 0].tolist() == [4] * 4
    sites = shape[0] * shape[1] * shape[2]
    path = cm.serpentine(shape)
    assert (first[1][3][path] == 0).all() and np.bincount(first[1][1]).max() > sites // 2
    print(f"cluster {shape} stats {st.tolist()}", flush=True)


def _thermal(shape, R=4, **kw):
    E = _ens(shape, R=R, dtau=hmc._dtau(shape), **kw)
    E.init_field(0.5)
    E.step(THERM)
    return E


def test_sweeps_split_over_calls(gpu):
    shape = (8, 17, 31)
    with _thermal(shape) as A, _thermal(shape) as B:
        for E in (A, B):
            E.cluster_sweep = 2 ** 32 - 2              # the low word wraps inside the call
        ba, la = A.cluster(3, record=True)
        parts = [B.cluster(1, record=True) for _ in range(3)]
        assert np.array_equal(ba, np.concatenate([p[0] for p in parts]))
        assert np.array_equal(la, np.concatenate([p[1] for p in parts]))
        _same(_state(A), _state(B))
        assert A.cluster_sweep == 2 ** 32 + 1 and A.cluster_stats()[:, 0].tolist() == [3] * 4
        assert A.cluster(0) is None and A.cluster(0, record=True)[0].shape == (0, 4, 8 * 17 * 31)
        assert A.cluster(2) is None and A.cluster_sweep == 2 ** 32 + 3
        A.cluster_reset(first=1, count=2)
        assert A.cluster_stats()[:, 0].tolist() == [5, 0, 0, 5] and not A.cluster_stats(1, 2).any()
        A.cluster_reset()
        assert not A.cluster_stats().any() and A.cluster_sweep == 2 ** 32 + 3


def test_a_replica_does_not_depend_on_the_others(gpu):
    shape = (16, 4, 31)
    seeds = cm.oracle_seeds(5)
    C = list(np.resize(cm.ORACLE_C[:3], 5))
    with _thermal(shape, R=5, C=C, seeds=seeds) as A, _thermal(shape, R=5, C=C, seeds=seeds) as L:
        L.set_ladder(5)                                     # a ladder changes nothing
        ba, la = A.cluster(2, record=True)
        bl, ll = L.cluster(2, record=True)
        assert np.array_equal(ba, bl) and np.array_equal(la, ll) and same_bits(A.download(), L.download())
        assert np.array_equal(A.cluster_stats(), L.cluster_stats()) and list(L.walkers()) == list(range(5))
        for r in (0, 3, 4):
            with _thermal(shape, R=1, C=[C[r]], seeds=[seeds[r]]) as B:
                bb, lb = B.cluster(2, record=True)
                assert np.array_equal(ba[:, r], bb[:, 0]) and np.array_equal(la[:, r], lb[:, 0])
                assert same_bits(A.download(r, 1), B.download())
                assert np.array_equal(A.cluster_stats(r, 1), B.cluster_stats())


@pytest.mark.parametrize("shape", [(8, 8, 8), (64, 16, 8), (16, 24, 24), (32, 24, 24)])
def test_non_finite_and_zero_sites(gpu, shape):
    """NaN (both signs, with payloads), +-inf and +-0 planted in field 0: a NaN or a zero never bonds, inf inf > 0
    bonds for certain, and only sign bits change."""
    assert [assert_shape(shape)["K"]] == [{(8, 8, 8): 1, (64, 16, 8): 2, (16, 24, 24): 4, (32, 24, 24): 8}[shape]]
    Lx, Ly, Lz = shape
    sites = Lx * Ly * Lz
    f = cm.oracle_fields(shape)
    u = f.view(np.uint32)
    fwd = cm.forward(shape)
    at = {"nan": 5, "-nan": Lx * Ly + 9, "inf": 2 * Lx * Ly + 3, "-inf": sites - 1, "zero": 3 * Lx + 2,
          "-zero": sites // 2 + 1}
    u[0, at["nan"]], u[0, at["-nan"]] = 0x7FC12345, 0xFFA00001
    f[0, at["inf"]] = f[0, fwd[0][at["inf"]]] = f[0, fwd[1][at["inf"]]] = np.inf       # inf inf in x and in y
    f[0, at["-inf"]] = f[0, fwd[2][at["-inf"]]] = -np.inf                             # across the z wrap
    f[0, at["zero"]], f[0, at["-zero"]] = 0.0, -0.0
    f[1, 7] = np.nan
    seeds = cm.oracle_seeds(4)
    with _ens(shape) as E:
        E.upload(_lat(E, f))
        E.cluster_sweep = 11
        bonds, labels = check_sweeps(E, seeds, 2)
        after = _flat(E, E.download()).view(np.uint32)
    assert not ((after ^ u) & ~SIGN).any(), "only sign bits"
    for b, lab in zip(bonds, labels):
        for k in ("nan", "-nan", "zero", "-zero"):
            i = at[k]
            assert b[0, i] == 0 and lab[0, i] == i and (lab[0] == i).sum() == 1, k
            back = [int(np.nonzero(fwd[mu] == i)[0][0]) for mu in range(3)]
            assert all(not (b[0, j] >> mu) & 1 for mu, j in enumerate(back)), k
        assert b[0, at["inf"]] & 3 == 3 and (b[0, at["-inf"]] >> 2) & 1
        assert lab[0, at["inf"]] == lab[0, fwd[0][at["inf"]]] == lab[0, fwd[1][at["inf"]]]
        assert lab[0, at["-inf"]] == lab[0, fwd[2][at["-inf"]]]
        assert b[1, 7] == 0 and lab[1, 7] == 7


def test_a_replica_without_noise_is_refused(gpu, sqlib):
    from stochquant_amd import StochQuantError
    shape = (8, 8, 8)
    with _thermal(shape) as E:
        E.step_hmc(2, nleap=2)
        E.cluster(1)
        before = _state(E)
        E.set_params(C=0.0, first=2, count=1)
        for call in (lambda: E.cluster(1), lambda: E.cluster(0), lambda: E.cluster(2, record=True),
                     lambda: E.step_hmc_cluster(2, ntraj=2, nleap=2), lambda: E.step_hmc_cluster(0)):
            with pytest.raises(StochQuantError) as ei:
                call()
            assert ei.value.code == -4                     # SQ_E_STATE
        E.set_params(C=cm.ORACLE_C[2], first=2, count=1)
        _same(before, _state(E))
        # the C call's own argument checks, where the Python wrapper would raise first
        for args in ((2, 3, 1, 0, 2, None, 0, None, None, None), (2, 2, 0, 0, 0, None, 0, None, None, None),
                     (-1, 2, 1, 0, 0, None, 0, None, None, None), (2, -1, 1, 0, 0, None, 0, None, None, None),
                     (2, 2, 1, 0, 0, None, 1, None, None, None), (2, 2, 1, 0, 0, None, 2, None, None, None)):
            assert sqlib.sq_phi4_ens_step_hmc_cluster(E._h, *args) == -1, args
        assert sqlib.sq_phi4_ens_cluster(E._h, -1, None, None) == -1
        _same(before, _state(E))


@pytest.mark.parametrize("shape", CLASS_SHAPES)
def test_fused_call_is_the_loop(gpu, shape):
    assert_shape(shape)
    with _thermal(shape) as A, _thermal(shape) as B:
        ser, rh, bo, la = A.step_hmc_cluster(3, ntraj=2, nleap=3, every=1, correlate=True, record=True)
        sites = shape[0] * shape[1] * shape[2]
        assert ser.shape == (6, 4, 4) and rh.shape == (6, 4, 4) and bo.shape == la.shape == (3, 4, sites)
        parts = []
        for _ in range(3):
            s, r = B.step_hmc(2, nleap=3, every=1, correlate=True, record=True)
            b, l = B.cluster(1, record=True)
            parts.append((s, r, b, l))
        for got, k in ((ser, 0), (rh, 1)):
            assert np.array_equal(_bits(got), _bits(np.concatenate([p[k] for p in parts]))), k
        assert np.array_equal(bo, np.concatenate([p[2] for p in parts]))
        assert np.array_equal(la, np.concatenate([p[3] for p in parts]))
        _same(_state(A), _state(B))
        assert A.cluster_sweep == 3 and A.cluster_stats()[:, 0].tolist() == [3] * 4 and not A.cluster_stats()[:, 4].any()
        assert (rh[:, :, 2] == 1.0).any() and A.cluster_stats()[:, 3].any()
        with _thermal(shape) as C:                          # without records and measurements: the same fields
            assert C.step_hmc_cluster(3, ntraj=2, nleap=3) is None
            assert same_bits(C.download(), A.download())
            assert np.array_equal(C.cluster_stats(), A.cluster_stats()) and list(C.step_counter) == list(A.step_counter)


def test_detailed_balance_by_enumeration(gpu):
    """8 x 2 x 2, R = 4096: the live sites x in {0, 1} carry fixed magnitudes with random start signs, every other
    site is 1e-30 and decoupled for certain.  Eight snapshots ten sweeps apart; the histogram of the 256 live sign
    configurations against the exact weights of that graph (single x-bond, doubled y- and z-bonds).  The bound and
    the minimum expected count are test_phi4_cluster_model.py's, which runs the model on the same graph and shows
    that the two wrong couplings fail at this sample size."""
    shape, R = cm.DB_SHAPE, cm.DB_R
    live = cm.db_live(shape)
    start = cm.db_start(shape, R)
    with _ens(shape, R=R, C=[cm.DB_C] * R, seeds=cm.oracle_seeds(R, 4321)) as E:
        beta = _betas(E)[0]
        E.upload(_lat(E, start))
        codes = []
        for _ in range(cm.DB_SNAPSHOTS):
            E.cluster(cm.DB_GAP)
            f = _flat(E, E.download())
            codes.append(cm.sign_code(f, live))
        st = E.cluster_stats()
    assert np.array_equal(np.abs(f), np.abs(start)) and not st[:, 4].any()
    assert st[:, 0].tolist() == [cm.DB_SNAPSHOTS * cm.DB_GAP] * R
    p = cm.exact_weights(cm.db_magnitudes(), live, beta, shape)
    chi2, emin = cm.chi2(np.concatenate(codes), p)
    print(f"cluster detailed balance chi2 {chi2:.1f} bound {cm.DB_CHI2_BOUND:.1f} min expected {emin:.2f}", flush=True)
    assert emin >= cm.DB_MIN_EXPECTED and chi2 <= cm.DB_CHI2_BOUND, (chi2, emin)


def test_the_interacting_law_against_metropolis(gpu):
    """test_gpu_phi4_ens_sampler_edges.py's HMC run (8 x 4 x 4, R = 256, m2 = 0.25, lam = 6, C = 0.7; 300 Heun steps,
    1500 randomised trajectories of nleap = 8, a record each) with one cluster sweep after every trajectory: <phi^2>
    against the Metropolis fixture, |mean - ref| < 4 sqrt(sem^2 + sem_ref^2), that test's bound."""
    ref = _metropolis()
    tgt = ref["target"]
    shape, R = tuple(ref["shape"]), 256
    assert shape == (8, 4, 4) and (tgt["m2"], tgt["lam"], tgt["C"]) == (0.25, 6.0, 0.7)
    with hmc._ens(shape, R, dtau=LAW_DTAU["hmc"], m2=tgt["m2"], lam=tgt["lam"], C=tgt["C"], seeds=None,
                  seed=4242) as E:
        E.step(300, scheme="heun")
        ser = E.step_hmc_cluster(1500, ntraj=1, nleap=8, randomize=True, every=1)
        assert not E.flags().any()
        stats, cst = E.hmc_stats(), E.cluster_stats()
    per = ser[:, :, 1].mean(axis=0) / 128.0
    mean, sem = float(per.mean()), float(per.std(ddof=1) / np.sqrt(R))
    acc = float(stats[:, 1].sum()) / float(stats[:, 0].sum())
    err = math.sqrt(sem * sem + tgt["sem"] ** 2)
    print(f"LAW hmc+cluster PHI2 {mean:.6f} +- {sem:.6f}  metropolis {tgt['phi2']:.6f} +- {tgt['sem']:.6f}  deviation "
          f"{(mean - tgt['phi2']) / err:+.2f} sigma  acceptance {acc:.4f}  clusters per sweep "
          f"{cst[:, 1].sum() / cst[:, 0].sum():.1f}  flipped sites per sweep {cst[:, 3].sum() / cst[:, 0].sum():.1f}",
          flush=True)
    assert stats[:, 0].tolist() == [1500] * R and not stats[:, 2].any()
    assert cst[:, 0].tolist() == [1500] * R and not cst[:, 4].any()
    assert abs(mean - tgt["phi2"]) < 4.0 * err, (mean, sem, tgt)
    assert 0.6 <= acc <= 0.9, acc
