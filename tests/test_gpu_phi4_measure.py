"""In-stream measurements of the single phi^4 lattice (Phi4Lattice.measure, set_momenta, corr_sums and the every= /
correlate= / momenta= keywords of step_hmc and step_hmc_cluster; sq_phi4_measure.hip) on the seven shapes of
test_gpu_phi4_hmc.CASES: every tile case of the step kernel, a plane that is its own z neighbour, odd Ly, prime Lz,
rows of several spans and 65,536 sites.

The reference is float64 NumPy with math.fsum over the downloaded field.  The bound on the device's double sums is
the project's 1e-10 x sum |terms| (test_gpu_phi4_ens_mala.py derives it); the largest sum here has N = 3 x 65,536
terms, for which a double sum in any order errs by at most (N + 4) 2^-53 < 2.2e-11 of that.  g and gp are
checked bit for bit against the z-ascending loop without fused multiply-add that include/stochquant.h states,
applied to the S and AB the device returned.
"""
import math

import numpy as np
import pytest

from test_gpu_phi4_hmc import CASES, THERM, _lat, _start
from test_oracle import same_bits

pytestmark = pytest.mark.gpu

TOL = 1e-10


def _momenta(shape):
    return [(0, 0), (1, 0), (0, 1), (shape[0] // 2, 1 % shape[1])]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _close(got, terms):
    """got against fsum(terms), within TOL x fsum(|terms|)"""
    t = np.asarray(terms, dtype=np.float64).ravel()
    return abs(got - math.fsum(t)) <= TOL * math.fsum(np.abs(t))


def _g(A, B=None):
    """g(t) = sum_z [A(z) A(z + t) + B(z) B(z + t)], z ascending, every product and sum rounded once"""
    Lz = len(A)
    out = np.zeros(Lz // 2 + 1)
    for t in range(Lz // 2 + 1):
        acc = 0.0
        for z in range(Lz):
            zt = (z + t) % Lz
            acc = acc + float(A[z]) * float(A[zt])
            if B is not None:
                acc = acc + float(B[z]) * float(B[zt])
        out[t] = acc
    return out


def _thermalised(shape, n=1, **kw):
    dtau, seed, _ = CASES[shape]
    lats = [_lat(shape, dtau, seed, **kw) for _ in range(n)]
    for X in lats:
        X.upload(_start(shape, seed))
        X.step(THERM)
    return lats


@pytest.mark.parametrize("shape", list(CASES))
def test_measure_against_fsum(gpu, shape):
    from stochquant_amd import Phi4Ensemble
    Lx, Ly, Lz = shape
    A, = _thermalised(shape)
    with A:
        A.set_momenta(_momenta(shape))
        assert A.momenta == _momenta(shape)
        m = A.measure(slices=True)
        only = A.measure()
        p = A.download().astype(np.float64)
    assert set(only) == {"sums"} and np.array_equal(_bits(only["sums"]), _bits(m["sums"]))
    fwd = [p * np.roll(p, -1, axis=ax) for ax in (2, 1, 0)]
    for got, terms in zip(m["sums"], (p, p ** 2, p ** 4, np.stack(fwd))):
        assert _close(got, terms), (got, math.fsum(np.ravel(terms)))
    for z in range(Lz):
        assert _close(m["S"][z], p[z])
    for k, (nx, ny) in enumerate(_momenta(shape)):
        cx, sx = Phi4Ensemble.momentum_table(Lx, nx)
        cy, sy = Phi4Ensemble.momentum_table(Ly, ny)
        cc, ss, sc, cs = np.outer(cy, cx), np.outer(sy, sx), np.outer(sy, cx), np.outer(cy, sx)
        for z in range(Lz):
            assert _close(m["AB"][k, z, 0], np.stack([p[z] * cc, -p[z] * ss])), (k, z)
            assert _close(m["AB"][k, z, 1], np.stack([p[z] * sc, p[z] * cs])), (k, z)
        assert np.array_equal(_bits(m["gp"][k]), _bits(_g(m["AB"][k, :, 0], m["AB"][k, :, 1]))), k
    assert np.array_equal(_bits(m["AB"][0, :, 0]), _bits(m["S"]))
    assert np.array_equal(_bits(m["AB"][0, :, 1]), _bits(np.zeros(Lz)))      # +0.0
    assert np.array_equal(_bits(m["g"]), _bits(_g(m["S"])))


def _check_accumulators(X, meas):
    G, Gp, S1 = np.zeros_like(meas[0]["g"]), np.zeros_like(meas[0]["gp"]), 0.0
    for m in meas:
        G, Gp, S1 = G + m["g"], Gp + m["gp"], S1 + m["sums"][0]
    acc = X.corr_sums()
    assert np.array_equal(_bits(acc["G"]), _bits(G)) and np.array_equal(_bits(acc["Gp"]), _bits(Gp))
    assert _bits(acc["S1"]) == _bits(S1) and acc["nmeas"] == acc["nmeas_p"] == len(meas)
    X.corr_reset()
    acc = X.corr_sums()
    assert not acc["G"].any() and not acc["Gp"].any() and acc["S1"] == 0.0 and acc["nmeas"] == acc["nmeas_p"] == 0


@pytest.mark.parametrize("shape", [(8, 2, 2), (64, 11, 29), (256, 16, 16)])
def test_in_flight_is_stand_alone(gpu, shape):
    A, B, C = _thermalised(shape, 3)
    with A, B, C:
        for X in (A, B):
            X.set_momenta(_momenta(shape))
        series, ra = A.step_hmc(6, nleap=3, every=2, correlate=True, momenta=True, record=True)
        rb, meas = [], []
        for _ in range(3):
            rb.append(B.step_hmc(2, nleap=3, record=True))
            meas.append(B.measure(slices=True))
        rc = C.step_hmc(6, nleap=3, record=True)
        assert series.shape == (3, 4)
        assert np.array_equal(_bits(series), _bits(np.stack([m["sums"] for m in meas])))
        assert np.array_equal(_bits(ra), _bits(np.concatenate(rb))) and np.array_equal(_bits(ra), _bits(rc))
        fa = A.download()
        assert same_bits(fa, B.download()) and same_bits(fa, C.download())
        assert not B.corr_sums()["nmeas"]        # a stand-alone measurement accumulates nothing
        _check_accumulators(A, meas)


@pytest.mark.parametrize("shape", [(64, 11, 29), (16, 4, 1)])
def test_in_flight_behind_cluster_sweeps(gpu, shape):
    A, B = _thermalised(shape, 2)
    with A, B:
        for X in (A, B):
            X.set_momenta(_momenta(shape))
        series, rh, bonds, labels = A.step_hmc_cluster(4, ntraj=1, nleap=2, every=2, correlate=True, momenta=True,
                                                       record=True)
        meas = []
        for r in range(4):
            assert np.array_equal(_bits(B.step_hmc(1, nleap=2, record=True)), _bits(rh[r:r + 1]))
            b, lab = B.cluster(1, record=True)
            assert np.array_equal(b[0], bonds[r]) and np.array_equal(lab[0], labels[r])
            if r % 2:
                meas.append(B.measure(slices=True))
        assert np.array_equal(_bits(series), _bits(np.stack([m["sums"] for m in meas])))
        assert same_bits(A.download(), B.download())
        _check_accumulators(A, meas)


def test_refusals_launch_nothing(gpu):
    from stochquant_amd import Phi4Lattice, StochQuantError
    shape = (16, 4, 1)
    A, B = _thermalised(shape, 2)
    refused = [(ValueError, None, lambda: A.step_hmc(2, nleap=2, every=0, correlate=True)),
               (StochQuantError, -4, lambda: A.step_hmc(2, nleap=2, every=1, momenta=True)),
               (StochQuantError, -1, lambda: A.set_momenta([(0, 0)] * 9))]
    with A, B:
        for err, code, call in refused:
            launches = A.perf()["kernel_launches"]
            with pytest.raises(err) as ei:
                call()
            assert code is None or ei.value.code == code
            assert A.perf()["kernel_launches"] == launches and A.momenta == []
            sa, sb = A.step_hmc(2, nleap=2, every=1), B.step_hmc(2, nleap=2, every=1)
            assert np.array_equal(_bits(sa), _bits(sb)) and same_bits(A.download(), B.download())
    with Phi4Lattice((16, 4, 4), dtau=0.05, comm="loopback", nslabs=2) as S:
        launches = S.perf()["kernel_launches"]
        for call in (lambda: S.step_hmc(2, nleap=2, every=1), S.measure, lambda: S.set_momenta([(0, 0)])):
            with pytest.raises(StochQuantError) as ei:
                call()
            assert ei.value.code == -4
        assert S.perf()["kernel_launches"] == launches and S.step_counter == 0
