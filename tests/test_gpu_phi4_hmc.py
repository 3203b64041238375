"""HMC trajectories of the single phi^4 lattice on the GPU (sq_phi4_hmc.hip, sq_phi4_step_hmc,
Phi4Lattice.step_hmc) against the composed oracle of test_gpu_phi4_ens_hmc.py (oracle.phi4_step, oracle.philox,
float64 NumPy with math.fsum) and against a Phi4Ensemble of one replica.

Parameters: m2, lambda, C and the clamp of the ensemble tests' replica 0.  Start fields: 0.5 x NumPy normals of
the case's seed, thermalised with 20 Euler steps on the device.  dtau = round(0.4 / sqrt(V), 5) as in the ensemble
tests (0.004 at 256 x 16 x 16, where that rule accepted everything), the seed the first of 11, 12, .. for which
the oracle alone, run on the CPU with the same start and thermalisation, accepts some and rejects some of the 12
trajectories with |exp(-dH) - u| > 0.01 throughout: the verdicts below are that run's.

Tolerances: fields, u, L, verdicts, counters and counts exact; dH within 1e-10 x the sum of the absolute values
of all summed terms over sig^2, the ensemble tests' bound (test_gpu_phi4_ens_mala.py derives it; the lattice sums
the same terms in another fixed order).

The context has no guard-flag read-back outside frames: a trip shows as verdict 2 and in the third counter.
"""
import numpy as np
import pytest

from test_gpu_phi4_ens_heun import CLAMP, LAM, M2
from test_gpu_phi4_ens_hmc import check_trajectories, dH_reference, trajectory
from test_gpu_phi4_ens_mala import CS, _record
from test_oracle import same_bits

pytestmark = pytest.mark.gpu

THERM = 20
# shape: (dtau, seed, the oracle's verdicts of 4 + 2 + 2 trajectories of 3 steps, then 4 of up to 5)
CASES = {
    (8, 2, 2): (0.07071, 11, [0, 1, 0, 0, 1, 1, 1, 1, 1, 0, 0, 1]),       # narrowest row, tile taller than Ly
    (16, 4, 1): (0.05, 11, [1, 1, 1, 0, 1, 1, 0, 0, 1, 1, 1, 1]),         # the plane its own z neighbour
    (64, 11, 29): (0.0028, 20, [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1]),     # odd Ly, partial tile, prime Lz
    (256, 4, 6): (0.0051, 11, [1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1]),      # full-wave rows
    (512, 2, 5): (0.00559, 11, [1, 1, 1, 1, 1, 0, 1, 1, 1, 0, 1, 1]),     # two segments per lane
    (768, 3, 4): (0.00417, 14, [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1]),     # three spans per row
    (256, 16, 16): (0.004, 11, [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1]),     # 65,536 sites: past the ensemble
}


def _lat(shape, dtau, seed, **kw):
    from stochquant_amd import Phi4Lattice
    kw.setdefault("clamp", CLAMP)
    kw.setdefault("C", CS[0])
    return Phi4Lattice(shape, dtau=dtau, m2=M2[0], lam=LAM[0], seed=seed, **kw)


def _start(shape, seed):
    return (0.5 * np.random.default_rng(seed).standard_normal(tuple(reversed(shape)))).astype(np.float32)


@pytest.mark.parametrize("shape", list(CASES))
def test_against_the_composed_oracle(gpu, dev_oracle, shape):
    dtau, seed, want = CASES[shape]
    par = (dtau, M2[0], LAM[0], CS[0], seed)
    with _lat(shape, dtau, seed) as A, _lat(shape, dtau, seed) as B:
        for X in (A, B):
            X.upload(_start(shape, seed))
            X.step(THERM)
        start, s0 = A.download(), A.step_counter
        assert s0 == THERM
        recs, after = [], []
        for n, nleap, rnd in ((4, 3, False), (2, 3, False), (2, 3, False), (4, 5, True)):
            recs.append(A.step_hmc(n, nleap=nleap, randomize=rnd, record=True))
            after.append(A.download())
        rec = np.concatenate(recs)
        assert rec.shape == (12, 4)
        # the same eight trajectories from one call
        rb = B.step_hmc(8, nleap=3, record=True)
        assert np.array_equal(rb.view(np.uint64), rec[:8].view(np.uint64))
        assert same_bits(B.download(), after[2]) and B.step_counter == s0 + 8
        assert A.step_counter == s0 + 12
        stats = A.hmc_stats()
    f3, v3, l3 = check_trajectories(dev_oracle, shape, par, start, s0, rec[:8], 3, False)
    f5, v5, l5 = check_trajectories(dev_oracle, shape, par, f3[-1], s0 + 8, rec[8:], 5, True)
    fields, verdicts, lengths = f3 + f5, v3 + v5, l3 + l5
    print(f"HMC lattice {shape} dtau {dtau} verdicts {verdicts} lengths {lengths}", flush=True)
    for done, got in zip((4, 6, 8, 12), after):
        assert same_bits(got, fields[done - 1]), f"after trajectory {done}: " \
            f"{np.count_nonzero(got != fields[done - 1])} sites differ"
    assert list(stats) == [12, verdicts.count(1), verdicts.count(2), sum(lengths)]
    assert verdicts == want and {0, 1} <= set(verdicts)


@pytest.mark.parametrize("shape", [(8, 8, 8), (64, 11, 29), (32, 32, 32)])
def test_is_the_ensemble_replica(gpu, dev_oracle, shape):
    from stochquant_amd import Phi4Ensemble
    dtau, seed = round(0.4 / (shape[0] * shape[1] * shape[2]) ** 0.5, 5), 11
    par = (dtau, M2[0], LAM[0], CS[0], seed)
    with _lat(shape, dtau, seed) as A, \
            Phi4Ensemble(shape, 1, dtau=dtau, m2=M2[:1], lam=LAM[:1], C=CS[:1], seeds=[seed], clamp=CLAMP) as E:
        A.upload(_start(shape, seed))
        A.step(THERM)
        phi, s0 = A.download(), A.step_counter
        E.upload(phi[None])
        E.step_counter = [s0]
        ra = A.step_hmc(6, nleap=4, randomize=True, record=True)
        re = E.step_hmc(6, nleap=4, randomize=True, record=True)[1][:, 0]
        assert same_bits(A.download(), E.download()[0])
        assert np.array_equal(ra[:, 1:].view(np.uint64), re[:, 1:].view(np.uint64)), (ra, re)
        assert list(A.hmc_stats()) == list(E.hmc_stats()[0]) and A.step_counter == int(E.step_counter[0])
    R = _record(*par[:4])
    for k in range(6):
        p1, pm, pL, hit = trajectory(dev_oracle, shape, par, phi, s0 + k, int(ra[k, 3]))
        assert not hit
        _, bound = dH_reference(phi, p1, pm, pL, R)
        assert abs(ra[k, 0] - re[k, 0]) <= 1e-10 * bound, (k, ra[k, 0], re[k, 0], bound)
        if ra[k, 2] == 1.0:
            phi = pL


@pytest.mark.parametrize("shape", [(8, 2, 2), (256, 4, 6)])
def test_a_trip_inside_the_trajectory(gpu, dev_oracle, shape):
    """The ensemble test's input: m2 = -0.5 without a quartic term pushes a uniform field of 9.0 outwards; phi_1 =
    9.0 + 0.225 + noise of width 0.03 stays below the clamp of 10, the second interior step's g is beyond it.
    Verdict 2, the field kept bit for bit, a guard trip counted; the next trajectory, one step long, is ordinary."""
    from stochquant_amd import Phi4Lattice
    par = (0.05, -0.5, 0.0, 0.1, 11)
    start = np.full(tuple(reversed(shape)), 9.0, dtype=np.float32)
    phi1, _, _, hit = trajectory(dev_oracle, shape, par, start, 0, 3, clamp=10.0)
    assert float(np.max(np.abs(phi1))) < 9.5 and hit
    assert not trajectory(dev_oracle, shape, par, start, 1, 1, clamp=10.0)[3]
    with Phi4Lattice(shape, dtau=par[0], m2=par[1], lam=par[2], C=par[3], seed=par[4], clamp=10.0) as A:
        A.upload(start)
        rec = A.step_hmc(1, nleap=3, record=True)
        assert rec[0, 2] == 2.0 and rec[0, 3] == 3.0
        assert same_bits(A.download(), start) and A.step_counter == 1
        assert list(A.hmc_stats()) == [1, 0, 1, 3]
        rec1 = A.step_hmc(1, nleap=1, record=True)
        got = A.download()
        assert list(A.hmc_stats()) == [2, int(rec1[0, 2]), 1, 4]
    check_trajectories(dev_oracle, shape, par, start, 0, rec, 3, False, clamp=10.0)
    fields, verdicts, _ = check_trajectories(dev_oracle, shape, par, start, 1, rec1, 1, False, clamp=10.0)
    assert verdicts[0] in (0, 1) and same_bits(got, fields[0])


def test_refusals_leave_the_context_running(gpu, sqlib):
    from stochquant_amd import Phi4Lattice, Qm1dChain, StochQuantError
    shape, dtau, seed = (16, 4, 2), 0.05, 11
    ARG, STATE = -1, -4
    with _lat(shape, dtau, seed) as A, _lat(shape, dtau, seed) as B:
        for X in (A, B):
            X.upload(_start(shape, seed))
            X.step(THERM)
        launches = A.perf()["kernel_launches"]
        call = lambda h, *a: sqlib.sq_phi4_step_hmc(h, *a)      # noqa: E731
        assert call(A._h, 2, 0, 0, None) == ARG and call(A._h, 2, 4097, 0, None) == ARG
        assert call(A._h, -1, 3, 0, None) == ARG and call(None, 2, 3, 0, None) == ARG
        assert sqlib.sq_last_error().decode() != ""
        A.set_noise(0.0)
        assert call(A._h, 2, 3, 0, None) == STATE and call(A._h, 0, 3, 1, None) == STATE
        with pytest.raises(StochQuantError):
            A.step_hmc(2, nleap=3)
        A.set_noise(CS[0])
        assert call(A._h, 0, 3, 0, None) == 0
        assert A.perf()["kernel_launches"] == launches and A.step_counter == THERM and not A.hmc_stats().any()
        ra, rb = A.step_hmc(3, nleap=2, record=True), B.step_hmc(3, nleap=2, record=True)
        assert np.array_equal(ra.view(np.uint64), rb.view(np.uint64)) and same_bits(A.download(), B.download())
        assert list(A.hmc_stats()) == list(B.hmc_stats()) and A.hmc_stats()[0] == 3
    with Phi4Lattice((16, 4, 4), dtau=dtau, comm="loopback", nslabs=2) as S:
        launches = S.perf()["kernel_launches"]
        assert call(S._h, 2, 3, 0, None) == STATE and sqlib.sq_phi4_hmc_stats(S._h, None) == STATE
        assert S.perf()["kernel_launches"] == launches and S.step_counter == 0
    with Qm1dChain(16, 0.1, 0.002) as Q:
        assert call(Q._h, 2, 3, 0, None) == STATE and sqlib.sq_phi4_hmc_reset(Q._h) == STATE
