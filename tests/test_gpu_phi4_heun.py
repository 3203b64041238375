"""The Heun step of the single phi^4 lattice on the GPU (sq_phi4_heun.hip, sq_phi4_step_heun,
Phi4Lattice.step(scheme="heun")) against the CPU oracle's Heun entry (oracle.phi4_heun_step, written from the
header's definition), against a Phi4Ensemble of one replica, and its in-stream measurements against stand-alone
ones.  Shapes: the seven of test_gpu_phi4_hmc.CASES (every tile case of the step kernel, a plane that is its own z
neighbour, odd and prime extents, one to three spans per row, 65,536 sites).

Tolerances: none.  Fields, counters, series rows and accumulators are compared bit for bit; the measurement's own
arithmetic is held against fsum by test_gpu_phi4_measure.py.
"""
import numpy as np
import pytest

from test_gpu_phi4_ens_heun import CLAMP, LAM, M2
from test_gpu_phi4_ens_mala import CS
from test_gpu_phi4_hmc import CASES, THERM, _lat, _start
from test_gpu_phi4_measure import _bits, _check_accumulators, _momenta
from test_oracle import HEUN_GUARD_IDS, HEUN_GUARD_PARAMS, assert_heun_guard_maxima, heun_guard_field, same_bits

pytestmark = pytest.mark.gpu

# (shape, C, first counter): noise on everywhere, noise off on a narrow and a two-segment tile, and one call
# whose counter crosses into the high word
ORACLE_CASES = [(s, CS[0], 0) for s in CASES] + [((8, 2, 2), 0.0, 0), ((512, 2, 5), 0.0, 0),
                                                 ((64, 11, 29), CS[0], 2 ** 32 - 2)]


@pytest.mark.parametrize("shape,C,s0", ORACLE_CASES)
def test_bitwise_against_the_oracle(gpu, dev_oracle, shape, C, s0):
    dtau, seed, _ = CASES[shape]
    p = dev_oracle.phi4_params(shape, dtau, M2[0], LAM[0], seed, clamp=CLAMP, C=C)
    phi0 = dev_oracle.phi4_init(p, 0.5)
    with _lat(shape, dtau, seed, C=C) as A, _lat(shape, dtau, seed, C=C) as B:
        for X in (A, B):
            X.upload(phi0)
            X.step_counter = s0
        assert A.step(3, scheme="heun") is None
        A.step(2, scheme="heun")
        B.step(5, scheme="heun")
        got, twin = A.download(), B.download()
        assert A.step_counter == B.step_counter == s0 + 5
    ref = phi0
    for k in range(5):
        ref, _ = dev_oracle.phi4_heun_step(p, ref, s0 + k)
    assert same_bits(got, ref), f"{np.count_nonzero(got != ref)} sites differ, max {np.max(np.abs(got - ref))}"
    assert same_bits(twin, ref)


@pytest.mark.parametrize("case,shape", HEUN_GUARD_PARAMS, ids=HEUN_GUARD_IDS)
def test_guard_stage_by_stage(gpu, oracle_mod, case, shape):
    """One Heun step of test_oracle.HEUN_GUARD_CASES (C = 0, clamp 1000): no maximum at the clamp, max |e| alone,
    max |p| and max |e|, max |p| alone.  The context keeps no guard flag outside frames: the field decides."""
    from stochquant_amd import Phi4Lattice
    dt, m2, lam = case[3]
    p = oracle_mod.phi4_params(shape, dt, m2, lam, 1, clamp=CLAMP, C=0.0)
    phi0 = heun_guard_field(case, shape)
    with Phi4Lattice(shape, dtau=dt, m2=m2, lam=lam, C=0.0, seed=1, clamp=CLAMP) as A:
        A.upload(phi0)
        A.step(1, scheme="heun")
        got = A.download()
        assert A.step_counter == 1
    ref, maxima = oracle_mod.phi4_heun_step(p, phi0, 0)
    assert_heun_guard_maxima(case, maxima)
    assert same_bits(got, ref), case[0]


@pytest.mark.parametrize("shape", [(8, 8, 8), (64, 11, 29)])
def test_is_the_ensemble_replica(gpu, shape):
    from stochquant_amd import Phi4Ensemble
    dtau, seed = round(0.4 / (shape[0] * shape[1] * shape[2]) ** 0.5, 5), 11
    with _lat(shape, dtau, seed) as A, \
            Phi4Ensemble(shape, 1, dtau=dtau, m2=M2[:1], lam=LAM[:1], C=CS[:1], seeds=[seed], clamp=CLAMP) as E:
        A.upload(_start(shape, seed))
        A.step(THERM)
        E.upload(A.download()[None])
        E.step_counter = [A.step_counter]
        A.step(6, scheme="heun")
        E.step(6, scheme="heun")
        assert same_bits(A.download(), E.download()[0])
        assert A.step_counter == int(E.step_counter[0]) == THERM + 6


@pytest.mark.parametrize("shape", [(16, 4, 1), (512, 2, 5)])
def test_in_stream_is_stand_alone(gpu, shape):
    dtau, seed, _ = CASES[shape]
    with _lat(shape, dtau, seed) as A, _lat(shape, dtau, seed) as B:
        for X in (A, B):
            X.upload(_start(shape, seed))
            X.step(THERM)
            X.set_momenta(_momenta(shape))
        series = A.step(4, scheme="heun", every=2, correlate=True, momenta=True)
        meas = []
        for _ in range(2):
            B.step(2, scheme="heun")
            meas.append(B.measure(slices=True))
        assert series.shape == (2, 4)
        assert np.array_equal(_bits(series), _bits(np.stack([m["sums"] for m in meas])))
        assert same_bits(A.download(), B.download()) and A.step_counter == B.step_counter == THERM + 4
        _check_accumulators(A, meas)


def test_refusals_launch_nothing(gpu, sqlib):
    from stochquant_amd import Phi4Lattice, Qm1dChain, StochQuantError
    ARG, STATE = -1, -4
    with _lat((16, 4, 2), 0.05, 11) as A:
        launches = A.perf()["kernel_launches"]
        assert sqlib.sq_phi4_step_heun(A._h, -1) == ARG and sqlib.sq_phi4_step_heun(A._h, 0) == 0
        assert sqlib.sq_phi4_step_heun_meas(A._h, 2, 0, None, 0) == ARG
        assert sqlib.sq_phi4_step_heun_meas(A._h, 2, 1, None, 4) == ARG
        with pytest.raises(StochQuantError) as ei:
            A.step(2, scheme="heun", every=1, momenta=True)      # no momenta set
        assert ei.value.code == STATE
        assert A.perf()["kernel_launches"] == launches and A.step_counter == 0
        A.step(1, scheme="heun")
        assert A.perf()["kernel_launches"] == launches + 2 and A.perf()["steps"] == 1
    with Phi4Lattice((16, 4, 4), dtau=0.05, comm="loopback", nslabs=2) as S:
        launches = S.perf()["kernel_launches"]
        assert sqlib.sq_phi4_step_heun(S._h, 1) == STATE and sqlib.sq_phi4_step_heun_meas(S._h, 1, 1, None, 0) == STATE
        assert S.perf()["kernel_launches"] == launches and S.step_counter == 0
    with Qm1dChain(16, 0.1, 0.002) as Q:
        assert sqlib.sq_phi4_step_heun(Q._h, 1) == STATE
