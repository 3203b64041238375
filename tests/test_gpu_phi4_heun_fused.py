"""The one-launch Heun step of the single phi^4 lattice on the GPU (sq_phi4_heun_fused.hip,
sq_phi4_step_heun_fused, Phi4Lattice.step(scheme="heun", fused=True)) against the CPU oracle's Heun entry and
against the two-launch step, its in-stream measurements against stand-alone ones, and its refusals.

Tolerances: none.  Fields, counters, series rows and accumulators are compared bit for bit.
"""
import numpy as np
import pytest

from test_gpu_phi4_ens_heun import CLAMP, LAM, M2
from test_gpu_phi4_ens_mala import CS
from test_gpu_phi4_hmc import _lat, _start
from test_gpu_phi4_measure import _bits
from test_oracle import HEUN_GUARD_CASES, assert_heun_guard_maxima, heun_guard_field, same_bits

pytestmark = pytest.mark.gpu

DTAU, SEED = 0.004, 11
# (shape, SQ_FUSE2_Z or None, C, first counter)
ORACLE_CASES = [
    ((256, 8, 2), None, CS[0], 0),             # both z-neighbours the same plane; one y-band, its own neighbour
    ((256, 16, 7), "1", CS[0], 0),             # chunks of every length mod 3, a ragged last chunk, both wraps
    ((256, 16, 7), "2", CS[0], 0),
    ((256, 16, 7), "3", CS[0], 0),
    ((512, 8, 3), None, CS[0], 0),             # two x-segments: the x-halo wave
    ((768, 16, 4), "3", CS[0], 0),             # three x-segments, two y-bands, a ragged last chunk
    ((256, 8, 5), None, 0.0, 0),               # the instance without noise
    ((256, 8, 4), None, CS[0], 2 ** 32 - 2),   # the counter crosses into the high word
]


@pytest.mark.parametrize("shape,zc,C,s0", ORACLE_CASES)
def test_bitwise_against_the_oracle_and_the_two_launch_step(gpu, dev_oracle, monkeypatch, shape, zc, C, s0):
    if zc is not None:
        monkeypatch.setenv("SQ_FUSE2_Z", zc)   # read when the context is created
    p = dev_oracle.phi4_params(shape, DTAU, M2[0], LAM[0], SEED, clamp=CLAMP, C=C)
    phi0 = dev_oracle.phi4_init(p, 0.5)
    with _lat(shape, DTAU, SEED, C=C) as A, _lat(shape, DTAU, SEED, C=C) as B:
        for X in (A, B):
            X.upload(phi0)
            X.step_counter = s0
        assert A.step(3, scheme="heun", fused=True) is None
        A.step(2, scheme="heun", fused=True)
        B.step(5, scheme="heun")
        got, twin = A.download(), B.download()
        assert A.step_counter == B.step_counter == s0 + 5
    ref = phi0
    for k in range(5):
        ref, _ = dev_oracle.phi4_heun_step(p, ref, s0 + k)
    assert same_bits(got, ref), f"{np.count_nonzero(got != ref)} sites differ, max {np.max(np.abs(got - ref))}"
    assert same_bits(twin, ref)


@pytest.mark.parametrize("case", HEUN_GUARD_CASES, ids=[c[0] for c in HEUN_GUARD_CASES])
def test_guard_stage_by_stage(gpu, oracle_mod, case):
    """One fused step of test_oracle.HEUN_GUARD_CASES (C = 0, clamp 1000) on (256, 8, 3): no maximum at the clamp,
    max |e| alone, max |p| and max |e|, max |p| alone; then the same field with a NaN and an infinity uploaded."""
    from stochquant_amd import Phi4Lattice
    shape = (256, 8, 3)
    dt, m2, lam = case[3]
    p = oracle_mod.phi4_params(shape, dt, m2, lam, 1, clamp=CLAMP, C=0.0)
    phi0 = heun_guard_field(case, shape)
    bad = phi0.copy()
    bad[1, 3, 7], bad[2, 0, 255] = np.nan, np.inf
    with Phi4Lattice(shape, dtau=dt, m2=m2, lam=lam, C=0.0, seed=1, clamp=CLAMP) as A:
        for start in (phi0, bad):
            A.upload(start)
            A.step_counter = 0
            A.step(1, scheme="heun", fused=True)
            ref, maxima = oracle_mod.phi4_heun_step(p, start, 0)
            if start is phi0:
                assert_heun_guard_maxima(case, maxima)
            assert same_bits(A.download(), ref), case[0]


def test_in_stream_is_stand_alone(gpu):
    shape = (256, 8, 4)
    with _lat(shape, DTAU, SEED) as A, _lat(shape, DTAU, SEED) as B:
        for X in (A, B):
            X.upload(_start(shape, SEED))
        series = A.step(4, scheme="heun", every=2, correlate=True, fused=True)
        meas = []
        for _ in range(2):
            B.step(2, scheme="heun", fused=True)
            meas.append(B.measure(slices=True))
        assert series.shape == (2, 4)
        assert np.array_equal(_bits(series), _bits(np.stack([m["sums"] for m in meas])))
        assert same_bits(A.download(), B.download()) and A.step_counter == B.step_counter == 4
        acc = A.corr_sums()
        assert np.array_equal(_bits(acc["G"]), _bits(meas[0]["g"] + meas[1]["g"]))
        assert _bits(acc["S1"]) == _bits(0.0 + meas[0]["sums"][0] + meas[1]["sums"][0]) and acc["nmeas"] == 2


@pytest.mark.parametrize("shape,kw", [((16, 4, 2), {}), ((256, 4, 6), {}),
                                      ((256, 8, 4), {"comm": "loopback", "nslabs": 2})])
def test_refusals_launch_nothing(gpu, sqlib, shape, kw):
    from stochquant_amd import StochQuantError
    with _lat(shape, 0.005, SEED, **kw) as A:
        launches = A.perf()["kernel_launches"]
        with pytest.raises(StochQuantError) as ei:
            A.step(1, scheme="heun", fused=True)
        assert ei.value.code == -4
        assert sqlib.sq_phi4_step_heun_fused_meas(A._h, 1, 1, None, 0) == -4
        assert sqlib.sq_phi4_step_heun_fused(A._h, -1) == -1
        assert A.perf()["kernel_launches"] == launches and A.step_counter == 0


def test_one_step_is_one_launch(gpu, sqlib):
    with _lat((256, 8, 4), DTAU, SEED) as A:
        launches = A.perf()["kernel_launches"]
        assert sqlib.sq_phi4_step_heun_fused(A._h, -1) == -1 and sqlib.sq_phi4_step_heun_fused(A._h, 0) == 0
        assert A.perf()["kernel_launches"] == launches and A.step_counter == 0
        A.step(1, scheme="heun", fused=True)
        assert A.perf()["kernel_launches"] == launches + 1 and A.perf()["steps"] == 1 and A.step_counter == 1
