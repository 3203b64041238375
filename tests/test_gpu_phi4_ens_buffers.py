"""The buffers of the phi^4 ensemble's handle on the GPU.  Every buffer that grows or is created at its first use is
a sq::Buf (csrc/sq_buf.h) the handle owns.  Handle A makes each call that owns such a buffer twice, the second time
larger, so that the buffer is reallocated between the two; handle B, built from the same seeds and fields, makes the
first call without records (or, where the call only measures, not at all) and then the larger call.  Everything the
larger call returns, and the fields, counters and flags after it, are bit for bit equal between A and B: a pointer
taken before a reserve, or a stale capacity, shows as a difference or a fault.  Both handles are then destroyed, and
so is one that was never used.  All comparisons are exact."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPE, R = (8, 2, 2), 4
SEEDS = [0xB0F + 17 * r for r in range(R)]
EPS = 0.01


def _ens():
    from stochquant_amd import Phi4Ensemble
    return Phi4Ensemble(SHAPE, R, dtau=0.01, m2=0.5, lam=1.0, C=1.0, seeds=SEEDS, loops=2)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _state(E):
    p = E.get_params()
    return [E.download(), E.step_counter, E.flags(), p["dtau"], E.walkers(), np.asarray(E.exchange_round),
            np.asarray(E.cluster_sweep), E.mala_stats(), E.hmc_stats(), E.exchange_stats(), E.cluster_stats(),
            np.asarray(E.perf()["steps"])]


def _same(what, a, b):
    a = a if isinstance(a, (tuple, list)) else (a,)
    b = b if isinstance(b, (tuple, list)) else (b,)
    assert len(a) == len(b), what
    for i, (x, y) in enumerate(zip(a, b)):
        if x is None or y is None:
            assert x is None and y is None, (what, i)
            continue
        x, y = _bits(x), _bits(y)
        assert x.shape == y.shape and x.dtype == y.dtype, (what, i, x.shape, y.shape)
        assert np.array_equal(x, y), (what, i)


def test_a_reallocated_buffer_serves_the_larger_call_as_a_fresh_one_does():
    A, B = _ens(), _ens()
    try:
        for E in (A, B):
            E.init_field(0.5)
            E.step(20)
        start = A.download()
        B.upload(start)
        _same("start", _state(A), _state(B))

        def both(what, small_a, small_b, large):
            """small_a on A, small_b (None: nothing) on B, then `large` on both: its results and the states agree."""
            small_a(A)
            if small_b is not None:
                small_b(B)
            ra, rb = large(A), large(B)
            _same(what, ra, rb)
            _same(what + ": state", _state(A), _state(B))
            return ra

        # the pinned series buffer
        ser = both("step", lambda E: E.step(4, every=2), lambda E: E.step(4), lambda E: E.step(8, every=1))
        assert ser.shape == (8, R, 4) and np.all(ser[:, :, 1] > 0)
        # the frames' verdict buffers, the frame records (first use) and the series again
        fr = both("run_frames", lambda E: E.run_frames(1, measure=True), lambda E: E.run_frames(1),
                  lambda E: E.run_frames(3, measure=True))
        assert fr[2].shape == (3, R, 4)
        _same("stability", list(A.stability().values()), list(B.stability().values()))
        # the slices' device buffer
        both("slices", lambda E: E.slices(count=1), None, lambda E: E.slices())
        # the twiddle tables (first use), the momentum accumulators and the pslices' device buffer
        both("pslices", lambda E: (E.set_momenta([(1, 0)]), E.pslices(count=1)), lambda E: E.set_momenta([(1, 0)]),
             lambda E: (E.set_momenta([(1, 0), (0, 1), (1, 1)]), E.pslices())[1])
        # the flow records (first use), the flow accumulators (three temporaries swapped in), the flow's device
        # buffer and the series with F rows per record
        def flow_calls(E, levels):
            E.set_flow(EPS, levels)
            return E.flowed() + (E.flow_field(2), E.step_flow(4, 2))
        fl = both("flow", lambda E: flow_calls(E, (1,)), lambda E: (E.set_flow(EPS, (1,)), E.step(4)),
                  lambda E: flow_calls(E, (0, 1, 2)))
        assert fl[0].shape == (R, 3, 4) and fl[4].shape == (2, 3, R, 4)
        _same("fcorr_sums", A.fcorr_sums(), B.fcorr_sums())
        # the MALA counters (first use) and records
        ml = both("step_mala", lambda E: E.step_mala(2, record=True), lambda E: E.step_mala(2),
                  lambda E: E.step_mala(6, record=True))
        assert ml[0] is None and ml[1].shape == (6, R, 3)
        # the HMC counters (first use) and records
        hm = both("step_hmc", lambda E: E.step_hmc(1, 2, record=True), lambda E: E.step_hmc(1, 2),
                  lambda E: E.step_hmc(4, 2, record=True))
        assert hm[1].shape == (4, R, 4)
        # the exchange records
        for E in (A, B):
            E.set_ladder(2)
        xr = both("exchange", lambda E: E.exchange(1, record=True), lambda E: E.exchange(1),
                  lambda E: E.exchange(4, record=True))
        assert xr.shape == (4, R, 5)
        # the cluster sweeps' bond and label records
        cl = both("cluster", lambda E: E.cluster(1, record=True), lambda E: E.cluster(1),
                  lambda E: E.cluster(3, record=True))
        assert cl[0].shape == cl[1].shape == (3, R, 32)
        # the fused calls: series, trajectory records and the second sampler's records, all at once
        fx = both("step_hmc_exchange", lambda E: E.step_hmc_exchange(1, 2, 2, every=1, record=True),
                  lambda E: E.step_hmc_exchange(1, 2, 2),
                  lambda E: E.step_hmc_exchange(3, 2, 2, every=1, record=True))
        assert [a.shape for a in fx] == [(6, R, 4), (6, R, 4), (3, R, 5)]
        fc = both("step_hmc_cluster", lambda E: E.step_hmc_cluster(1, 2, 2, every=1, record=True),
                  lambda E: E.step_hmc_cluster(1, 2, 2),
                  lambda E: E.step_hmc_cluster(3, 2, 2, every=1, record=True))
        assert [a.shape for a in fc] == [(6, R, 4), (6, R, 4), (3, R, 32), (3, R, 32)]
        assert not np.array_equal(A.download(), start)      # the calls did move the fields
        # 20 to thermalise, 4 + 8 steps, (1 + 3) frames of 2, 4 + 4 flow steps, 2 + 6 MALA steps, 1 + 4 trajectories,
        # and (1 + 3) rounds of 2 trajectories in either fused call
        assert int(A.step_counter[0]) == 20 + 12 + 8 + 8 + 8 + 5 + 8 + 8
    finally:
        A.close()
        B.close()
    from stochquant_amd import Phi4Ensemble
    Phi4Ensemble(SHAPE, R, loops=2).close()                 # a handle never used: its lazy buffers are all empty
