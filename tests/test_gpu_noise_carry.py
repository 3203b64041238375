"""The fused kernels take the step-only Philox words from the host
(Phi4StepArgs::nw0 / nw1) and start step s+1's noise from the prefix step s
left at the same sites one plane iteration earlier (sq_phi4.hip, NoisePre).
Every path that does so must give the field of one step per launch
(SQ_FUSE2=0) bit for bit, noise on: every exit of the march's unroll with the
periodic z-wrap inside the chunk, halo rows from another block, wide rows in
both fused kernels, the neighbour-sync kernel, a slab decomposition, a frame,
and the pairs around step 2^32, where the two steps of a pair differ in
step_hi and the carried prefix is re-keyed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_FUSE_ENV = ("SQ_FUSE2", "SQ_FUSE2_Z", "SQ_TB2_PIPE", "SQ_TB2_SYNC", "SQ_GHOST")


def _lat(shape, **kw):
    from stochquant_amd import Phi4Lattice
    return Phi4Lattice(shape, dtau=0.02, m2=0.5, lam=1.0, seed=4242, C=1.0, **kw)


def _phi0(shape):
    rng = np.random.default_rng(shape[0] + 7 * shape[1] + 31 * shape[2])
    return (0.9 * rng.standard_normal((shape[2], shape[1], shape[0]))).astype(np.float32)


_refs = {}


def _ref(monkeypatch, shape, steps=6, step0=0):
    """One step per launch from _phi0(shape), computed once per (shape, steps, step0)."""
    key = (shape, steps, step0)
    if key not in _refs:
        for k in _FUSE_ENV:
            monkeypatch.delenv(k, raising=False)
        monkeypatch.setenv("SQ_FUSE2", "0")
        with _lat(shape) as L:
            assert "tb2" not in L.kernel_name, L.kernel_name
            L.upload(_phi0(shape))
            L.step_counter = step0
            L.step(steps)
            ref = L.download()
        ref.setflags(write=False)
        _refs[key] = ref
    return _refs[key]


def _fused(monkeypatch, shape, steps=6, step0=0, env=(), kernel="tb2", **kw):
    ref = _ref(monkeypatch, shape, steps, step0)
    monkeypatch.setenv("SQ_FUSE2", "1")
    for k, v in env:
        monkeypatch.setenv(k, v)
    with _lat(shape, **kw) as L:
        L.upload(_phi0(shape))
        L.step_counter = step0
        L.step(steps)
        got = L.download()
        assert L.step_counter == step0 + steps
        if kernel:
            assert kernel in L.launch_info()["kernel"], L.launch_info()  # the kernel launched most often
        assert L.perf()["fused_steps"] > 0
    assert np.array_equal(got, ref), f"{np.count_nonzero(got != ref)} sites differ"


@pytest.mark.parametrize("nz", [4, 5, 6])
def test_carry_at_every_unroll_exit(gpu, monkeypatch, nz):
    """One y-band, the whole lattice one chunk: nz + 2 plane iterations, so the
    three-way unrolled march ends at each of its three positions, and the
    periodic z-wrap of the quad base falls inside the chunk at both ends."""
    _fused(monkeypatch, (256, 8, nz), env=[("SQ_FUSE2_Z", str(nz))])


def test_carry_two_y_bands(gpu, monkeypatch):
    """The halo rows of step s come from another block's band."""
    _fused(monkeypatch, (256, 16, 7))


@pytest.mark.parametrize("pipe", ["0", "1"])
def test_carry_wide_rows(gpu, monkeypatch, pipe):
    """512-site rows: the x-halo wave (no carry), in the pipelined kernel (which carries) and the other."""
    _fused(monkeypatch, (512, 8, 5), env=[("SQ_TB2_PIPE", pipe)], kernel="tb2p" if pipe == "1" else "tb2_kernel")


def test_carry_neighbour_sync(gpu, monkeypatch):
    _fused(monkeypatch, (256, 8, 6), env=[("SQ_TB2_PIPE", "0"), ("SQ_TB2_SYNC", "p2p")])


def test_carry_loopback_slabs(gpu, monkeypatch):
    """Deep-halo blocks of two slabs (4 ghost planes: blocks of fewer than 3
    steps do not fuse): launches on ranges with ghost zones, the quad base of
    ghost planes wrapped."""
    _fused(monkeypatch, (256, 8, 24), env=[("SQ_FUSE2_Z", "3"), ("SQ_GHOST", "4")], kernel=None, comm="loopback",
           nslabs=2)  # (most launches there are the rims' single steps)


@pytest.mark.parametrize("step0", [0xFFFFFFFD, 0xFFFFFFFE, 0xFFFFFFFF])
def test_pairs_around_step_2_pow_32(gpu, monkeypatch, step0):
    """4 steps from step0: a pair ends on the boundary, straddles it (steps
    0xFFFFFFFF and 2^32 in one launch: step_hi differs inside the pair) and
    begins after it."""
    _fused(monkeypatch, (256, 8, 4), steps=4, step0=step0, env=[("SQ_FUSE2_Z", "4")])


def test_frame_equals_raw_steps(gpu, monkeypatch):
    """Two raw steps and a frame of 4 (sq_run_frames, the frame instances of the fused kernels) == 6 raw steps."""
    shape = (256, 8, 6)
    ref = _ref(monkeypatch, shape)
    monkeypatch.setenv("SQ_FUSE2", "1")
    with _lat(shape, loops=4) as L:
        L.upload(_phi0(shape))
        L.step(2)
        st, _ = L.run_frames(1)
        assert st[0]
        got = L.download()
        assert L.step_counter == 6
    assert np.array_equal(got, ref), f"{np.count_nonzero(got != ref)} sites differ"
