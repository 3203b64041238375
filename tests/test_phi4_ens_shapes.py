"""Every work-group shape of the phi^4 ensemble kernels, without a GPU.

sq_phi4_ens_shape_info (Phi4Ensemble.shape_info) reports, from the function
the launchers call, how a lattice is dealt to its work-group: K float4 quads
per lane, T lanes, and per launch the LDS images and dynamic LDS bytes.  This
file calls it for every legal (Lx, Ly, Lz), checks the invariants the kernels
rely on, and asserts that the GPU suites' shape list (GPU_SHAPES, run by
test_gpu_phi4_ens.py, test_gpu_phi4_ens_frames.py and
test_gpu_phi4_ens_shapes.py) holds a lattice of every class that exists:

    class = (K, images of the step launch, images of the frames launch,
             K T == Q, the last j's boundary lies inside a wave,
             a whole wave has no quad at the last j)

with Q = sites / 4 the lattice's quads.  Lane t owns quads t + j T, j < K; the
quads of j = K - 1 exist for t < n_last = Q - (K - 1) T only, so K T - Q owned
quads do not exist: n_last % 64 != 0 puts the boundary inside a wave, and
T - n_last >= 64 leaves whole waves without one.  If a threshold of
phi4_ens_shape moves, the coverage test names the class no GPU test runs.
"""
import pytest

LDS_LIMIT = 160 * 1024
# sq_phi4_ens.h: per wave 4 doubles and one float for 16 waves; the frames launch adds three step records
# (u64 key, u32 max) and the start field's two maxima, padded to 8 bytes
SCRATCH = 16 * 4 * 8 + 16 * 4
FRAME_SCRATCH = SCRATCH + 3 * 8 + 3 * 4 + 2 * 4 + 4
MAX_SITES = 32768
LX = (8, 16, 32, 64)

# The shapes the ensemble's GPU tests run: (K, T, images of the step launch, images of the frames launch).
GPU_SHAPES = {
    (8, 2, 2): (1, 64, 2, 2),          # one wave, 56 of its lanes without a quad; y and z neighbours coincide
    (8, 8, 8): (1, 128, 2, 2),
    (16, 4, 31): (1, 512, 2, 2),       # partial last wave
    (32, 8, 13): (1, 832, 2, 2),
    (64, 16, 8): (2, 1024, 2, 2),
    (32, 32, 32): (8, 1024, 1, 1),
    (64, 16, 32): (8, 1024, 1, 1),
    (8, 17, 31): (2, 576, 2, 2),       # 98 missing quads: the last j ends mid-wave, one wave has none
    (16, 24, 24): (4, 576, 2, 2),      # exact fit
    (64, 3, 43): (4, 576, 2, 2),       # 240 missing quads: mid-wave and three empty waves
    (16, 32, 32): (4, 1024, 2, 2),     # the largest K = 4 lattice
    (32, 24, 24): (8, 576, 2, 2),      # K = 8 with two images
    (8, 50, 51): (8, 640, 2, 2),       # the largest two-image lattice, 20 missing quads
    (64, 11, 29): (8, 640, 1, 1),      # the first one-image lattice, 16 missing quads
    (32, 2, 321): (8, 704, 1, 1),      # Ly = 2, 496 missing quads
    (8, 2, 2048): (8, 1024, 1, 1),     # a plane of four quads
    (64, 256, 2): (8, 1024, 1, 1),     # Lz = 2 at full size
    # the classes the coverage test named beyond those: a boundary inside a wave and no empty wave (32 missing
    # quads), whole waves only (64 missing), at the K and image counts where the list had neither
    (8, 20, 28): (2, 576, 2, 2),       # 32 missing
    (8, 16, 34): (2, 576, 2, 2),       # 64 missing
    (32, 4, 71): (4, 576, 2, 2),       # 32 missing
    (16, 20, 28): (4, 576, 2, 2),      # 64 missing
    (32, 12, 47): (8, 576, 2, 2),      # 96 missing: mid-wave and one empty wave, two images
    (16, 16, 71): (8, 576, 2, 2),      # 64 missing, two images
    (64, 12, 29): (8, 704, 1, 1),      # 64 missing, one image
}


# The shapes at which the MALA and HMC samplers measure in flight (test_gpu_phi4_ens_sampler_edges.py), one or
# two of every class (K, images of the plain step launch, images of the step launch with the correlator): the
# measuring kernels are instances of their own, and their image count follows the correlator's layout.
SAMPLER_MEASURE_SHAPES = [(8, 8, 8), (8, 17, 31), (64, 16, 8), (16, 24, 24), (64, 3, 43), (32, 24, 24), (8, 50, 51),
                          (64, 11, 29)]
TWO_TO_ONE = (8, 50, 51)      # two images plain, one with the correlator's 8 Lz bytes


def shape_info(shape):
    from stochquant_amd import Phi4Ensemble
    return Phi4Ensemble.shape_info(shape)


def measure_class(shape, info=None):
    """(K, images of the plain step launch, images of the step launch with the correlator)."""
    from stochquant_amd import Phi4Ensemble
    i = shape_info(shape) if info is None else info
    return (i["K"], i["images"], Phi4Ensemble.corr_shape_info(shape)["images"])


def shape_class(shape, info=None):
    """The class of the module docstring, from what shape_info reports."""
    i = shape_info(shape) if info is None else info
    Q = shape[0] * shape[1] * shape[2] // 4
    K, T = i["K"], i["T"]
    n_last = Q - (K - 1) * T
    return (K, i["images"], i["frames_images"], K * T == Q, n_last % 64 != 0, T - n_last >= 64)


def assert_shape(shape):
    """A GPU test's gate: the library still gives `shape` the work-group shape the test was written for."""
    i = shape_info(shape)
    assert (i["K"], i["T"], i["images"], i["frames_images"]) == GPU_SHAPES[tuple(shape)], (shape, i)
    return i


def legal_shapes():
    for Lx in LX:
        for Ly in range(2, MAX_SITES // (2 * Lx) + 1):
            for Lz in range(2, MAX_SITES // (Lx * Ly) + 1):
                yield (Lx, Ly, Lz)


@pytest.fixture(scope="module")
def infos(sqlib):
    return {s: shape_info(s) for s in legal_shapes()}


def test_every_legal_shape(infos):
    assert len(infos) == 45843
    for (Lx, Ly, Lz), i in infos.items():
        tag = ((Lx, Ly, Lz), i)
        sites = Lx * Ly * Lz
        Q = sites // 4
        K, T = i["K"], i["T"]
        assert K in (1, 2, 4, 8), tag
        assert T % 64 == 0 and 64 <= T <= 1024, tag
        assert K * T >= Q and (K - 1) * T < Q, tag        # every j has a quad somewhere in the block
        assert T <= (Q + 63) // 64 * 64, tag
        assert T - 64 < Q, tag                            # every wave owns an existing quad at j = 0
        assert i["lds_limit"] == LDS_LIMIT, tag
        for images, nbytes, scratch in ((i["images"], i["lds_bytes"], SCRATCH),
                                        (i["frames_images"], i["frames_lds_bytes"], FRAME_SCRATCH)):
            assert images in (1, 2), tag
            assert nbytes == images * 4 * sites + scratch <= LDS_LIMIT, tag
            assert (images == 2) == (2 * 4 * sites + scratch <= LDS_LIMIT), tag   # two images exactly when they fit
        assert i["moments_lds_bytes"] == 4 * sites + SCRATCH <= LDS_LIMIT, tag


@pytest.mark.parametrize("shape", [(4, 8, 8), (12, 8, 8), (24, 8, 8), (128, 8, 8), (0, 8, 8), (-8, 8, 8), (8, 1, 8),
                                   (8, 8, 1), (8, 0, 8), (8, 8, -2), (8, 17, 241), (8, 2, 2049), (8, 2049, 2), (16, 2, 1025),
                                   (32, 32, 33), (64, 2, 257), (8, 4097, 1), (8, 65536, 65536), (64, 32768, 32768)])
def test_shapes_just_outside_are_refused(sqlib, shape):
    import ctypes
    from stochquant_amd import StochQuantError
    with pytest.raises(StochQuantError) as ei:
        shape_info(shape)
    assert ei.value.code == -1 and str(ei.value) != ""
    out = (ctypes.c_int * 8)()
    assert sqlib.sq_phi4_ens_shape_info(None, out) == -1
    assert sqlib.sq_phi4_ens_shape_info((ctypes.c_int * 3)(8, 8, 8), None) == -1


def test_refusals_are_those_of_create(sqlib):
    """The query and sq_phi4_ens_create draw the same line: create answers SQ_E_ARG
    exactly where the query does (elsewhere it goes on to look for a device)."""
    from test_phi4_ens_boundary import _create
    for shape in [(8, 2, 2), (8, 2, 2048), (64, 256, 2), (16, 2, 1024), (8, 2, 2049), (16, 2, 1025), (8, 1, 8),
                  (8, 8, 1), (12, 8, 8), (128, 2, 2), (32, 32, 33)]:
        try:
            shape_info(shape)
            refused = False
        except Exception:
            refused = True
        rc, _ = _create(sqlib, shape=shape)
        assert (rc == -1) == refused, (shape, rc)


def test_gpu_shape_list_covers_every_class(infos):
    have = {}
    for s, want in GPU_SHAPES.items():
        i = infos[s]
        assert (i["K"], i["T"], i["images"], i["frames_images"]) == want, (s, i)
        have.setdefault(shape_class(s, i), s)
    missing = {}
    for s, i in infos.items():
        c = shape_class(s, i)
        if c not in have:
            missing.setdefault(c, s)
    names = ("K", "images", "frames images", "K T == Q", "boundary inside a wave", "a wave without a last-j quad")
    assert not missing, "no GPU test runs: " + "; ".join(
        ", ".join(f"{n} = {v}" for n, v in zip(names, c)) + f" (e.g. {s[0]} x {s[1]} x {s[2]})"
        for c, s in sorted(missing.items()))
    assert {s[0] for s in GPU_SHAPES} == set(LX)


def test_sampler_measure_list_covers_every_class(infos):
    """The samplers' measuring instances: every (K, plain images, correlator images) that a legal shape has is in
    SAMPLER_MEASURE_SHAPES, the correlator never adds an image, and TWO_TO_ONE is the class it takes one from."""
    classes = {}
    for s, i in infos.items():
        classes.setdefault(measure_class(s, i), s)
    assert set(classes) == {(1, 2, 2), (2, 2, 2), (4, 2, 2), (8, 2, 2), (8, 2, 1), (8, 1, 1)}, classes
    have = {measure_class(s, infos[s]) for s in SAMPLER_MEASURE_SHAPES}
    assert have == set(classes), {c: s for c, s in classes.items() if c not in have}
    assert measure_class(TWO_TO_ONE, infos[TWO_TO_ONE]) == (8, 2, 1) and TWO_TO_ONE in SAMPLER_MEASURE_SHAPES
    assert all(s in GPU_SHAPES for s in SAMPLER_MEASURE_SHAPES)
    # missing quads (K T > Q) at K = 2, 4 and in all three K = 8 classes
    missing = {measure_class(s, infos[s]) for s in SAMPLER_MEASURE_SHAPES
               if infos[s]["K"] * infos[s]["T"] > s[0] * s[1] * s[2] // 4}
    assert missing == {(2, 2, 2), (4, 2, 2), (8, 2, 1), (8, 1, 1)}, missing


# ---- the one LDS rule (sq_phi4_ens.h, phi4_ens_lds), stated here and held against every number that every
# *_shape_info entry point returns, for every legal shape.  A launch's dynamic LDS is the image(s) of the lattice
# (4 bytes a site), the launch's scratch, then the bytes its measurement keeps behind the scratch; two images
# exactly when 2 * 4 * sites + scratch + behind fits in 160 KiB, and always one for a launch that works on the
# stored field.

def lds_rule(sites, kind, behind):
    """(images, bytes) of a launch of `kind`: "step", "frames" or "stored"."""
    rest = (FRAME_SCRATCH if kind == "frames" else SCRATCH) + behind
    images = 2 if kind != "stored" and 2 * 4 * sites + rest <= LDS_LIMIT else 1
    return images, images * 4 * sites + rest


def none(Lz):
    return 0


def corr(Lz):  # the slice sums: Lz doubles
    return 8 * Lz


def pcorr(Lz):  # the projections: 2 Lz doubles
    return 16 * Lz


def sums(Lz):  # the cluster sums' per-weight totals
    return 32


def momenta_fit(sites, Lz):
    """One image fits in each of the three launches that take momenta."""
    return all(4 * sites + scratch + pcorr(Lz) <= LDS_LIMIT for scratch in (SCRATCH, FRAME_SCRATCH, SCRATCH))


# (entry point; index into its out[], or (index, shift) of a byte packed into it; launch kind; bytes behind the
# scratch; which of the rule's two numbers)
LDS_TABLE = [
    ("sq_phi4_ens_shape_info", 2, "step", none, "images"),
    ("sq_phi4_ens_shape_info", 3, "step", none, "bytes"),
    ("sq_phi4_ens_shape_info", 4, "frames", none, "images"),
    ("sq_phi4_ens_shape_info", 5, "frames", none, "bytes"),
    ("sq_phi4_ens_shape_info", 6, "stored", none, "bytes"),                  # moments
    ("sq_phi4_ens_corr_shape_info", 0, "step", corr, "images"),
    ("sq_phi4_ens_corr_shape_info", 1, "step", corr, "bytes"),
    ("sq_phi4_ens_corr_shape_info", 2, "frames", corr, "images"),
    ("sq_phi4_ens_corr_shape_info", 3, "frames", corr, "bytes"),
    ("sq_phi4_ens_corr_shape_info", 4, "stored", corr, "bytes"),             # slices
    ("sq_phi4_ens_pcorr_shape_info", 0, "step", pcorr, "images"),
    ("sq_phi4_ens_pcorr_shape_info", 1, "step", pcorr, "bytes"),
    ("sq_phi4_ens_pcorr_shape_info", 2, "frames", pcorr, "images"),
    ("sq_phi4_ens_pcorr_shape_info", 3, "frames", pcorr, "bytes"),
    ("sq_phi4_ens_pcorr_shape_info", 4, "stored", pcorr, "bytes"),           # pslices
    ("sq_phi4_ens_flow_shape_info", 0, "step", none, "images"),
    ("sq_phi4_ens_flow_shape_info", 1, "step", none, "bytes"),
    ("sq_phi4_ens_flow_shape_info", 2, "step", corr, "images"),
    ("sq_phi4_ens_flow_shape_info", 3, "step", corr, "bytes"),
    ("sq_phi4_ens_flow_shape_info", 4, "step", corr, "bytes"),               # flowed: it ping-pongs as a step launch
    ("sq_phi4_ens_frames_flow_shape_info", 0, "frames", none, "images"),
    ("sq_phi4_ens_frames_flow_shape_info", 1, "frames", none, "bytes"),
    ("sq_phi4_ens_frames_flow_shape_info", 2, "frames", corr, "images"),
    ("sq_phi4_ens_frames_flow_shape_info", 3, "frames", corr, "bytes"),
    ("sq_phi4_ens_frames_flow_shape_info", (4, 0), "step", none, "images"),  # the Heun step launch
    ("sq_phi4_ens_frames_flow_shape_info", (4, 8), "step", corr, "images"),
    ("sq_phi4_ens_frames_flow_shape_info", 5, "step", corr, "bytes"),
    ("sq_phi4_ens_heun_frames_shape_info", 0, "frames", none, "images"),
    ("sq_phi4_ens_heun_frames_shape_info", 1, "frames", none, "bytes"),
    ("sq_phi4_ens_exchange_shape_info", 2, "stored", none, "bytes"),
    ("sq_phi4_ens_cluster_shape_info", 2, "stored", none, "bytes"),
    ("sq_phi4_ensemble_cluster_improved_shape_info", 2, "stored", sums, "bytes"),
]
LDS_CALLS = sorted({row[0] for row in LDS_TABLE})


def test_the_lds_table_names_every_shape_info_entry_point():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "stochquant.h")) as fh:
        declared = set(re.findall(r"\bint\s+(sq_phi4_ens\w*shape_info)\s*\(", fh.read()))
    assert declared == set(LDS_CALLS)


def test_the_legal_shapes_lie_on_both_sides_of_every_threshold_of_the_rule():
    seen, fits = {}, set()
    for Lx, Ly, Lz in legal_shapes():
        sites = Lx * Ly * Lz
        fits.add(momenta_fit(sites, Lz))
        for _, _, kind, behind, _ in LDS_TABLE:
            seen.setdefault((kind, behind.__name__), set()).add(lds_rule(sites, kind, behind(Lz))[0])
    for (kind, _), images in seen.items():
        assert images == ({1} if kind == "stored" else {1, 2})
    assert fits == {True, False}


def test_every_shape_info_number_follows_the_one_rule(sqlib):
    import ctypes
    dims = (ctypes.c_int * 3)()
    out = (ctypes.c_int * 8)()
    fns = {name: getattr(sqlib, name) for name in LDS_CALLS}
    rows = {name: [r for r in LDS_TABLE if r[0] == name] for name in LDS_CALLS}
    nshapes = 0
    for Lx, Ly, Lz in legal_shapes():
        sites = Lx * Ly * Lz
        dims[0], dims[1], dims[2] = Lx, Ly, Lz
        nshapes += 1
        fit = momenta_fit(sites, Lz)
        for name in LDS_CALLS:
            rc = fns[name](dims, out)
            if name == "sq_phi4_ens_pcorr_shape_info" and not fit:
                assert rc == -1, (name, Lx, Ly, Lz)  # SQ_E_ARG: the shape cannot hold momenta
                continue
            assert rc == 0, (name, Lx, Ly, Lz)
            for _, idx, kind, behind, which in rows[name]:
                images, nbytes = lds_rule(sites, kind, behind(Lz))
                got = out[idx] if isinstance(idx, int) else (out[idx[0]] >> idx[1]) & 0xff
                assert got == (images if which == "images" else nbytes), (name, idx, Lx, Ly, Lz)
                assert nbytes <= LDS_LIMIT, (name, idx, Lx, Ly, Lz)
            if name == "sq_phi4_ens_heun_frames_shape_info":
                assert out[2] == (0xf if fit else 0x3), (Lx, Ly, Lz)  # momenta only where they fit
    assert nshapes == 45843
