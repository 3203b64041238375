"""The momentum-projected correlator's boundary without a GPU: libstochquant.so
exports the sq_phi4_ens_*momenta / *pcorr* / _pslices / _momentum_table symbols
and _lib.SIGNATURES binds them, the ABI version stays 6, the twiddle tables
(sq_phi4_ens_momentum_table, host only) are what include/stochquant.h states,
and the momentum launches' LDS requests (sq_phi4_ens_pcorr_shape_info, host
only) follow the stated rule over every legal ensemble shape."""
import ctypes

import numpy as np
import pytest

PCORR_SYMBOLS = ["sq_phi4_ens_momentum_table", "sq_phi4_ens_set_momenta", "sq_phi4_ens_get_momenta",
                 "sq_phi4_ens_step_pcorr", "sq_phi4_ens_run_frames_pcorr", "sq_phi4_ens_pcorr_sums",
                 "sq_phi4_ens_pcorr_reset", "sq_phi4_ens_pslices", "sq_phi4_ens_pcorrelator",
                 "sq_phi4_ens_pcorr_shape_info"]
SCRATCH, FRAME_SCRATCH, LIMIT = 576, 624, 160 * 1024


def test_library_exports_the_momentum_symbols(sqlib):
    from stochquant_amd import _lib
    assert [s for s in PCORR_SYMBOLS if not hasattr(sqlib, s)] == []
    assert [s for s in PCORR_SYMBOLS if s not in _lib.SIGNATURES] == []
    assert sqlib.sq_abi_version() == _lib.ABI_VERSION == 6
    assert _lib.SQ_PHI4_ENS_MAX_MOMENTA == 8


def test_null_handle_is_an_argument_error(sqlib):
    d = (ctypes.c_double * 4)()
    i = (ctypes.c_int * 4)()
    n = (ctypes.c_longlong * 4)()
    assert sqlib.sq_phi4_ens_set_momenta(None, 1, i) == -1
    assert sqlib.sq_phi4_ens_get_momenta(None, i, i) == -1
    assert sqlib.sq_phi4_ens_step_pcorr(None, 4, 2, None, 0) == -1
    assert sqlib.sq_phi4_ens_run_frames_pcorr(None, 1, i, d, None, 0) == -1
    assert sqlib.sq_phi4_ens_pcorr_sums(None, 0, 1, d, n) == -1
    assert sqlib.sq_phi4_ens_pcorr_reset(None, 0, 1) == -1
    assert sqlib.sq_phi4_ens_pslices(None, 0, 1, d, d) == -1
    assert sqlib.sq_phi4_ens_pcorrelator(None, d, d, 1, i) == -1
    assert sqlib.sq_phi4_ens_pcorr_shape_info(None, i) == -1


def test_momenta_need_every_before_any_device_call(sqlib):
    from stochquant_amd import Phi4Ensemble
    E = Phi4Ensemble.__new__(Phi4Ensemble)      # no handle: a library call would fail differently
    E._h = ctypes.c_void_p()
    E.R = 2
    for every in (0, -1):
        with pytest.raises(ValueError):
            E.step(4, every=every, momenta=True)


def _quarter(L, j):
    """(c, s) exactly where 4 j is a multiple of L, else None."""
    if (4 * j) % L:
        return None
    return [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)][4 * j // L]


@pytest.mark.parametrize("L", [2, 3, 4, 5, 8, 12, 16, 31, 32, 50, 64, 2000])
def test_momentum_table_values(sqlib, L):
    from stochquant_amd import Phi4Ensemble
    for n in sorted({0, 1, 2, L // 4, L // 2, L - 1} & set(range(L))):
        c, s = Phi4Ensemble.momentum_table(L, n)
        assert c.shape == s.shape == (L,)
        for k in range(L):
            j = (n * k) % L
            q = _quarter(L, j)
            if q is not None:
                # exact, signs of the zeros included
                assert (c[k], s[k]) == q and not np.signbit(c[k] if q[0] == 0.0 else s[k]), (L, n, k)
                continue
            a = 2.0 * np.pi * float(j) / float(L)
            rc, rs = np.cos(a), np.sin(a)
            assert abs(c[k] - rc) <= np.spacing(abs(rc)) and abs(s[k] - rs) <= np.spacing(abs(rs)), (L, n, k)


def test_momentum_table_index_rule(sqlib):
    """j = (n k) mod L: (L, n) = (8, 3) against the angles written out."""
    from stochquant_amd import Phi4Ensemble
    c, s = Phi4Ensemble.momentum_table(8, 3)
    js = [0, 3, 6, 1, 4, 7, 2, 5]
    assert js == [(3 * k) % 8 for k in range(8)]
    h = np.sqrt(0.5)
    want = {0: (1.0, 0.0), 1: (h, h), 2: (0.0, 1.0), 3: (-h, h), 4: (-1.0, 0.0), 5: (-h, -h), 6: (0.0, -1.0),
            7: (h, -h)}
    for k, j in enumerate(js):
        wc, ws = want[j]
        assert abs(c[k] - wc) <= 2.0 ** -52 and abs(s[k] - ws) <= 2.0 ** -52, (k, j, c[k], s[k])
        if j % 2 == 0:
            assert (c[k], s[k]) == (wc, ws)
    # the table of n is the table of 1 read at stride n
    c1, s1 = Phi4Ensemble.momentum_table(8, 1)
    assert np.array_equal(c, c1[js]) and np.array_equal(s, s1[js])


def test_momentum_table_argument_errors(sqlib):
    d = (ctypes.c_double * 8)()
    assert sqlib.sq_phi4_ens_momentum_table(1, 0, d, d) == -1
    assert sqlib.sq_phi4_ens_momentum_table(0, 0, d, d) == -1
    assert sqlib.sq_phi4_ens_momentum_table(8, -1, d, d) == -1
    assert sqlib.sq_phi4_ens_momentum_table(8, 8, d, d) == -1
    assert sqlib.sq_phi4_ens_momentum_table(8, 1, None, d) == -1
    assert sqlib.sq_phi4_ens_momentum_table(8, 1, d, None) == -1
    assert sqlib.sq_last_error().decode() != ""
    assert sqlib.sq_phi4_ens_momentum_table(8, 7, d, d) == 0


def _legal_shapes():
    """Every Lx, with Ly and Lz at both ends and at each side of every site-count threshold of the shape rule,
    and the longest columns, where the momentum rule refuses."""
    out = set()
    for Lx in (8, 16, 32, 64):
        for Ly in (2, 3, 8, 16, 32, 50):
            top = 32768 // (Lx * Ly)
            if top < 2:
                continue
            cands = {2, 3, top, top - 1, max(2, top // 2), max(2, top // 2 + 1)}
            for sites in (4096, 8192, 16384, 20408, 20336, 20200, 19800):   # K thresholds, the two-image limits
                z = sites // (Lx * Ly)
                cands |= {z - 1, z, z + 1}
            out |= {(Lx, Ly, z) for z in cands if 2 <= z <= top}
    # 80 Lz + 624 <= 163,840 up to Lz = 2040; two images with Lz doubles but not with 2 Lz for 1134 <= Lz <= 1200
    out |= {(8, 2, z) for z in (1133, 1134, 1150, 1200, 1201, 2000, 2039, 2040, 2041, 2047, 2048)}
    out |= {(8, 3, 1365), (8, 3, 1360), (16, 2, 1024)}
    return sorted(out)


def test_pcorr_shape_info_over_legal_shapes(sqlib):
    from stochquant_amd import Phi4Ensemble, StochQuantError
    refused, one_where_corr_has_two = 0, False
    for shape in _legal_shapes():
        Lx, Ly, Lz = shape
        sites = Lx * Ly * Lz
        base = Phi4Ensemble.shape_info(shape)           # legal for the ensemble
        co = Phi4Ensemble.corr_shape_info(shape)
        need = [4 * sites + sc + 16 * Lz for sc in (SCRATCH, FRAME_SCRATCH, SCRATCH)]
        if max(need) > LIMIT:
            with pytest.raises(StochQuantError) as ei:
                Phi4Ensemble.pcorr_shape_info(shape)
            assert ei.value.code == -1, shape
            refused += 1
            continue
        pc = Phi4Ensemble.pcorr_shape_info(shape)
        assert pc["nt"] == Lz // 2 + 1
        for images, lds, scratch in ((pc["images"], pc["lds_bytes"], SCRATCH),
                                     (pc["frames_images"], pc["frames_lds_bytes"], FRAME_SCRATCH)):
            assert images in (1, 2)
            assert lds == images * 4 * sites + scratch + 16 * Lz, shape
            assert lds <= LIMIT == base["lds_limit"], shape
            assert (images == 2) == (2 * 4 * sites + scratch + 16 * Lz <= LIMIT), shape
        assert pc["slices_lds_bytes"] == 4 * sites + SCRATCH + 16 * Lz <= LIMIT
        # the correlator launches' layout with the slice region doubled
        assert pc["images"] <= co["images"] and pc["frames_images"] <= co["frames_images"]
        assert pc["lds_bytes"] - pc["images"] * 4 * sites == co["lds_bytes"] - co["images"] * 4 * sites + 8 * Lz
        one_where_corr_has_two |= pc["images"] < co["images"]
    assert refused >= 3 and one_where_corr_has_two
    with pytest.raises(StochQuantError):
        Phi4Ensemble.pcorr_shape_info((8, 2, 2048))     # 131,072 + 624 + 32,768 > 163,840
    assert Phi4Ensemble.pcorr_shape_info((8, 2, 2000))["frames_lds_bytes"] == 128000 + 624 + 32000
    assert Phi4Ensemble.pcorr_shape_info((8, 2, 2040))["frames_lds_bytes"] == 163824
    for bad in ((12, 8, 8), (8, 1, 8), (64, 32, 32)):   # refused as sq_phi4_ens_shape_info refuses them
        with pytest.raises(StochQuantError) as ei:
            Phi4Ensemble.pcorr_shape_info(bad)
        assert ei.value.code == -1


def test_older_shape_queries_unchanged(sqlib):
    """The plain and the correlator launches keep their layouts (values of the parent's rule, written out)."""
    from stochquant_amd import Phi4Ensemble
    want = {
        (8, 8, 8): ((1, 128, 2, 4672, 2, 4720, 2624, LIMIT), (2, 4736, 2, 4784, 2688, 5)),
        (32, 32, 32): ((8, 1024, 1, 131648, 1, 131696, 131648, LIMIT), (1, 131904, 1, 131952, 131904, 17)),
        (8, 2, 2048): ((8, 1024, 1, 131648, 1, 131696, 131648, LIMIT), (1, 148032, 1, 148080, 148032, 1025)),
        (64, 16, 8): ((2, 1024, 2, 66112, 2, 66160, 33344, LIMIT), (2, 66176, 2, 66224, 33408, 5)),
        (16, 4, 31): ((1, 512, 2, 16448, 2, 16496, 8512, LIMIT), (2, 16696, 2, 16744, 8760, 16)),
    }
    for shape, (plain, corr) in want.items():
        assert tuple(Phi4Ensemble.shape_info(shape).values()) == plain, shape
        assert tuple(Phi4Ensemble.corr_shape_info(shape).values()) == corr, shape
