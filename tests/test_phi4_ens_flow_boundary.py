"""The gradient-flow measurements' boundary without a GPU: libstochquant.so
exports the sq_phi4_ens_*flow* / _flowed / _fcorr* symbols and _lib.SIGNATURES
binds them, the ABI version stays 6, a NULL handle is an argument error on
every entry, Phi4Ensemble.step refuses the combinations that are out of scope
before any library call, and the flow launches' LDS requests
(sq_phi4_ens_flow_shape_info, host only) are the plain and the correlator
launches' over every class of legal ensemble shape."""
import ctypes

import pytest

from test_phi4_ens_pcorr_boundary import _legal_shapes

FLOW_SYMBOLS = ["sq_phi4_ens_set_flow", "sq_phi4_ens_get_flow", "sq_phi4_ens_step_flow", "sq_phi4_ens_flowed",
                "sq_phi4_ens_flow_field", "sq_phi4_ens_fcorr_sums", "sq_phi4_ens_fcorr_reset",
                "sq_phi4_ens_fcorrelator", "sq_phi4_ens_flow_shape_info"]


def test_library_exports_the_flow_symbols(sqlib):
    from stochquant_amd import _lib
    assert [s for s in FLOW_SYMBOLS if not hasattr(sqlib, s)] == []
    assert [s for s in FLOW_SYMBOLS if s not in _lib.SIGNATURES] == []
    assert sqlib.sq_abi_version() == _lib.ABI_VERSION == 6
    assert _lib.SQ_PHI4_ENS_MAX_FLOW_LEVELS == 4
    assert _lib.SQ_PHI4_ENS_MAX_FLOW_STEPS == 4096


def test_header_states_the_constants():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                            "stochquant.h")).read()
    assert re.search(r"#define SQ_PHI4_ENS_MAX_FLOW_LEVELS 4\b", hdr)
    assert re.search(r"#define SQ_PHI4_ENS_MAX_FLOW_STEPS 4096\b", hdr)
    assert re.search(r"#define SQ_ABI_VERSION 6\b", hdr)


def test_null_handle_is_an_argument_error(sqlib):
    d = (ctypes.c_double * 8)()
    i = (ctypes.c_int * 8)()
    f = (ctypes.c_float * 8)()
    n = (ctypes.c_longlong * 8)()
    lev = (ctypes.c_int * 2)(0, 3)
    assert sqlib.sq_phi4_ens_set_flow(None, 0.05, 2, lev, None, None) == -1
    assert sqlib.sq_phi4_ens_set_flow(None, 0.05, 0, None, None, None) == -1
    assert sqlib.sq_phi4_ens_get_flow(None, d, i, i, d, d) == -1
    assert sqlib.sq_phi4_ens_step_flow(None, 4, 2, None, 0) == -1
    assert sqlib.sq_phi4_ens_step_flow(None, 4, 2, d, 1) == -1
    assert sqlib.sq_phi4_ens_flowed(None, 0, 1, d, d, d) == -1
    assert sqlib.sq_phi4_ens_flow_field(None, 0, 1, 3, f) == -1
    assert sqlib.sq_phi4_ens_fcorr_sums(None, 0, 1, d, d, n) == -1
    assert sqlib.sq_phi4_ens_fcorr_reset(None, 0, 1) == -1
    assert sqlib.sq_phi4_ens_fcorrelator(None, 1, d, d, 1, i) == -1
    assert sqlib.sq_phi4_ens_flow_shape_info(None, i) == -1
    assert sqlib.sq_phi4_ens_flow_shape_info((ctypes.c_int * 3)(8, 8, 8), None) == -1
    assert sqlib.sq_last_error().decode() != ""


def test_flow_refusals_before_any_device_call(sqlib):
    from stochquant_amd import Phi4Ensemble
    E = Phi4Ensemble.__new__(Phi4Ensemble)      # no handle: a library call would fail differently
    E._h = ctypes.c_void_p()
    E.R = 2
    for every in (0, -1):
        with pytest.raises(ValueError):
            E.step(4, every=every, flow=True)
        with pytest.raises(ValueError):
            E.step(4, every=every, flow=True, correlate=True)
    with pytest.raises(ValueError):
        E.step(4, every=2, flow=True, momenta=True)
    with pytest.raises(ValueError):
        E.step(4, every=2, flow=True, momenta=True, correlate=True)
    with pytest.raises(ValueError):
        E.step(4, every=2, flow=True, scheme="heun")


def test_flow_shape_info_over_legal_shapes(sqlib):
    from stochquant_amd import Phi4Ensemble, StochQuantError
    stash = {}
    for shape in _legal_shapes():
        base = Phi4Ensemble.shape_info(shape)
        co = Phi4Ensemble.corr_shape_info(shape)
        fl = Phi4Ensemble.flow_shape_info(shape)
        assert (fl["images"], fl["lds_bytes"]) == (base["images"], base["lds_bytes"]), shape
        assert (fl["corr_images"], fl["corr_lds_bytes"]) == (co["images"], co["lds_bytes"]), shape
        # the flowed launch flows and measures: the correlator step launch's layout
        assert fl["flowed_lds_bytes"] == co["lds_bytes"] <= base["lds_limit"], shape
        assert fl["stash"] in (0, 1), shape
        for key in ((base["K"], base["images"]), (base["K"], co["images"])):
            assert stash.setdefault(key, fl["stash"]) == fl["stash"], (shape, key)
    assert {k for k, _ in stash} == {1, 2, 4, 8}
    # at K = 8 with 1024 lanes the register budget leaves no room for a second copy of the lane's quads
    assert Phi4Ensemble.flow_shape_info((32, 32, 32))["stash"] == 1
    assert tuple(Phi4Ensemble.flow_shape_info((8, 8, 8)).values())[:5] == (2, 4672, 2, 4736, 4736)
    assert tuple(Phi4Ensemble.flow_shape_info((8, 2, 2048)).values())[:5] == (1, 131648, 1, 148032, 148032)
    for bad in ((12, 8, 8), (8, 1, 8), (64, 32, 32), (8, 2, 2049)):   # refused as sq_phi4_ens_shape_info refuses them
        with pytest.raises(StochQuantError) as ei:
            Phi4Ensemble.flow_shape_info(bad)
        assert ei.value.code == -1
