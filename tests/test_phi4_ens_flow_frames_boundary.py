"""The boundary of the flow measurements in frames and Heun steps without a GPU:
libstochquant.so exports sq_phi4_ens_step_flow_heun, sq_phi4_ens_run_frames_flow and
sq_phi4_ens_frames_flow_shape_info and _lib.SIGNATURES binds them, the ABI version stays 6, a
NULL handle is an argument error on each, the Python signatures the earlier tests pin are
unchanged while `flow` is accepted as a keyword, the refusals come before any library call,
and sq_phi4_ens_frames_flow_shape_info (host only) reports the frames / correlator layouts
over every legal ensemble shape."""
import ctypes
import inspect

import pytest

from test_phi4_ens_shapes import legal_shapes

SYMBOLS = ["sq_phi4_ens_step_flow_heun", "sq_phi4_ens_run_frames_flow", "sq_phi4_ens_frames_flow_shape_info"]


def test_library_exports_the_symbols(sqlib):
    from stochquant_amd import _lib
    assert [s for s in SYMBOLS if not hasattr(sqlib, s)] == []
    assert [s for s in SYMBOLS if s not in _lib.SIGNATURES] == []
    assert sqlib.sq_abi_version() == _lib.ABI_VERSION == 6


def test_null_handle_is_an_argument_error(sqlib):
    d = (ctypes.c_double * 64)()
    i = (ctypes.c_int * 8)()
    assert sqlib.sq_phi4_ens_step_flow_heun(None, 4, 2, None, 0) == -1
    assert sqlib.sq_phi4_ens_step_flow_heun(None, 4, 2, d, 1) == -1
    for scheme in (0, 1, 2):
        assert sqlib.sq_phi4_ens_run_frames_flow(None, 1, i, d, d, 1, scheme) == -1
        assert sqlib.sq_phi4_ens_run_frames_flow(None, 0, None, None, None, 0, scheme) == -1
    assert sqlib.sq_phi4_ens_frames_flow_shape_info(None, i) == -1
    assert sqlib.sq_phi4_ens_frames_flow_shape_info((ctypes.c_int * 3)(8, 8, 8), None) == -1
    assert sqlib.sq_last_error().decode() != ""


def test_python_signatures(sqlib):
    from stochquant_amd import Phi4Ensemble

    def names(f):
        return list(inspect.signature(f).parameters)

    assert names(Phi4Ensemble.run_frames) == ["self", "n", "measure", "correlate", "momenta", "scheme"]
    assert names(Phi4Ensemble.run_frame) == ["self", "scheme"]
    assert names(Phi4Ensemble.step) == ["self", "n", "every", "correlate", "momenta", "scheme"]
    p = inspect.signature(Phi4Ensemble.step_flow).parameters
    assert list(p) == ["self", "n", "every", "correlate", "scheme"] and p["scheme"].default == "euler"
    p = inspect.signature(Phi4Ensemble.run_frames_flow).parameters
    assert list(p) == ["self", "n", "correlate", "scheme"]
    assert p["correlate"].default is False and p["scheme"].default == "euler"


def test_refusals_before_any_library_call(sqlib):
    from stochquant_amd import Phi4Ensemble
    E = Phi4Ensemble.__new__(Phi4Ensemble)      # no handle: a library call would fail differently
    E._h = ctypes.c_void_p()
    E.R = 2
    with pytest.raises(ValueError):
        E.run_frames(2, flow=True, momenta=True)
    with pytest.raises(ValueError):
        E.run_frames(2, flow=True, momenta=True, correlate=True, scheme="heun")
    with pytest.raises(ValueError):
        E.run_frames(2, flow=True, scheme="rk4")
    with pytest.raises(ValueError):
        E.run_frames_flow(2, scheme="rk4")
    with pytest.raises(ValueError):
        E.step_flow(4, 2, scheme="rk4")
    with pytest.raises(ValueError):
        E.step_flow(4, 0, scheme="heun")
    with pytest.raises(ValueError) as ei:       # the deliberate wart: step() does not reach the Heun flow
        E.step(4, every=2, flow=True, scheme="heun")
    assert "step_flow" in str(ei.value)
    with pytest.raises(TypeError):              # keyword-only
        E.run_frames(2, False, False, False, "euler", True)


def test_frames_flow_shape_info_over_legal_shapes(sqlib):
    from stochquant_amd import Phi4Ensemble, StochQuantError
    stash, seen = {}, set()
    for shape in legal_shapes():
        base = Phi4Ensemble.shape_info(shape)
        co = Phi4Ensemble.corr_shape_info(shape)
        hf = Phi4Ensemble.heun_frames_shape_info(shape)
        ff = Phi4Ensemble.frames_flow_shape_info(shape)
        # the frames launches of both schemes: the frames layout, with the correlator the correlator frames layout
        assert (ff["images"], ff["lds_bytes"]) == (base["frames_images"], base["frames_lds_bytes"]), shape
        assert (ff["images"], ff["lds_bytes"]) == (hf["images"], hf["lds_bytes"]), shape
        assert (ff["corr_images"], ff["corr_lds_bytes"]) == (co["frames_images"], co["frames_lds_bytes"]), shape
        # the Heun step launch: the step layouts, as step_flow's
        assert ff["heun_step_images"] == base["images"], shape
        assert (ff["heun_step_corr_images"], ff["heun_step_corr_lds_bytes"]) == (co["images"], co["lds_bytes"]), shape
        assert max(ff["lds_bytes"], ff["corr_lds_bytes"], ff["heun_step_corr_lds_bytes"]) <= base["lds_limit"], shape
        for name, imgs in (("stash", (ff["images"], ff["corr_images"])),
                           ("heun_stash", (ff["images"], ff["corr_images"])),
                           ("heun_step_stash", (ff["heun_step_images"], ff["heun_step_corr_images"]))):
            assert ff[name] in (0, 1), shape
            for im in imgs:                     # uniform per (K, images)
                assert stash.setdefault((name, base["K"], im), ff[name]) == ff[name], (shape, name)
        assert 0 <= ff["mask"] <= 0xf, shape
        for corr, im in ((0, ff["images"]), (1, ff["corr_images"])):
            assert ff["mask"] >> corr & 1, shape                      # the Euler frames never lack a bit
            if not ff["mask"] >> (2 + corr) & 1:                      # a lacking bit: K = 8 with one image only
                assert base["K"] == 8 and im == 1, (shape, ff)
        seen.add(base["K"])
    assert seen == {1, 2, 4, 8}
    # the frames kernels stash in the replica's row for every K; the Heun step kernel as step_flow's
    assert Phi4Ensemble.frames_flow_shape_info((8, 8, 8))["stash"] == 1
    assert Phi4Ensemble.frames_flow_shape_info((8, 8, 8))["heun_step_stash"] == \
        Phi4Ensemble.flow_shape_info((8, 8, 8))["stash"] == 0
    assert Phi4Ensemble.frames_flow_shape_info((32, 32, 32))["heun_step_stash"] == 1
    for bad in ((12, 8, 8), (8, 1, 8), (64, 32, 32), (8, 2, 2049)):   # refused as sq_phi4_ens_shape_info refuses them
        with pytest.raises(StochQuantError) as ei:
            Phi4Ensemble.frames_flow_shape_info(bad)
        assert ei.value.code == -1
        with pytest.raises(StochQuantError):
            Phi4Ensemble.shape_info(bad)
