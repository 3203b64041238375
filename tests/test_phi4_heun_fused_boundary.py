"""The fused Heun entry points at the library boundary (CPU only): exported, prototyped, bound, refusing a null
context before anything touches a device; the fused keyword's rule; the shapes the fused step serves."""
import ctypes
import os

import pytest

from conftest import ROOT
from stochquant_amd import Phi4Lattice, _lib

NAMES = ("sq_phi4_step_heun_fused", "sq_phi4_step_heun_fused_meas", "sq_phi4_heun_fused_shape_info")


def test_the_symbols_are_exported_prototyped_and_bound(sqlib):
    header = open(os.path.join(ROOT, "include", "stochquant.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and f"int {name}(" in header, name
        fn = getattr(sqlib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(_lib.SIGNATURES[name][1])
    assert sqlib.sq_abi_version() == 6


def test_null_arguments_are_argument_errors(sqlib):
    dims = (ctypes.c_int * 3)(256, 8, 2)
    for rc in (sqlib.sq_phi4_step_heun_fused(None, 1), sqlib.sq_phi4_step_heun_fused_meas(None, 1, 1, None, 0),
               sqlib.sq_phi4_heun_fused_shape_info(dims, None), sqlib.sq_phi4_heun_fused_shape_info(None, None)):
        assert rc == -1
        assert sqlib.sq_last_error().decode() != ""


def test_fused_needs_heun_before_the_library():
    lat = object.__new__(Phi4Lattice)      # no context: a call that reached the library would fail on _h
    with pytest.raises(ValueError) as ei:
        lat.step(2, scheme="euler", fused=True)
    assert 'scheme="heun"' in str(ei.value)


@pytest.mark.parametrize("shape,want", [((256, 8, 2), (True, False, True)), ((512, 16, 5), (True, True, True)),
                                        ((256, 4, 6), (False, False, False)), ((64, 8, 8), (False, False, False)),
                                        ((256, 8, 1), (False, False, False)),
                                        ((1024, 1024, 512), (True, True, False))])   # 514 planes of 4 MiB: past 2^31 B
def test_shape_info(sqlib, shape, want):
    info = Phi4Lattice.heun_fused_shape_info(shape)
    assert (info["supported"], info["wide"], info["one_descriptor"]) == want
