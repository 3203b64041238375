"""The single lattice's Heun entry points at the library boundary (CPU only): exported, prototyped, bound,
refusing a null context before anything touches a device; Phi4Lattice.step's keyword rules, which are decided
before the library is called."""
import ctypes
import os

import pytest

from conftest import ROOT
from stochquant_amd import Phi4Lattice, _lib

NAMES = ("sq_phi4_step_heun", "sq_phi4_step_heun_meas")


def test_the_symbols_are_exported_prototyped_and_bound(sqlib):
    header = open(os.path.join(ROOT, "include", "stochquant.h")).read()
    for name in NAMES:
        assert name in _lib.SIGNATURES and f"int {name}(sq_ctx *ctx, int nsteps" in header, name
        fn = getattr(sqlib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(_lib.SIGNATURES[name][1])
    assert sqlib.sq_abi_version() == 6


def test_a_null_context_is_an_argument_error(sqlib):
    for rc in (sqlib.sq_phi4_step_heun(None, 1), sqlib.sq_phi4_step_heun_meas(None, 1, 1, None, 0)):
        assert rc == -1
        assert sqlib.sq_last_error().decode() != ""


@pytest.mark.parametrize("kw,word", [({"scheme": "rk4"}, "rk4"), ({"every": 1}, 'scheme="heun"'),
                                     ({"scheme": "euler", "correlate": True}, 'scheme="heun"'),
                                     ({"momenta": True}, 'scheme="heun"'),
                                     ({"scheme": "heun", "correlate": True}, "every")])
def test_step_keywords_are_checked_before_the_library(kw, word):
    lat = object.__new__(Phi4Lattice)      # no context: a call that reached the library would fail on _h
    with pytest.raises(ValueError) as ei:
        lat.step(2, **kw)
    assert word in str(ei.value)
