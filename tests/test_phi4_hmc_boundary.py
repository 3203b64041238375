"""The single lattice's HMC entry points at the library boundary (CPU only): exported, prototyped, declared in
the header, and refusing a null context before anything touches a device."""
import ctypes
import os

from stochquant_amd import _lib

NAMES = ("sq_phi4_step_hmc", "sq_phi4_hmc_stats", "sq_phi4_hmc_reset")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "stochquant.h")


def test_the_three_symbols_are_exported_and_prototyped(sqlib):
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        fn = getattr(sqlib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(_lib.SIGNATURES[name][1])
    assert sqlib.sq_abi_version() == 6


def test_the_header_declares_them():
    with open(HEADER) as fh:
        text = fh.read()
    for name in NAMES:
        assert f"int {name}(sq_ctx *ctx" in text, name
    assert "#define SQ_ABI_VERSION 6" in text


def test_a_null_context_is_an_argument_error(sqlib):
    out = (ctypes.c_longlong * 4)()
    for rc in (sqlib.sq_phi4_step_hmc(None, 1, 1, 0, None), sqlib.sq_phi4_hmc_stats(None, out),
               sqlib.sq_phi4_hmc_reset(None)):
        assert rc == -1
        assert sqlib.sq_last_error().decode() != ""
