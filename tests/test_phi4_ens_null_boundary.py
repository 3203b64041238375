"""Every sq_phi4_ens_* entry point without a GPU, table-driven from _lib.SIGNATURES: called with all-zero /
all-null arguments built from its argtypes, each returns SQ_E_ARG (-1) and leaves a message in sq_last_error() --
it checks its handle or its pointers before anything else -- and sq_phi4_ens_destroy(NULL) returns 0.  The host
side of these calls is split over several files (csrc/sq_phi4_ens*.cpp): an entry point that lost its export
fails the lookup here, one that lost its null check crashes or returns another code."""
import ctypes

SQ_E_ARG = -1


def _names():
    from stochquant_amd import _lib
    return sorted(n for n in _lib.SIGNATURES if n.startswith("sq_phi4_ens_"))


def _zero(t):
    """The all-zero value of a ctypes argument type: NULL for pointers, 0 for numbers."""
    if t is ctypes.c_void_p or hasattr(t, "contents"):
        return None
    return t(0)


def test_the_table_covers_the_ensembles_abi():
    from stochquant_amd import _lib
    names = _names()
    assert len(names) == 72
    for n in names:
        restype, argtypes = _lib.SIGNATURES[n]
        assert restype is ctypes.c_int and len(argtypes) >= 1, n


def test_every_entry_point_refuses_null_arguments(sqlib):
    from stochquant_amd import _lib
    called = 0
    for name in _names():
        fn = getattr(sqlib, name)                  # AttributeError: the library no longer exports it
        args = [_zero(t) for t in _lib.SIGNATURES[name][1]]
        assert all(a is None or a.value == 0 for a in args), name
        rc = fn(*args)
        called += 1
        if name == "sq_phi4_ens_destroy":
            assert rc == 0, name
            continue
        assert rc == SQ_E_ARG, (name, rc)
        assert sqlib.sq_last_error().decode() != "", name
    assert called == len(_names()) == 72
