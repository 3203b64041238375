"""The phi^4 ensemble's frame entry points without a GPU: the library exports
them, they check their arguments before any device work, the Python class
carries `loops` / `adapt_dtau` and the frame methods, the ABI version stays 6,
and no instance of the resident kernels (raw steps or frames) uses private
memory (a spilled register in a kernel that keeps its lattice in registers for
a whole call costs every step)."""
import ctypes
import inspect
import os

FRAME_SYMBOLS = ["sq_phi4_ens_run_frames", "sq_phi4_ens_stability", "sq_phi4_ens_set_stability"]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_the_frame_symbols(sqlib):
    from stochquant_amd import _lib
    assert [s for s in FRAME_SYMBOLS if not hasattr(sqlib, s)] == []
    assert [s for s in FRAME_SYMBOLS if s not in _lib.SIGNATURES] == []


def test_null_ensemble_is_an_argument_error(sqlib):
    st = (ctypes.c_int * 4)()
    dt = (ctypes.c_double * 4)()
    assert sqlib.sq_phi4_ens_run_frames(None, 1, st, dt, None) == -1
    assert sqlib.sq_last_error().decode() != ""
    assert sqlib.sq_phi4_ens_run_frames(None, 0, None, None, None) == -1
    assert sqlib.sq_phi4_ens_stability(None, 0, 1, None, None, None, None, None, 0) == -1
    assert sqlib.sq_phi4_ens_set_stability(None, 0, 1, dt, dt) == -1


def test_abi_version_is_still_6(sqlib):
    from stochquant_amd import _lib
    assert sqlib.sq_abi_version() == _lib.ABI_VERSION == 6


def test_python_class_has_the_frame_interface(sqlib):
    from stochquant_amd import Phi4Ensemble, Phi4Lattice
    sig = inspect.signature(Phi4Ensemble.__init__).parameters
    ref = inspect.signature(Phi4Lattice.__init__).parameters
    for k in ("loops", "adapt_dtau"):
        assert k in sig and sig[k].default == ref[k].default, k
    for m in ("run_frames", "run_frame", "stability", "set_stability"):
        assert callable(getattr(Phi4Ensemble, m, None)), m
    assert "measure" in inspect.signature(Phi4Ensemble.run_frames).parameters


def test_resident_kernels_use_no_private_memory(sqlib):
    from stochquant_amd import isa_check
    md = isa_check.kernel_metadata(os.path.join(ROOT, "stochquant_amd", "lib", "libstochquant.so"))
    frames = {k: v for k, v in md.items() if "phi4_ens_frames_kernel" in k}
    steps = {k: v for k, v in md.items() if "phi4_ens_step_kernel" in k}
    assert len(frames) >= 4 and len(steps) >= 4, sorted(k for k in md if "phi4_ens" in k)
    bad = {k: v for k, v in {**frames, **steps}.items() if v.get("private", 0) != 0 or v.get("vgpr_spill", 0) != 0}
    assert bad == {}, bad
