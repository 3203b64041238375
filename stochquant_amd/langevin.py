"""Host-side mirror of the reference's interface for the Langevin path.

The reference exposes no Python API: `taumain.py:132` spawns `./tauhost.o`
with 13 positional arguments and parses its stdout.  This module offers that
same contract (`run_tauhost`, `parse_frame_line`) plus thin numpy wrappers of
the C ABI for the two models:

* `Qm1dChain`  -- tau_kernel.cl time_dev + the tauhost.c frame loop (fp64)
* `Qm1dEnsemble` -- R such chains per launch, one work-group per replica
* `Phi4Lattice` -- the 3-D fp32 north-star extension (slab / multi-GPU)
* `Phi4Ensemble` -- R small φ⁴ lattices per launch, each on-chip in one work-group

Everything computes on the MI355X through libstochquant.so; nothing here has a
CPU path.
"""
import ctypes
import functools
import inspect
import io
import os
import subprocess

import numpy as np

from . import _lib
from ._lib import (SQ_COMM_LOOPBACK, SQ_COMM_NONE, SQ_COMM_P2P, SQ_COMM_RCCL, SQ_MODEL_PHI4, SQ_MODEL_QM1D, SQ_ORDER_JACOBI,
                   SQ_ORDER_SERIAL)

_DP = ctypes.POINTER(ctypes.c_double)
_FP = ctypes.POINTER(ctypes.c_float)


def _dptr(a):
    return a.ctypes.data_as(_DP)


def _fptr(a):
    return a.ctypes.data_as(_FP)


class _Ctx:
    def __init__(self, params):
        self._h = ctypes.c_void_p()
        _lib.call("sq_create", ctypes.byref(params), ctypes.byref(self._h))
        self.params = params

    def close(self):
        if self._h:
            _lib.call("sq_destroy", self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # shared controls ------------------------------------------------------
    @property
    def dtau(self):
        d = ctypes.c_double()
        _lib.call("sq_get_dtau", self._h, ctypes.byref(d))
        return d.value

    @dtau.setter
    def dtau(self, v):
        _lib.call("sq_set_dtau", self._h, float(v))

    @property
    def step_counter(self):
        s = ctypes.c_ulonglong()
        _lib.call("sq_get_step", self._h, ctypes.byref(s))
        return s.value

    @step_counter.setter
    def step_counter(self, v):
        _lib.call("sq_set_step", self._h, int(v))

    def run_frame(self):
        """`loops` steps + stability check + rollback + Δτ control; returns True if stable."""
        st = ctypes.c_int()
        _lib.call("sq_run_frame", self._h, ctypes.byref(st))
        return st.value == 1

    def run_frames(self, n):
        """n frames back to back (sq_run_frames: for phi^4 the verdict, rollback
        and Δτ controller stay on the device); returns (stable bool array, Δτ
        after each frame)."""
        import numpy as np
        st = np.zeros(max(n, 1), dtype=np.int32)
        dt = np.zeros(max(n, 1), dtype=np.float64)
        _lib.call("sq_run_frames", self._h, int(n), st.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                  dt.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
        return st[:n] == 1, dt[:n]

    def set_profiling(self, mode=1):
        """0 off; 1 every step kernel timed by dispatch events; 2 one event pair per step() call."""
        _lib.call("sq_set_profiling", self._h, int(mode))

    def perf(self):
        p = _lib.SqPerf()
        _lib.call("sq_perf", self._h, ctypes.byref(p))
        return {k: getattr(p, k) for k, _ in p._fields_}

    def perf_reset(self):
        _lib.call("sq_perf_reset", self._h)

    def sync(self):
        _lib.call("sq_sync", self._h)

    def set_noise(self, C):
        """Noise amplitude C of the open context (C = 0: drift only, deterministic)."""
        _lib.call("sq_set_noise", self._h, float(C))
        self.params.C = float(C)


class Qm1dChain(_Ctx):
    """The reference's 1-D chain: N sites (Δt spacing), potID 0 or 3, noise C,
    `loops` steps per frame (tauhost.c argv[1..10] meaning)."""

    def __init__(self, N, deltat, deltatau, pot=3, C=1.0, loops=1000, seed=0x5EED, device=0,
                 adapt_dtau=True, ordering="jacobi", lcg_seed=None):
        p = _lib.default_params()
        p.model = SQ_MODEL_QM1D
        p.dims[0] = int(N)
        p.deltat = float(deltat)
        p.deltatau = float(deltatau)
        p.pot = int(pot)
        p.C = float(C)
        p.loops = int(loops)
        p.seed = int(seed)
        p.device = int(device)
        p.adapt_dtau = 1 if adapt_dtau else 0
        super().__init__(p)
        self.N = int(N)
        if ordering != "jacobi":
            self.set_ordering(ordering)
        if lcg_seed is not None:
            self.lcg_seed = lcg_seed

    def set_ordering(self, ordering):
        """"jacobi" (Philox noise, the fast path) or "serial" (the reference's
        Gauss-Seidel order with its shared-seed LCG, SQ_ORDER_SERIAL)."""
        _lib.call("sq_qm1d_set_ordering", self._h, {"jacobi": SQ_ORDER_JACOBI, "serial": SQ_ORDER_SERIAL}[ordering])

    @property
    def lcg_seed(self):
        v = ctypes.c_ulonglong()
        _lib.call("sq_qm1d_get_lcg_seed", self._h, ctypes.byref(v))
        return v.value

    @lcg_seed.setter
    def lcg_seed(self, v):
        _lib.call("sq_qm1d_set_lcg_seed", self._h, int(v))

    def inject_noise(self, xi):
        """Draws for the next serial frame, in call order (round*(N+1) + item)."""
        xi = np.ascontiguousarray(xi, dtype=np.float64)
        _lib.call("sq_qm1d_inject_noise", self._h, _dptr(xi), xi.size)

    @property
    def noise_consumed(self):
        v = ctypes.c_ulonglong()
        _lib.call("sq_qm1d_noise_consumed", self._h, ctypes.byref(v))
        return v.value

    def upload(self, f, x=None, xx0=None, omega=0.0, runs=0):
        f = np.ascontiguousarray(f, dtype=np.float64)
        x = np.zeros(self.N) if x is None else np.ascontiguousarray(x, dtype=np.float64)
        xx0 = np.zeros(self.N) if xx0 is None else np.ascontiguousarray(xx0, dtype=np.float64)
        if f.shape != (self.N,) or x.shape != (self.N,) or xx0.shape != (self.N,):
            raise ValueError("state arrays must have N entries")
        _lib.call("sq_upload", self._h, _dptr(f), _dptr(x), _dptr(xx0), float(omega), int(runs))

    def download(self):
        f, x, xx0 = np.empty(self.N), np.empty(self.N), np.empty(self.N)
        om = ctypes.c_double()
        runs = ctypes.c_long()
        _lib.call("sq_download", self._h, _dptr(f), _dptr(x), _dptr(xx0), ctypes.byref(om), ctypes.byref(runs))
        return {"f": f, "x": x, "xx0": xx0, "omega": om.value, "runs": runs.value}

    @property
    def scan(self):
        e, v, t = ctypes.c_int(), ctypes.c_double(), ctypes.c_ulonglong()
        _lib.call("sq_qm1d_get_scan", self._h, ctypes.byref(e), ctypes.byref(v), ctypes.byref(t))
        return {"lrgEl": e.value, "lrgVl": v.value, "tick": t.value}

    def set_scan(self, lrgEl, lrgVl, tick):
        _lib.call("sq_qm1d_set_scan", self._h, int(lrgEl), float(lrgVl), int(tick))

    def xavg(self):
        """xavg = xx0 - x * x[mid] (tauhost.c:519-521)."""
        out = np.empty(self.N)
        _lib.call("sq_correlator", self._h, _dptr(out), self.N)
        return out


class Qm1dEnsemble:
    """`replicas` independent Qm1dChain-equivalent chains (Jacobi order, Philox
    noise) advanced together, one frame per launch, one work-group per replica
    (sq_ens_*).  Replica r behaves bit for bit as a `Qm1dChain` with
    seed = seeds[r] (default seed + r) given the same uploads and frame calls;
    the Δτ controller acts per replica.  2 <= N <= 4096, potID 0 or 3."""

    def __init__(self, N, deltat, deltatau, replicas, seeds=None, pot=3, C=1.0, loops=1000, seed=0x5EED,
                 adapt_dtau=True, device=0):
        p = _lib.default_params()
        p.model = SQ_MODEL_QM1D
        p.dims[0] = int(N)
        p.deltat = float(deltat)
        p.deltatau = float(deltatau)
        p.pot = int(pot)
        p.C = float(C)
        p.loops = int(loops)
        p.seed = int(seed)
        p.device = int(device)
        p.adapt_dtau = 1 if adapt_dtau else 0
        self._h = ctypes.c_void_p()
        sp = None
        if seeds is not None:
            s = np.ascontiguousarray(seeds, dtype=np.uint64)
            if s.shape != (int(replicas),):
                raise ValueError("seeds must have one entry per replica")
            sp = s.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong))
        _lib.call("sq_ens_create", ctypes.byref(p), int(replicas), sp, ctypes.byref(self._h))
        self.params = p
        self.N = int(N)
        self.R = int(replicas)

    def close(self):
        if self._h:
            _lib.call("sq_ens_destroy", self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _rows(self, a, k, name):
        """(N,) -> k equal rows; (k, N) as given."""
        a = np.asarray(a, dtype=np.float64)
        if a.shape == (self.N,):
            a = np.broadcast_to(a, (k, self.N))
        if a.shape != (k, self.N):
            raise ValueError(f"{name} must have shape (N,) or ({k}, N)")
        return np.ascontiguousarray(a)

    def upload(self, f, x=None, xx0=None, omega=0.0, runs=0, first=0):
        """State of replicas first .. first + k: arrays of shape (N,) go to every
        replica (k = all of them from `first`), arrays of shape (k, N) to k
        replicas; omega and runs are scalars or have k entries."""
        k = None
        for a in (f, x, xx0):
            if a is not None and np.ndim(a) == 2:
                k = np.shape(a)[0]
        if k is None:
            k = self.R - int(first)
        f = self._rows(f, k, "f")
        x = None if x is None else self._rows(x, k, "x")
        xx0 = None if xx0 is None else self._rows(xx0, k, "xx0")
        om = np.ascontiguousarray(np.broadcast_to(np.asarray(omega, dtype=np.float64), (k,)))
        rn = np.ascontiguousarray(np.broadcast_to(np.asarray(runs, dtype=np.int64), (k,)).astype(ctypes.c_long))
        _lib.call("sq_ens_upload", self._h, int(first), int(k), _dptr(f), None if x is None else _dptr(x),
                  None if xx0 is None else _dptr(xx0), _dptr(om), rn.ctypes.data_as(ctypes.POINTER(ctypes.c_long)))

    def download(self, first=0, count=None):
        k = self.R - int(first) if count is None else int(count)
        f, x, xx0 = (np.empty((max(k, 0), self.N)) for _ in range(3))
        om = np.empty(max(k, 0))
        runs = np.empty(max(k, 0), dtype=ctypes.c_long)
        _lib.call("sq_ens_download", self._h, int(first), k, _dptr(f), _dptr(x), _dptr(xx0), _dptr(om),
                  runs.ctypes.data_as(ctypes.POINTER(ctypes.c_long)))
        return {"f": f, "x": x, "xx0": xx0, "omega": om, "runs": runs.astype(np.int64)}

    def run_frames(self, n):
        """n frames of every replica back to back (n launches, one read-back);
        returns the (n, R) bool matrix of verdicts."""
        st = np.zeros((max(int(n), 0), self.R), dtype=np.int32)
        _lib.call("sq_ens_run_frames", self._h, int(n), st.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        return st == 1

    def run_frame(self):
        """One frame of every replica; returns the (R,) bool array of verdicts."""
        return self.run_frames(1)[0]

    @property
    def dtau(self):
        d = np.empty(self.R)
        _lib.call("sq_ens_get_dtau", self._h, 0, self.R, _dptr(d))
        return d

    @dtau.setter
    def dtau(self, v):
        d = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64), (self.R,)))
        _lib.call("sq_ens_set_dtau", self._h, 0, self.R, _dptr(d))

    @property
    def scan(self):
        e = np.empty(self.R, dtype=np.int32)
        v = np.empty(self.R)
        t = np.empty(self.R, dtype=np.uint64)
        _lib.call("sq_ens_get_scan", self._h, 0, self.R, e.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _dptr(v),
                  t.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)))
        return {"lrgEl": e, "lrgVl": v, "tick": t}

    def set_scan(self, lrgEl, lrgVl, tick):
        """Scalars (every replica) or (R,) arrays."""
        e = np.ascontiguousarray(np.broadcast_to(np.asarray(lrgEl, dtype=np.int32), (self.R,)))
        v = np.ascontiguousarray(np.broadcast_to(np.asarray(lrgVl, dtype=np.float64), (self.R,)))
        t = np.ascontiguousarray(np.broadcast_to(np.asarray(tick, dtype=np.uint64), (self.R,)))
        _lib.call("sq_ens_set_scan", self._h, 0, self.R, e.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _dptr(v),
                  t.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)))

    def correlator(self, n=None):
        """(mean, standard error) over the replicas of xx0 - x * x[mid], per site."""
        n = self.N if n is None else int(n)
        mean, err = np.empty(n), np.empty(n)
        _lib.call("sq_ens_correlator", self._h, _dptr(mean), _dptr(err), n)
        return mean, err

    def perf(self):
        p = _lib.SqPerf()
        _lib.call("sq_ens_perf", self._h, ctypes.byref(p))
        return {k: getattr(p, k) for k, _ in p._fields_}


class Phi4Lattice(_Ctx):
    """Periodic 3-D φ⁴ lattice (Lx, Ly, Lz) in fp32, V = m²/2 φ² + λ/24 φ⁴.

    comm="none"     one slab, z wraps in-kernel
    comm="loopback" `nslabs` slabs on one device, halos by D2D copies
    comm="rccl"     one slab per process (rank / nranks), halos over RCCL;
                    `comm_id` from `unique_id()` on rank 0
    comm="p2p"      one slab per process, halos pulled from the neighbours'
                    memory (IPC peer pointers), no RCCL; every rank passes
                    all ranks' `p2p_handle()` blobs, in rank order, to
                    `p2p_connect` before stepping (`connect_p2p` does it over
                    a torch.distributed group)
    """

    def __init__(self, shape, dtau=0.01, m2=1.0, lam=1.0, seed=0x5EED, device=0, comm="none",
                 nslabs=1, nranks=1, rank=0, comm_id=None, clamp=1000.0, loops=100, C=1.0,
                 adapt_dtau=True):
        p = _lib.default_params()
        p.model = SQ_MODEL_PHI4
        for i in range(3):
            p.dims[i] = int(shape[i])
        p.deltatau = float(dtau)
        p.m2 = float(m2)
        p.lambda_ = float(lam)
        p.seed = int(seed)
        p.device = int(device)
        p.clamp = float(clamp)
        p.loops = int(loops)
        p.C = float(C)
        p.adapt_dtau = 1 if adapt_dtau else 0
        p.comm = {"none": SQ_COMM_NONE, "loopback": SQ_COMM_LOOPBACK, "rccl": SQ_COMM_RCCL, "p2p": SQ_COMM_P2P}[comm]
        p.nslabs = int(nslabs)
        p.nranks = int(nranks)
        p.rank = int(rank)
        if comm_id is not None:
            b = bytes(comm_id)
            ctypes.memmove(p.comm_id, b, min(len(b), 128))
        super().__init__(p)
        self.shape = tuple(int(s) for s in shape)
        nz, z0 = ctypes.c_longlong(), ctypes.c_longlong()
        _lib.call("sq_slab", self._h, ctypes.byref(nz), ctypes.byref(z0))
        self.nz_local, self.z0 = nz.value, z0.value

    @property
    def local_shape(self):
        return (self.nz_local, self.shape[1], self.shape[0])  # numpy order: z, y, x

    def step(self, n=1):
        _lib.call("sq_step", self._h, int(n))

    def upload(self, phi):
        a = np.ascontiguousarray(phi, dtype=np.float32)
        if a.size != int(np.prod(self.local_shape)):
            raise ValueError(f"field must have {self.local_shape} entries")
        _lib.call("sq_upload_field", self._h, _fptr(a), a.size)

    def download(self):
        a = np.empty(self.local_shape, dtype=np.float32)
        _lib.call("sq_download_field", self._h, _fptr(a), a.size)
        return a

    def init_field(self, amp):
        _lib.call("sq_init_field", self._h, float(amp))

    def init_field_hash(self, amp, key):
        """phi = amp * (top 24 bits of splitmix64(global index ^ key) - 2^23) / 2^23 (sq_init_field_hash)."""
        _lib.call("sq_init_field_hash", self._h, float(amp), int(key))

    def moments(self):
        out = np.zeros(3)
        _lib.call("sq_moments", self._h, _dptr(out))
        return {"sum": out[0], "sum2": out[1], "maxabs": out[2]}

    @property
    def tile(self):
        """(lanes per x segment, rows per lane, z planes per wave, float4 segments per lane)."""
        out = (ctypes.c_int * 4)()
        _lib.call("sq_phi4_tile", self._h, out)
        return tuple(out)

    @property
    def kernel_name(self):
        """The step kernel instance as rocprofv3 names it, plus the z-chunk."""
        buf = ctypes.create_string_buffer(160)
        _lib.call("sq_phi4_kernel", self._h, buf, len(buf))
        return buf.value.decode()

    def launch_info(self):
        """The step kernel launched most often since perf_reset(): {"kernel": template
        instance as rocprofv3 names it, "grid": threads, "launches": n}."""
        buf = ctypes.create_string_buffer(160)
        g, n = ctypes.c_longlong(), ctypes.c_longlong()
        _lib.call("sq_phi4_launch_info", self._h, buf, len(buf), ctypes.byref(g), ctypes.byref(n))
        return {"kernel": buf.value.decode(), "grid": g.value, "launches": n.value}

    @property
    def ghost(self):
        """(active, allocated) ghost-zone depth of a slab decomposition; (0, 0) for one periodic slab."""
        a, b = ctypes.c_int(), ctypes.c_int()
        _lib.call("sq_phi4_ghost", self._h, ctypes.byref(a), ctypes.byref(b))
        return a.value, b.value

    @property
    def schedule(self):
        """{"ghost", "core_pairs", "rims_b", "edge_first", "tuned", "exchange_in_order", "kstaged"} of a slab
        decomposition's block schedule (sq_phi4_schedule, sq_phi4_edge_first, sq_phi4_exchange_stream)."""
        k, b, t, e = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib.call("sq_phi4_schedule", self._h, ctypes.byref(k), ctypes.byref(b), ctypes.byref(t))
        _lib.call("sq_phi4_edge_first", self._h, ctypes.byref(e))
        a, ks = ctypes.c_int(), ctypes.c_int()
        _lib.call("sq_phi4_exchange_stream", self._h, ctypes.byref(a), ctypes.byref(ks))
        return {"ghost": self.ghost[0], "core_pairs": k.value, "rims_b": bool(b.value), "edge_first": bool(e.value),
                "tuned": bool(t.value), "exchange_in_order": bool(a.value), "kstaged": bool(ks.value)}

    def save(self, path):
        """Binary checkpoint: <path> (.npy float32 (nz, Ly, Lx)) + <path>.json (step, dtau, seed, z0)."""
        _lib.call("sq_save_field", self._h, os.fsencode(path))

    def load(self, path, restore_counters=True):
        _lib.call("sq_load_field", self._h, os.fsencode(path), 1 if restore_counters else 0)

    def stability(self, n=None):
        """The frame stability heuristic's state: {"T", "V", "fired" (step of the
        last frame it fired at, -1 none), "M", "D", "A" (that frame's per-step
        records)} -- DESIGN.md §7."""
        n = self.params.loops if n is None else int(n)
        st = np.zeros(2)
        fired = ctypes.c_int()
        M, D, A = (np.zeros(n, dtype=np.float32) for _ in range(3))
        _lib.call("sq_phi4_stability", self._h, _dptr(st), ctypes.byref(fired), _fptr(M), _fptr(D), _fptr(A), n)
        return {"T": st[0], "V": st[1], "fired": fired.value, "M": M, "D": D, "A": A}

    def block_stamps(self, cap=1 << 16):
        """Run 2 steps (one fused launch) with per-block clock stamps; returns
        (start, end) int64 arrays in ticks of the 100 MHz constant clock."""
        a = np.zeros(2 * cap, dtype=np.uint64)
        nb = ctypes.c_int()
        _lib.call("sq_phi4_block_stamps", self._h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)), int(cap),
                  ctypes.byref(nb))
        a = a[:2 * nb.value].astype(np.int64)
        return a[0::2], a[1::2]

    def block_clocks(self, cap=1 << 16):
        """The last block_stamps launch's shader-clock counter (s_memtime) at each
        block's start and end: (start, end) int64 arrays in shader cycles."""
        a = np.zeros(2 * cap, dtype=np.uint64)
        nb = ctypes.c_int()
        _lib.call("sq_phi4_block_clocks", self._h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)), int(cap),
                  ctypes.byref(nb))
        a = a[:2 * nb.value].astype(np.int64)
        return a[0::2], a[1::2]

    def set_stability(self, T, V):
        _lib.call("sq_phi4_set_stability", self._h, float(T), float(V))

    def correlator(self, n=None):
        n = self.shape[2] if n is None else int(n)
        out = np.empty(n)
        _lib.call("sq_correlator", self._h, _dptr(out), n)
        return out

    def p2p_handle(self):
        """This rank's SQ_COMM_P2P handle blob (bytes) for the other ranks."""
        buf = (ctypes.c_ubyte * _lib.SQ_P2P_HANDLE_BYTES)()
        _lib.call("sq_p2p_handle", self._h, buf)
        return bytes(buf)

    def p2p_connect(self, blobs):
        """Map the peers of an SQ_COMM_P2P context: `blobs` = every rank's p2p_handle(), in rank order."""
        n = _lib.SQ_P2P_HANDLE_BYTES
        if any(len(b) != n for b in blobs):
            raise ValueError(f"every handle blob has {n} bytes")
        buf = (ctypes.c_ubyte * (n * len(blobs))).from_buffer_copy(b"".join(blobs))
        _lib.call("sq_p2p_connect", self._h, buf, len(blobs))


_MALA_NO_FRAMES = ("frames do not run with scheme='mala': the stability rule and the dtau controller have no meaning "
                   "under an accept/reject step (use step(scheme='mala') and mala_stats())")


def _refuse_hmc(scheme, what):
    """Trajectories have an interface of their own: no call that takes a scheme runs them."""
    if scheme == "hmc":
        raise ValueError(f"{what} does not run with scheme='hmc': trajectories are step_hmc(n, nleap, ...), which takes "
                         "their length (momenta, the flow and frames do not run with them, as with scheme='mala')")


def _accepts_flow(step):
    """`Phi4Ensemble.step` with the keyword-only `flow`: flow=True hands the call
    to `step_flow` after refusing what the flow does not run with.  The
    positional parameters, their order and their defaults stay those of `step`
    itself, which is what introspection reports (functools.wraps)."""
    sig = inspect.signature(step)

    @functools.wraps(step)
    def wrapper(self, *args, flow=False, **kw):
        if not flow:
            return step(self, *args, **kw)
        a = sig.bind(self, *args, **kw)
        a.apply_defaults()
        a = a.arguments
        _refuse_hmc(a["scheme"], "step")
        if a["scheme"] == "mala":
            raise ValueError("scheme='mala' does not run with flow=True (use flowed() between calls)")
        if a["scheme"] not in ("euler", "heun"):
            raise ValueError(f"scheme must be 'euler', 'heun' or 'mala', not {a['scheme']!r}")
        if a["momenta"]:
            raise ValueError("flow=True does not run with momenta=True (use flowed() between calls)")
        if a["scheme"] == "heun":
            raise ValueError("step(flow=True) does not run with scheme='heun' (use step_flow(..., scheme='heun'))")
        return self.step_flow(a["n"], a["every"], correlate=a["correlate"])
    return wrapper


def _frames_accept_flow(run_frames):
    """`Phi4Ensemble.run_frames` with the keyword-only `flow`, made as
    `_accepts_flow` makes `step`'s: flow=True hands the call to
    `run_frames_flow` (`measure` is ignored: the series is always returned)
    after refusing momenta=True; the signature introspection reports stays
    that of `run_frames` itself."""
    sig = inspect.signature(run_frames)

    @functools.wraps(run_frames)
    def wrapper(self, *args, flow=False, **kw):
        if not flow:
            return run_frames(self, *args, **kw)
        a = sig.bind(self, *args, **kw)
        a.apply_defaults()
        a = a.arguments
        _refuse_hmc(a["scheme"], "run_frames")
        if a["scheme"] == "mala":
            raise ValueError(_MALA_NO_FRAMES)
        if a["scheme"] not in ("euler", "heun"):
            raise ValueError(f"scheme must be 'euler' or 'heun', not {a['scheme']!r}")
        if a["momenta"]:
            raise ValueError("flow=True does not run with momenta=True (use flowed() between calls)")
        return self.run_frames_flow(a["n"], correlate=a["correlate"], scheme=a["scheme"])
    return wrapper


class Phi4Ensemble:
    """`replicas` independent periodic φ⁴ lattices of one shape (Lx, Ly, Lz),
    each with its own seed, Δτ, m², λ and C, advanced together: one launch per
    `step` call, one work-group per lattice, the lattice on-chip for every step
    of the call (sq_phi4_ens_*).  Replica r is bit for bit the `Phi4Lattice`
    (comm="none") of the same shape, parameters, seed, step counter and start
    field.  Lx in {8, 16, 32, 64}, Ly, Lz >= 2, at most 32,768 sites.  Raw
    steps (`step`) or whole frames (`run_frames`): `loops` steps, the stability
    rule, the rollback and, with `adapt_dtau`, the Δτ controller, decided per
    replica inside the kernel, one launch per call, as `Phi4Lattice.run_frames`
    decides them for one lattice.  Both can measure, in flight, the time-slice
    correlator over z at zero momentum (`correlate`) and at up to eight spatial
    momenta set with `set_momenta` (`momenta`).  With `set_flow`, `step`,
    `step_flow` and `run_frames` can also flow a copy of every field (the
    noise-off update, a gradient flow) and measure the smoothed copies at up
    to four flow levels (`flow`).

    dtau, m2, lam and C are scalars or length-R sequences; seeds defaults to
    seed + r."""

    def __init__(self, shape, replicas, dtau=0.01, m2=1.0, lam=1.0, C=1.0, seeds=None, seed=0x5EED, clamp=1000.0,
                 device=0, loops=100, adapt_dtau=True):
        R = int(replicas)
        per = [np.asarray(v, dtype=np.float64) for v in (dtau, m2, lam, C)]
        for v in per:
            if v.ndim > 1 or (v.ndim == 1 and v.shape != (R,)):
                raise ValueError("dtau, m2, lam and C are scalars or have one entry per replica")
        p = _lib.default_params()
        p.model = SQ_MODEL_PHI4
        for i in range(3):
            p.dims[i] = int(shape[i])
        # the create call checks the parameters it is given: replica 0's, the others' arrive through set_params
        p.deltatau, p.m2, p.lambda_, p.C = (float(v.reshape(-1)[0]) for v in per)
        p.seed = int(seed)
        p.clamp = float(clamp)
        p.device = int(device)
        p.comm = SQ_COMM_NONE
        p.loops = int(loops)
        p.adapt_dtau = 1 if adapt_dtau else 0
        self._frames_run = False
        self._h = ctypes.c_void_p()
        sp = None
        if seeds is not None:
            s = np.ascontiguousarray(seeds, dtype=np.uint64)
            if s.shape != (R,):
                raise ValueError("seeds must have one entry per replica")
            sp = s.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong))
        _lib.call("sq_phi4_ens_create", ctypes.byref(p), R, sp, ctypes.byref(self._h))
        self.params = p
        self.shape = tuple(int(s) for s in shape)
        self.R = R
        if any(v.ndim == 1 for v in per):
            try:
                self.set_params(*per)
            except Exception:
                self.close()
                raise

    @staticmethod
    def shape_info(shape):
        """The work-group shape the launchers give a lattice of `shape`
        (sq_phi4_ens_shape_info; no device needed): {"K": float4 quads per lane,
        "T": lanes, "images" / "lds_bytes": LDS images and dynamic LDS bytes of
        the step launch, "frames_images" / "frames_lds_bytes": of the frames
        launch, "moments_lds_bytes", "lds_limit"}.  Raises StochQuantError
        (SQ_E_ARG) for a shape the constructor refuses."""
        dims = (ctypes.c_int * 3)(*(int(s) for s in shape))
        out = (ctypes.c_int * 8)()
        _lib.call("sq_phi4_ens_shape_info", dims, out)
        return dict(zip(("K", "T", "images", "lds_bytes", "frames_images", "frames_lds_bytes", "moments_lds_bytes",
                         "lds_limit"), (int(v) for v in out)))

    def close(self):
        if self._h:
            _lib.call("sq_phi4_ens_destroy", self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def lattice_shape(self):
        return (self.shape[2], self.shape[1], self.shape[0])  # numpy order: z, y, x

    def _count(self, first, count):
        return self.R - int(first) if count is None else int(count)

    def upload(self, phi, first=0):
        """Fields of replicas first .. first + k: an array of one lattice's shape
        (Lz, Ly, Lx) goes to every replica from `first`, (k, Lz, Ly, Lx) to k replicas."""
        a = np.asarray(phi, dtype=np.float32)
        ls = self.lattice_shape
        if a.shape == ls:
            a = np.broadcast_to(a, (max(self.R - int(first), 0),) + ls)
        if a.ndim != 4 or a.shape[1:] != ls:
            raise ValueError(f"fields must have shape {ls} or (k,) + {ls}")
        a = np.ascontiguousarray(a)
        _lib.call("sq_phi4_ens_upload", self._h, int(first), a.shape[0], _fptr(a))

    def download(self, first=0, count=None):
        k = self._count(first, count)
        a = np.empty((max(k, 0),) + self.lattice_shape, dtype=np.float32)
        _lib.call("sq_phi4_ens_download", self._h, int(first), k, _fptr(a))
        return a

    def init_field(self, amp):
        """Replica r: the `Phi4Lattice.init_field(amp)` of its seed."""
        _lib.call("sq_phi4_ens_init_field", self._h, float(amp))

    def set_params(self, dtau=None, m2=None, lam=None, C=None, first=0, count=None):
        """Per-replica parameters of replicas first .. first + count (scalars or
        `count` entries; None leaves a parameter alone).  Raises, changing
        nothing, when a replica would break the context's parameter bound."""
        k = self._count(first, count)
        arrs = [None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.float64),
                                                                           (max(k, 0),)))
                for v in (dtau, m2, lam, C)]
        _lib.call("sq_phi4_ens_set_params", self._h, int(first), k, *[None if a is None else _dptr(a) for a in arrs])

    def get_params(self, first=0, count=None):
        k = self._count(first, count)
        out = {n: np.empty(max(k, 0)) for n in ("dtau", "m2", "lam", "C")}
        _lib.call("sq_phi4_ens_get_params", self._h, int(first), k, *[_dptr(out[n]) for n in ("dtau", "m2", "lam", "C")])
        return out

    @property
    def dtau(self):
        return self.get_params()["dtau"]

    @dtau.setter
    def dtau(self, v):
        self.set_params(dtau=v)

    @property
    def step_counter(self):
        s = np.empty(self.R, dtype=np.uint64)
        _lib.call("sq_phi4_ens_get_step", self._h, 0, self.R, s.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)))
        return s

    @step_counter.setter
    def step_counter(self, v):
        s = np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype=np.uint64), (self.R,)))
        _lib.call("sq_phi4_ens_set_step", self._h, 0, self.R, s.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)))

    @_accepts_flow
    def step(self, n=1, every=0, correlate=False, momenta=False, scheme="euler"):
        """n steps of every replica in one launch.  every = k > 0: returns the
        (n // k, R, 4) array of S1 = Σφ, S2 = Σφ², S4 = Σφ⁴ and NN = Σ over
        sites and the three forward links of φ(x) φ(x + μ), recorded after each
        k-th step from the on-chip field; otherwise None.  `correlate` (needs
        every >= 1): the kernel also adds one time-slice correlator measurement
        after each k-th step to the replicas' accumulators (`corr_sums`,
        `correlator`); fields, counters, flags and the return value are those of
        the same call without it.  `momenta` (needs every >= 1 and
        `set_momenta`): likewise one measurement of the momentum-projected
        correlators (`pcorr_sums`, `pcorrelator`).

        scheme: "euler" (the default, first order in Δτ) or "heun", the
        second-order stochastic Heun step (sq_phi4_ens_step_heun): with E the
        Euler update at the step's counter, φ' = guard(0.5 (φ + E(E(φ)))), both
        applications with the same noise; the counter advances by one per Heun
        step, and `every`, `correlate` and `momenta` count and measure Heun
        steps.  Calls of either scheme may alternate.

        scheme="mala": the Metropolis-adjusted Langevin step, `step_mala(n,
        every, correlate)` (see there): the Euler update as a proposal, accepted
        or rejected per replica in the kernel, no step-size bias.  momenta=True
        and flow=True are refused with ValueError before any library call (use
        `pslices()` / `flowed()` between calls).

        The keyword-only flow=True (needs every >= 1 and `set_flow`; Euler steps,
        no momenta) is `step_flow(n, every, correlate)`: the measurements are
        taken of flowed copies of the fields, see there.  It is refused with
        ValueError, before any library call, with every < 1, momenta=True or
        scheme="heun": Heun steps with the flow are `step_flow(...,
        scheme="heun")`, which this keyword does not reach."""
        _refuse_hmc(scheme, "step")
        if scheme == "mala":
            if momenta:
                raise ValueError("scheme='mala' does not run with momenta=True (use pslices() between calls)")
            return self.step_mala(n, every, correlate=correlate)
        if scheme not in ("euler", "heun"):
            raise ValueError(f"scheme must be 'euler', 'heun' or 'mala', not {scheme!r}")
        n, every = int(n), int(every)
        fn, extra = "sq_phi4_ens_step", ()
        if correlate or momenta:
            if every < 1:
                raise ValueError("correlate=True and momenta=True need every >= 1")
            fn = "sq_phi4_ens_step_corr"
        if momenta:
            fn, extra = "sq_phi4_ens_step_pcorr", (1 if correlate else 0,)
        if scheme == "heun":
            fn, extra = "sq_phi4_ens_step_heun", ((1 if correlate else 0) | (2 if momenta else 0),)
        if every <= 0:
            _lib.call(fn, self._h, n, 0, None, *extra)
            return None
        ser = np.zeros((max(n, 0) // every, self.R, 4))
        _lib.call(fn, self._h, n, every, _dptr(ser) if ser.size else None, *extra)
        return ser

    def step_mala(self, n=1, every=0, correlate=False, record=False):
        """n Metropolis-adjusted Langevin (MALA) steps of every replica in one
        launch (sq_phi4_ens_step_mala; include/stochquant.h has the definition).
        Per step and replica the Euler update of `step` is a proposal p; the
        kernel forms dH = [2h (S(p) - S(φ)) + ½ (Σb² - Σa²)] / σ² in double from
        the two fields, draws one uniform u from the replica's Philox key, and
        the replica holds p when dH <= 0 or u < exp(-dH), else it keeps φ bit
        for bit.  The chain samples exp(-S / C²) with no Δτ bias; the counter
        advances by one per step whatever the verdict.  A proposal that reached
        the clamp is rejected and sets the replica's guard flag.

        every = k > 0: returns the (n // k, R, 4) sums of the field each
        replica holds after every k-th step's verdict, else None; `correlate`
        (needs every >= 1) adds one correlator measurement of that field per
        record, also after a rejected step.  record=True: returns (series,
        rec), rec the (n, R, 3) array of (dH, u, verdict) of every step, verdict
        0 rejected, 1 accepted, 2 guard trip.

        Use: thermalise with Euler or Heun steps first (from a cold field
        nothing is accepted), then choose Δτ by `mala_stats()`: the acceptance
        falls with the volume at fixed Δτ.  Every replica needs C != 0
        (StochQuantError otherwise).  Calls of the three schemes may alternate."""
        n, every = int(n), int(every)
        if correlate and every < 1:
            raise ValueError("correlate=True needs every >= 1")
        ser = np.zeros((max(n, 0) // every, self.R, 4)) if every > 0 else None
        rec = np.zeros((max(n, 0), self.R, 3)) if record else None
        _lib.call("sq_phi4_ens_step_mala", self._h, n, every,
                  _dptr(ser) if ser is not None and ser.size else None, 1 if correlate else 0,
                  _dptr(rec) if rec is not None and rec.size else None)
        return (ser, rec) if record else ser

    def mala_stats(self, first=0, count=None):
        """(count, 3) int64: MALA steps proposed, accepted and rejected by the
        guard, per replica, since creation or `mala_reset` (sq_phi4_ens_mala_stats)."""
        k = self._count(first, count)
        out = np.zeros((max(k, 0), 3), dtype=np.int64)
        _lib.call("sq_phi4_ens_mala_stats", self._h, int(first), k, out.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)))
        return out

    def mala_reset(self, first=0, count=None):
        """Clear the MALA counters of replicas first .. first + count."""
        _lib.call("sq_phi4_ens_mala_reset", self._h, int(first), self._count(first, count))

    def step_hmc(self, n=1, nleap=1, randomize=False, every=0, correlate=False, record=False):
        """n hybrid Monte Carlo (HMC) trajectories of every replica in one launch
        (sq_phi4_ens_step_hmc; include/stochquant.h has the definition).  Per
        trajectory and replica the momentum is drawn once -- the first leapfrog
        step is the Euler update of `step`, MALA's proposal --, L - 1 noise-free
        leapfrog steps of step length σ = C sqrt(2Δτ) follow in the kernel, and
        one Metropolis test on dH, formed in double from the two end fields,
        decides: the replica holds φ_L or keeps its field bit for bit.  The
        chain samples exp(-S / C²) with no Δτ bias and moves a distance L σ per
        test where MALA moves σ.  The counter advances by one per trajectory.
        nleap=1 is `step_mala` bit for bit.

        L = nleap, or with randomize=True uniform on 1 .. nleap per trajectory
        and replica, from the Philox block of the accept uniform.  A fixed
        length is non-ergodic where ω L σ nears a multiple of π for some mode
        (that mode returns to where it started): fixed lengths are for short
        trajectories and tests, randomize=True is for production.
        1 <= nleap <= 4096.

        every = k > 0: returns the (n // k, R, 4) sums of the field each
        replica holds after every k-th trajectory's verdict, else None;
        `correlate` (needs every >= 1) adds one correlator measurement of that
        field per record.  record=True: returns (series, rec), rec the (n, R, 4)
        array of (dH, u, verdict, L) of every trajectory, verdict 0 rejected, 1
        accepted, 2 guard trip (some field of the trajectory reached the clamp:
        rejected, the replica's guard flag set).

        Use as `step_mala`: thermalise first, choose Δτ and nleap by
        `hmc_stats()`; every replica needs C != 0 (StochQuantError otherwise).
        Calls of the four schemes may alternate."""
        n, nleap, every = int(n), int(nleap), int(every)
        if nleap < 1 or nleap > 4096:
            raise ValueError("step_hmc: nleap must lie in [1, 4096]")
        if correlate and every < 1:
            raise ValueError("step_hmc: correlate=True needs every >= 1")
        ser = np.zeros((max(n, 0) // every, self.R, 4)) if every > 0 else None
        rec = np.zeros((max(n, 0), self.R, 4)) if record else None
        _lib.call("sq_phi4_ens_step_hmc", self._h, n, nleap, 1 if randomize else 0, every,
                  _dptr(ser) if ser is not None and ser.size else None, 1 if correlate else 0,
                  _dptr(rec) if rec is not None and rec.size else None)
        return (ser, rec) if record else ser

    def hmc_stats(self, first=0, count=None):
        """(count, 4) int64: trajectories, accepted, rejected by the guard, and
        leapfrog steps, per replica, since creation or `hmc_reset`
        (sq_phi4_ens_hmc_stats).  The MALA counters are separate."""
        k = self._count(first, count)
        out = np.zeros((max(k, 0), 4), dtype=np.int64)
        _lib.call("sq_phi4_ens_hmc_stats", self._h, int(first), k, out.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)))
        return out

    def hmc_reset(self, first=0, count=None):
        """Clear the HMC counters of replicas first .. first + count."""
        _lib.call("sq_phi4_ens_hmc_reset", self._h, int(first), self._count(first, count))

    def set_ladder(self, n):
        """Cut the R replicas into R // n exchange ladders of n consecutive
        slots (sq_phi4_ens_set_ladder): 2 <= n <= R and R % n == 0; n = 0
        switches ladders off, the state at creation.  The rungs' parameters are
        what `set_params` gave the slots -- typically a ladder in C; the library
        neither orders nor checks them."""
        _lib.call("sq_phi4_ens_set_ladder", self._h, int(n))

    @property
    def ladder(self):
        n = ctypes.c_int(0)
        _lib.call("sq_phi4_ens_get_ladder", self._h, ctypes.byref(n))
        return n.value

    @property
    def exchange_round(self):
        x = ctypes.c_ulonglong(0)
        _lib.call("sq_phi4_ens_exchange_round", self._h, ctypes.byref(x))
        return x.value

    @exchange_round.setter
    def exchange_round(self, v):
        _lib.call("sq_phi4_ens_set_exchange_round", self._h, ctypes.c_ulonglong(int(v)))

    def exchange(self, rounds=1, record=False):
        """`rounds` replica-exchange rounds on the device, back to back
        (sq_phi4_ens_exchange; include/stochquant.h has the definition).  Round
        x pairs slots (l n + o + 2j, + 1), o = x & 1, inside every ladder; per
        pair one work-group forms Δ = E_a(φ_b) + E_b(φ_a) - E_a(φ_a) - E_b(φ_b),
        E_r = S_r / C_r², in double from the fields' sums, accepts when Δ <= 0
        or u < exp(-Δ), and on acceptance swaps the two rows of the field array
        and the two walker labels.  Parameters, counters, flags and every
        accumulator stay with the slot.  `exchange_round` advances by one per
        round.  record=True: returns the (rounds, R, 5) array of (Δ, u, verdict,
        partner, walker after the round); a slot without a partner in a round
        has verdict -1, partner -1.

        Needs `set_ladder` and C != 0 in every replica (StochQuantError
        otherwise).  The test is meaningful between equilibrium fields only:
        after `step_mala` / `step_hmc`, or Euler / Heun steps up to their Δτ
        bias."""
        rounds = int(rounds)
        rec = np.zeros((max(rounds, 0), self.R, 5)) if record else None
        _lib.call("sq_phi4_ens_exchange", self._h, rounds, _dptr(rec) if rec is not None and rec.size else None)
        return rec

    def step_hmc_exchange(self, rounds, ntraj=1, nleap=1, randomize=False, every=0, correlate=False, record=False):
        """`rounds` times: `step_hmc(ntraj, nleap, randomize, every, correlate)`,
        then one `exchange` round -- all launches enqueued back to back with one
        synchronisation at the end (sq_phi4_ens_step_hmc_exchange).  Bit for bit
        the loop of the separate calls in everything.  every = k > 0 needs
        ntraj % k == 0 and returns the (rounds * ntraj // k, R, 4) sums, taken
        of the field a slot holds after its trajectory and before the round's
        exchange; else None.  record=True: returns (series, rec_hmc, rec_x),
        the (rounds * ntraj, R, 4) trajectory records of `step_hmc` and the
        (rounds, R, 5) records of `exchange`.  nleap=1 is MALA with exchange."""
        rounds, ntraj, nleap, every = int(rounds), int(ntraj), int(nleap), int(every)
        if nleap < 1 or nleap > 4096:
            raise ValueError("step_hmc_exchange: nleap must lie in [1, 4096]")
        if correlate and every < 1:
            raise ValueError("step_hmc_exchange: correlate=True needs every >= 1")
        if every > 0 and ntraj % every != 0:
            raise ValueError("step_hmc_exchange: every must divide ntraj")
        nr, nj = max(rounds, 0), max(ntraj, 0)
        ser = np.zeros((nr * (nj // every), self.R, 4)) if every > 0 else None
        rh = np.zeros((nr * nj, self.R, 4)) if record else None
        rx = np.zeros((nr, self.R, 5)) if record else None
        _lib.call("sq_phi4_ens_step_hmc_exchange", self._h, rounds, ntraj, nleap, 1 if randomize else 0, every,
                  _dptr(ser) if ser is not None and ser.size else None, 1 if correlate else 0,
                  _dptr(rh) if rh is not None and rh.size else None,
                  _dptr(rx) if rx is not None and rx.size else None)
        return (ser, rh, rx) if record else ser

    def exchange_stats(self, first=0, count=None):
        """(count, 2) int64: attempts and acceptances of the pair (r, r + 1),
        stored at r, since creation or `exchange_reset`
        (sq_phi4_ens_exchange_stats)."""
        k = self._count(first, count)
        out = np.zeros((max(k, 0), 2), dtype=np.int64)
        _lib.call("sq_phi4_ens_exchange_stats", self._h, int(first), k,
                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)))
        return out

    def walkers(self, first=0, count=None):
        """(count,) int32: the walker label each slot holds -- the slot its
        field started in, carried along by every accepted exchange."""
        k = self._count(first, count)
        out = np.zeros(max(k, 0), dtype=np.int32)
        _lib.call("sq_phi4_ens_walkers", self._h, int(first), k, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        return out

    def exchange_reset(self, first=0, count=None, walkers=False):
        """Clear the exchange counters of replicas first .. first + count;
        walkers=True also sets their labels back to the slot index."""
        _lib.call("sq_phi4_ens_exchange_reset", self._h, int(first), self._count(first, count), 1 if walkers else 0)

    @staticmethod
    def exchange_shape_info(shape):
        """What the exchange launch asks for, without a device: K quads per
        lane, T lanes, dynamic LDS bytes and the LDS limit -- the moments
        launch's shape, one work-group per pair."""
        dims = (ctypes.c_int * 3)(*(int(s) for s in shape))
        out = (ctypes.c_int * 4)()
        _lib.call("sq_phi4_ens_exchange_shape_info", dims, out)
        return dict(zip(("K", "T", "lds_bytes", "lds_limit"), (int(v) for v in out)))

    @property
    def cluster_sweep(self):
        c = ctypes.c_ulonglong(0)
        _lib.call("sq_phi4_ens_cluster_sweep", self._h, ctypes.byref(c))
        return c.value

    @cluster_sweep.setter
    def cluster_sweep(self, v):
        _lib.call("sq_phi4_ens_set_cluster_sweep", self._h, ctypes.c_ulonglong(int(v)))

    def _cluster_records(self, n, record):
        sites = self.shape[0] * self.shape[1] * self.shape[2]
        if not record:
            return None, None
        return np.zeros((n, self.R, sites), dtype=np.uint8), np.zeros((n, self.R, sites), dtype=np.int32)

    def cluster(self, sweeps=1, record=False):
        """`sweeps` Swendsen-Wang cluster sweeps of every replica on the device,
        back to back (sq_phi4_ens_cluster; include/stochquant.h has the
        definition).  The embedded-Ising update of Brower and Tamayo: φ = s|φ|
        with |φ| frozen, every forward bond between sites of one sign switched
        on with probability 1 - exp(-2β φ_i φ_j), β = 1 / C², the clusters of
        the on-bonds labelled by their smallest site index, and every cluster's
        sign flipped with probability ½ -- all from the replica's Philox key at
        the counter `cluster_sweep`, which advances by one per sweep.  Only
        sign bits of the fields change; parameters, counters, flags, walkers
        and every accumulator stay.  record=True: returns (bonds, labels), the
        (sweeps, R, sites) uint8 array of the sites' forward bonds (bits 0, 1,
        2 = x, y, z) and the (sweeps, R, sites) int32 array of their cluster
        labels; else None.

        The sweep is exact for exp(-S / C²), the density `step_mala` and
        `step_hmc` sample, but alone it is not ergodic (|φ| never moves):
        alternate it with trajectories on thermalised fields
        (`step_hmc_cluster`).  Every replica needs C != 0 (StochQuantError
        otherwise)."""
        sweeps = int(sweeps)
        bonds, labels = self._cluster_records(max(sweeps, 0), record)
        _lib.call("sq_phi4_ens_cluster", self._h, sweeps,
                  bonds.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)) if record and bonds.size else None,
                  labels.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if record and labels.size else None)
        return (bonds, labels) if record else None

    def step_hmc_cluster(self, rounds, ntraj=1, nleap=1, randomize=False, every=0, correlate=False, record=False):
        """`rounds` times: `step_hmc(ntraj, nleap, randomize, every, correlate)`,
        then one `cluster` sweep -- all launches enqueued back to back with one
        synchronisation at the end (sq_phi4_ens_step_hmc_cluster).  Bit for bit
        the loop of the separate calls in everything.  every = k > 0 needs
        ntraj % k == 0 and returns the (rounds * ntraj // k, R, 4) sums, taken
        of the field a replica holds after its trajectory and before the
        round's sweep; else None.  record=True: returns (series, rec_hmc,
        bonds, labels), the (rounds * ntraj, R, 4) trajectory records of
        `step_hmc` and the (rounds, R, sites) records of `cluster`.  nleap=1 is
        MALA with cluster sweeps."""
        rounds, ntraj, nleap, every = int(rounds), int(ntraj), int(nleap), int(every)
        if nleap < 1 or nleap > 4096:
            raise ValueError("step_hmc_cluster: nleap must lie in [1, 4096]")
        if correlate and every < 1:
            raise ValueError("step_hmc_cluster: correlate=True needs every >= 1")
        if every > 0 and ntraj % every != 0:
            raise ValueError("step_hmc_cluster: every must divide ntraj")
        nr, nj = max(rounds, 0), max(ntraj, 0)
        ser = np.zeros((nr * (nj // every), self.R, 4)) if every > 0 else None
        rh = np.zeros((nr * nj, self.R, 4)) if record else None
        bonds, labels = self._cluster_records(nr, record)
        _lib.call("sq_phi4_ens_step_hmc_cluster", self._h, rounds, ntraj, nleap, 1 if randomize else 0, every,
                  _dptr(ser) if ser is not None and ser.size else None, 1 if correlate else 0,
                  _dptr(rh) if rh is not None and rh.size else None,
                  bonds.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)) if record and bonds.size else None,
                  labels.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if record and labels.size else None)
        return (ser, rh, bonds, labels) if record else ser

    def _cluster_weights(self, n, record):
        sites = self.shape[0] * self.shape[1] * self.shape[2]
        return np.zeros((n, self.R, sites, 7), dtype=np.int64) if record else None

    def cluster_improved(self, sweeps=1, record=False):
        """`cluster(sweeps)` with the cluster sums of the improved estimators
        (sq_phi4_ensemble_cluster_improved; include/stochquant.h has the
        definition): fields, counters and statistics are bit for bit those of
        `cluster`.  Returns the (sweeps, R, 8) series I2, I4, F_x, F_y, F_z,
        Mmax, Mtot, nsat per replica and sweep: with M_C = Σ_{i∈C} |φ_i|,
        I2 = Σ_C M_C² and I4 = Σ_C M_C⁴ give ⟨(Σφ)²⟩ = ⟨I2⟩ and ⟨(Σφ)⁴⟩ =
        ⟨3 I2² − 2 I4⟩, and F_µ = Σ_C |Σ_{i∈C} |φ_i| e^{ip·x_i}|² at the unit
        momentum of axis µ gives ⟨|Σφ e^{ip·x}|²⟩ (`cluster_observables` turns
        the series into χ, the Binder cumulant and ξ_2nd).  Sites with |φ| ≥
        2¹⁵, ∞ or NaN weigh nothing and are counted in nsat.  record=True:
        returns (series, bonds, labels, weights), weights the (sweeps, R,
        sites, 7) int64 sums M, A_x, B_x, A_y, B_y, A_z, B_z (fixed point, 32
        fractional bits) at each cluster's root, 0 elsewhere.

        A call of its own rather than a keyword of `cluster`: the signatures
        of `cluster` and `step_hmc_cluster` are pinned by their tests."""
        sweeps = int(sweeps)
        n = max(sweeps, 0)
        ser = np.zeros((n, self.R, 8))
        bonds, labels = self._cluster_records(n, record)
        weights = self._cluster_weights(n, record)
        _lib.call("sq_phi4_ensemble_cluster_improved", self._h, sweeps, _dptr(ser) if ser.size else None,
                  bonds.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)) if record and bonds.size else None,
                  labels.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if record and labels.size else None,
                  weights.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)) if record and weights.size else None)
        return (ser, bonds, labels, weights) if record else ser

    def step_hmc_cluster_improved(self, rounds, ntraj=1, nleap=1, randomize=False, every=0, correlate=False,
                                  record=False):
        """`step_hmc_cluster` with every round's sweep a `cluster_improved`
        sweep (sq_phi4_ensemble_step_hmc_cluster_improved), bit for bit the loop of
        `step_hmc` and `cluster_improved(1)`.  Returns (series, cseries), series
        as `step_hmc_cluster` returns it (None without `every`) and cseries the
        (rounds, R, 8) cluster series; record=True: (series, rec_hmc, bonds,
        labels, cseries, weights)."""
        rounds, ntraj, nleap, every = int(rounds), int(ntraj), int(nleap), int(every)
        if nleap < 1 or nleap > 4096:
            raise ValueError("step_hmc_cluster_improved: nleap must lie in [1, 4096]")
        if correlate and every < 1:
            raise ValueError("step_hmc_cluster_improved: correlate=True needs every >= 1")
        if every > 0 and ntraj % every != 0:
            raise ValueError("step_hmc_cluster_improved: every must divide ntraj")
        nr, nj = max(rounds, 0), max(ntraj, 0)
        ser = np.zeros((nr * (nj // every), self.R, 4)) if every > 0 else None
        rh = np.zeros((nr * nj, self.R, 4)) if record else None
        cser = np.zeros((nr, self.R, 8))
        bonds, labels = self._cluster_records(nr, record)
        weights = self._cluster_weights(nr, record)
        _lib.call("sq_phi4_ensemble_step_hmc_cluster_improved", self._h, rounds, ntraj, nleap, 1 if randomize else 0, every,
                  _dptr(ser) if ser is not None and ser.size else None, 1 if correlate else 0,
                  _dptr(rh) if rh is not None and rh.size else None,
                  bonds.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)) if record and bonds.size else None,
                  labels.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if record and labels.size else None,
                  _dptr(cser) if cser.size else None,
                  weights.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)) if record and weights.size else None)
        return (ser, rh, bonds, labels, cser, weights) if record else (ser, cser)

    @staticmethod
    def cluster_observables(cseries, shape, axis_mask=None):
        """The finite-size-scaling observables of a (sweeps, R, 8) cluster
        series of lattices of `shape`, over sweeps and replicas, each as
        (value, standard error): "chi" = ⟨M²⟩ / V from I2, "binder" = 1 −
        ⟨M⁴⟩ / (3 ⟨M²⟩²) with ⟨M⁴⟩ = ⟨3 I2² − 2 I4⟩, and "xi" = one pair per
        axis of `axis_mask` (default: all three), ξ_2nd = sqrt((⟨I2⟩ / ⟨F_µ⟩ −
        1) / (4 sin²(π / L_µ))).  The errors come from the scatter of the
        replicas (a jackknife over them: the plain standard error of the
        replica means for χ); they need R ≥ 2.  Unconverged sweeps (nsat < 0)
        are left out."""
        s = np.asarray(cseries, dtype=np.float64)
        if s.ndim != 3 or s.shape[2] != 8 or s.shape[1] < 2 or s.shape[0] < 1:
            raise ValueError("cluster_observables: a (sweeps >= 1, R >= 2, 8) series is needed")
        mask = [True] * 3 if axis_mask is None else [bool(m) for m in axis_mask]
        if len(mask) != 3:
            raise ValueError("cluster_observables: axis_mask holds one entry per axis x, y, z")
        ok = s[:, :, 7] >= 0
        if not ok.any(axis=0).all():
            raise ValueError("cluster_observables: a replica has no converged sweep")
        w = ok / ok.sum(axis=0, keepdims=True)
        q = np.stack([s[:, :, 0], 3.0 * s[:, :, 0] ** 2 - 2.0 * s[:, :, 1], s[:, :, 2], s[:, :, 3], s[:, :, 4]], axis=2)
        per = (q * w[:, :, None]).sum(axis=0)               # (R, 5) replica means
        V = float(shape[0] * shape[1] * shape[2])

        def f(m):
            out = [m[0] / V, 1.0 - m[1] / (3.0 * m[0] * m[0])]
            for mu in range(3):
                if mask[mu]:
                    x = (m[0] / m[2 + mu] - 1.0) / (4.0 * np.sin(np.pi / shape[mu]) ** 2)
                    out.append(np.sqrt(x) if x >= 0 else np.nan)
            return np.asarray(out)

        R = per.shape[0]
        full = f(per.mean(axis=0))
        jk = np.stack([f((per.sum(axis=0) - per[r]) / (R - 1)) for r in range(R)])
        err = np.sqrt((R - 1) / R * ((jk - jk.mean(axis=0)) ** 2).sum(axis=0))
        pairs = [(float(v), float(e)) for v, e in zip(full, err)]
        return {"chi": pairs[0], "binder": pairs[1], "xi": pairs[2:]}

    @staticmethod
    def cluster_improved_shape_info(shape):
        """What the sweep with the cluster sums asks for, without a device: K, T,
        dynamic LDS bytes, the LDS limit, and "park": 1 where a lane's labels
        wait in device memory while the LDS image serves as the accumulators
        (K = 8), 0 where they wait in registers."""
        dims = (ctypes.c_int * 3)(*(int(s) for s in shape))
        out = (ctypes.c_int * 5)()
        _lib.call("sq_phi4_ensemble_cluster_improved_shape_info", dims, out)
        return dict(zip(("K", "T", "lds_bytes", "lds_limit", "park"), (int(v) for v in out)))

    def cluster_stats(self, first=0, count=None):
        """(count, 5) int64: sweeps, clusters, flipped clusters, flipped sites
        and unconverged sweeps (always 0: the labelling's pass bound is its
        worst case) per replica, since creation or `cluster_reset`
        (sq_phi4_ens_cluster_stats)."""
        k = self._count(first, count)
        out = np.zeros((max(k, 0), 5), dtype=np.int64)
        _lib.call("sq_phi4_ens_cluster_stats", self._h, int(first), k,
                  out.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)))
        return out

    def cluster_reset(self, first=0, count=None):
        """Clear the cluster counters of replicas first .. first + count."""
        _lib.call("sq_phi4_ens_cluster_reset", self._h, int(first), self._count(first, count))

    @staticmethod
    def cluster_shape_info(shape):
        """What the cluster sweep's launch asks for, without a device: K quads
        per lane, T lanes, dynamic LDS bytes and the LDS limit -- the moments
        launch's shape, one work-group per replica."""
        dims = (ctypes.c_int * 3)(*(int(s) for s in shape))
        out = (ctypes.c_int * 4)()
        _lib.call("sq_phi4_ens_cluster_shape_info", dims, out)
        return dict(zip(("K", "T", "lds_bytes", "lds_limit"), (int(v) for v in out)))

    def step_flow(self, n=1, every=1, correlate=False, scheme="euler"):
        """n steps of every replica in one launch, as `step`, with a flow
        measurement after each every-th step (every >= 1, `set_flow` first;
        sq_phi4_ens_step_flow, with scheme="heun" sq_phi4_ens_step_flow_heun:
        every step the Heun step): the kernel flows a copy of every field and
        measures at each of the F flow levels.  Returns the (n // every, F, R, 4)
        array of the flowed fields' sums; `correlate` adds one correlator
        measurement per level to the FLOW accumulators (`fcorr_sums`,
        `fcorrelator`), not to the plain ones.  Fields, counters and flags are
        those of `step(n, scheme=scheme)`.  `step(n, every=k, flow=True,
        correlate=...)` is this call with Euler steps; scheme="heun" is reached
        here only (`step` refuses it with flow=True)."""
        _refuse_hmc(scheme, "step_flow")
        if scheme == "mala":
            raise ValueError("scheme='mala' does not run with the flow (use flowed() between calls)")
        if scheme not in ("euler", "heun"):
            raise ValueError(f"scheme must be 'euler' or 'heun', not {scheme!r}")
        n, every = int(n), int(every)
        if every < 1:
            raise ValueError("a flow measurement needs every >= 1")
        ser = np.zeros((max(n, 0) // every, self._flow_levels(), self.R, 4))
        _lib.call("sq_phi4_ens_step_flow_heun" if scheme == "heun" else "sq_phi4_ens_step_flow", self._h, n, every,
                  _dptr(ser) if ser.size else None, 1 if correlate else 0)
        return ser

    def run_frames_flow(self, n, correlate=False, scheme="euler"):
        """n frames of every replica in one launch, as `run_frames(n,
        scheme=scheme)`, with a flow measurement behind every frame's verdict
        (`set_flow` first; sq_phi4_ens_run_frames_flow): (stable (n, R) bool,
        dtau (n, R), series (n, F, R, 4)).  series[f] holds the F flow levels'
        sums of the field each replica holds after frame f, the adopted field
        after a stable frame, the frame's start field again after a rollback;
        with level 0 among the levels that row is `run_frames(n,
        measure=True)`'s series.  `correlate`: one correlator measurement per
        level after every stable frame of a replica, added to the FLOW
        accumulators (`fcorr_sums`, `fcorrelator`); a rolled-back frame adds
        nothing.  Verdicts, dtau, fields, counters, flags and the stability
        records are those of the call without the flow.  `run_frames(n,
        flow=True, ...)` is this call."""
        _refuse_hmc(scheme, "run_frames_flow")
        if scheme == "mala":
            raise ValueError(_MALA_NO_FRAMES)
        if scheme not in ("euler", "heun"):
            raise ValueError(f"scheme must be 'euler' or 'heun', not {scheme!r}")
        n = int(n)
        st = np.zeros((max(n, 0), self.R), dtype=np.int32)
        dt = np.zeros((max(n, 0), self.R))
        ser = np.zeros((max(n, 0), self._flow_levels(), self.R, 4))
        _lib.call("sq_phi4_ens_run_frames_flow", self._h, n, st.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _dptr(dt),
                  _dptr(ser) if ser.size else None, 1 if correlate else 0, 1 if scheme == "heun" else 0)
        if n > 0:
            self._frames_run = True
        return st != 0, dt, ser

    @staticmethod
    def frames_flow_shape_info(shape):
        """The LDS layout of the flow launches in frames and Heun steps for a
        lattice of `shape` (sq_phi4_ens_frames_flow_shape_info; no device
        needed): {"images" / "lds_bytes" of run_frames_flow without the
        correlator (either scheme), "corr_images" / "corr_lds_bytes" with it,
        "heun_step_images" / "heun_step_corr_images" / "heun_step_corr_lds_bytes"
        of step_flow(scheme="heun"), "stash", "heun_stash", "heun_step_stash":
        where the un-flowed field waits in Euler frames, Heun frames and Heun
        steps (0 = registers, 1 = device memory), "mask": bit 2 * (scheme ==
        "heun") + correlate set when run_frames_flow runs that combination on
        the shape}."""
        dims = (ctypes.c_int * 3)(*(int(s) for s in shape))
        out = (ctypes.c_int * 8)()
        _lib.call("sq_phi4_ens_frames_flow_shape_info", dims, out)
        o = [int(v) for v in out]
        return {"images": o[0], "lds_bytes": o[1], "corr_images": o[2], "corr_lds_bytes": o[3],
                "heun_step_images": o[4] & 0xff, "heun_step_corr_images": o[4] >> 8, "heun_step_corr_lds_bytes": o[5],
                "stash": o[6] & 1, "heun_stash": (o[6] >> 1) & 1, "heun_step_stash": (o[6] >> 2) & 1, "mask": o[7]}

    @_frames_accept_flow
    def run_frames(self, n, measure=False, correlate=False, momenta=False, scheme="euler"):
        """n frames of every replica in one launch: (stable (n, R) bool, dtau
        (n, R) after each frame), and with `measure` the (n, R, 4) sums S1, S2,
        S4, NN of each replica's field after the frame's verdict (the frame's
        start field again after a rollback).  `correlate`: one correlator
        measurement of the adopted field after every stable frame of a replica
        (a rolled-back frame measures nothing); the return values are unchanged.
        `momenta`: likewise one measurement of the momentum-projected correlators.

        scheme: "euler" (the default) or "heun": every step of the frame is the
        Heun step of `step(scheme="heun")` (sq_phi4_ens_run_frames_heun), the
        stability record taken of φ' against the step's input; the rule, the
        rollback, the controller and the measurements are the same, and T, V,
        Δτ and the counters are shared with the Euler frames.  Calls of either
        scheme, and raw steps, may alternate.

        The keyword-only flow=True (needs `set_flow`) is `run_frames_flow(n,
        correlate, scheme)`: `measure` is ignored, the (n, F, R, 4) series of
        the flowed fields' sums is always returned, and `correlate` feeds the
        flow accumulators.  momenta=True is refused with ValueError before any
        library call.  scheme="mala" is refused likewise: frames have no
        meaning under an accept/reject step."""
        _refuse_hmc(scheme, "run_frames")
        if scheme == "mala":
            raise ValueError(_MALA_NO_FRAMES)
        if scheme not in ("euler", "heun"):
            raise ValueError(f"scheme must be 'euler' or 'heun', not {scheme!r}")
        n = int(n)
        st = np.zeros((max(n, 0), self.R), dtype=np.int32)
        dt = np.zeros((max(n, 0), self.R))
        ser = np.zeros((max(n, 0), self.R, 4)) if measure else None
        fn, extra = ("sq_phi4_ens_run_frames_corr" if correlate else "sq_phi4_ens_run_frames"), ()
        if momenta:
            fn, extra = "sq_phi4_ens_run_frames_pcorr", (1 if correlate else 0,)
        if scheme == "heun":
            fn, extra = "sq_phi4_ens_run_frames_heun", ((1 if correlate else 0) | (2 if momenta else 0),)
        _lib.call(fn, self._h, n, st.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _dptr(dt),
                  None if ser is None else _dptr(ser), *extra)
        if n > 0:
            self._frames_run = True
        return (st != 0, dt) if ser is None else (st != 0, dt, ser)

    def run_frame(self, scheme="euler"):
        """One frame of every replica; (R,) bool: stable."""
        _refuse_hmc(scheme, "run_frame")
        return self.run_frames(1, scheme=scheme)[0][0]

    @staticmethod
    def heun_frames_shape_info(shape):
        """The Heun frames launch for a lattice of `shape`
        (sq_phi4_ens_heun_frames_shape_info; no device needed): {"images" /
        "lds_bytes" of the plain launch, "measure_mask": bit m set when the
        shape runs correlate / momenta = bit 0 / bit 1 of m}."""
        dims = (ctypes.c_int * 3)(*(int(s) for s in shape))
        out = (ctypes.c_int * 4)()
        _lib.call("sq_phi4_ens_heun_frames_shape_info", dims, out)
        return {"images": int(out[0]), "lds_bytes": int(out[1]), "measure_mask": int(out[2])}

    def stability(self, first=0, count=None, n=None):
        """The stability rule's state per replica: {"T", "V", "fired" (step of the
        last frame it fired at, -1 none): (count,) arrays; "M", "D", "A": (count,
        n) per-step records of the last frame, valid through the firing step}.
        n defaults to `loops` once a frame has run."""
        k = self._count(first, count)
        n = (self.params.loops if self._frames_run else 0) if n is None else int(n)
        tv = np.zeros((max(k, 0), 2))
        fired = np.zeros(max(k, 0), dtype=np.int32)
        M, D, A = (np.zeros((max(k, 0), max(n, 0)), dtype=np.float32) for _ in range(3))
        _lib.call("sq_phi4_ens_stability", self._h, int(first), k, _dptr(tv),
                  fired.ctypes.data_as(ctypes.POINTER(ctypes.c_int)), _fptr(M), _fptr(D), _fptr(A), n)
        return {"T": tv[:, 0].copy(), "V": tv[:, 1].copy(), "fired": fired, "M": M, "D": D, "A": A}

    def set_stability(self, T, V, first=0, count=None):
        """Set the carried T and V (scalars or `count` entries) and mark the replicas initialised."""
        k = self._count(first, count)
        t, v = (np.ascontiguousarray(np.broadcast_to(np.asarray(x, dtype=np.float64), (max(k, 0),))) for x in (T, V))
        _lib.call("sq_phi4_ens_set_stability", self._h, int(first), k, _dptr(t), _dptr(v))

    def moments(self, first=0, count=None):
        """{"S1", "S2", "S4", "NN", "maxabs"}: (count,) arrays of the current fields' sums."""
        k = self._count(first, count)
        out = np.empty((max(k, 0), 5))
        _lib.call("sq_phi4_ens_moments", self._h, int(first), k, _dptr(out))
        return {n: out[:, i].copy() for i, n in enumerate(("S1", "S2", "S4", "NN", "maxabs"))}

    @property
    def nt(self):
        """Correlator distances kept: t = 0 .. Lz // 2."""
        return self.shape[2] // 2 + 1

    def corr_sums(self, first=0, count=None):
        """The raw correlator accumulators of replicas first .. first + count:
        (G (count, nt) = Σ over measurements of g(t) = Σ_z S(z) S((z + t) mod Lz),
        S1 (count,) = Σ of Σ_z S(z), nmeas (count,) int64), S(z) the slice sums
        Σ_{x,y} φ; see include/stochquant.h for the summation order."""
        k = self._count(first, count)
        G = np.zeros((max(k, 0), self.nt))
        S1 = np.zeros(max(k, 0))
        nm = np.zeros(max(k, 0), dtype=np.int64)
        _lib.call("sq_phi4_ens_corr_sums", self._h, int(first), k, _dptr(G), _dptr(S1),
                  nm.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)))
        return G, S1, nm

    def corr_reset(self, first=0, count=None):
        """Zero the correlator accumulators of replicas first .. first + count (nothing else clears them)."""
        _lib.call("sq_phi4_ens_corr_reset", self._h, int(first), self._count(first, count))

    def slices(self, first=0, count=None):
        """One correlator measurement of the current fields, accumulating
        nothing: (S (count, Lz) slice sums, g (count, nt))."""
        k = self._count(first, count)
        S = np.zeros((max(k, 0), self.shape[2]))
        g = np.zeros((max(k, 0), self.nt))
        _lib.call("sq_phi4_ens_slices", self._h, int(first), k, _dptr(S), _dptr(g))
        return S, g

    def correlator(self, n=None, connected=True):
        """(mean (n,), err (n,), used): over the replicas with at least one
        measurement, in index order, the mean of c_r(t) = G_r(t) / (nmeas_r V)
        (minus (S1_r / nmeas_r)² / (Lz V) when `connected`) and its standard
        error sqrt(Σ (c_r − mean)² / (used (used − 1))), 0 for one replica;
        n defaults to nt = Lz // 2 + 1.  Raises StochQuantError (SQ_E_STATE)
        when no replica has a measurement."""
        n = self.nt if n is None else int(n)
        mean, err = np.zeros(max(n, 0)), np.zeros(max(n, 0))
        used = ctypes.c_int(0)
        _lib.call("sq_phi4_ens_correlator", self._h, 1 if connected else 0, _dptr(mean), _dptr(err), n,
                  ctypes.byref(used))
        return mean, err, used.value

    @staticmethod
    def corr_shape_info(shape):
        """The correlator launches' LDS layout for a lattice of `shape`
        (sq_phi4_ens_corr_shape_info; no device needed): {"images" / "lds_bytes"
        of the step launch with the correlator, "frames_images" /
        "frames_lds_bytes", "slices_lds_bytes", "nt"}."""
        dims = (ctypes.c_int * 3)(*(int(s) for s in shape))
        out = (ctypes.c_int * 6)()
        _lib.call("sq_phi4_ens_corr_shape_info", dims, out)
        return dict(zip(("images", "lds_bytes", "frames_images", "frames_lds_bytes", "slices_lds_bytes", "nt"),
                        (int(v) for v in out)))

    @staticmethod
    def momentum_table(L, n):
        """(c, s): the twiddle table of momentum index n on an axis of L sites,
        c[k] = cos(2π j / L), s[k] = sin(2π j / L), j = (n k) mod L, exact at the
        quarter turns (sq_phi4_ens_momentum_table; no device needed).  The
        kernels use these values."""
        c, s = np.zeros(max(int(L), 0)), np.zeros(max(int(L), 0))
        _lib.call("sq_phi4_ens_momentum_table", int(L), int(n), _dptr(c), _dptr(s))
        return c, s

    def set_momenta(self, pairs):
        """The spatial momenta (nx, ny), p = (2π nx / Lx, 2π ny / Ly), measured
        by step(momenta=True) and run_frames(momenta=True): at most 8, duplicates
        allowed.  Zeroes the momentum accumulators of every replica."""
        a = np.ascontiguousarray(np.asarray(list(pairs), dtype=np.int32).reshape(-1, 2))
        _lib.call("sq_phi4_ens_set_momenta", self._h, a.shape[0], a.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))

    @property
    def momenta(self):
        """The momenta set: a list of (nx, ny)."""
        M = ctypes.c_int(0)
        a = np.zeros((_lib.SQ_PHI4_ENS_MAX_MOMENTA, 2), dtype=np.int32)
        _lib.call("sq_phi4_ens_get_momenta", self._h, ctypes.byref(M), a.ctypes.data_as(ctypes.POINTER(ctypes.c_int)))
        return [(int(x), int(y)) for x, y in a[:M.value]]

    def pcorr_sums(self, first=0, count=None):
        """The raw momentum accumulators of replicas first .. first + count: (G
        (count, M, nt) = Σ over measurements of g_m(t) = Σ_z [A(z) A(z + t) +
        B(z) B(z + t)], nmeas (count,) int64), A + iB the slice's projection on
        momentum m; see include/stochquant.h for the arithmetic."""
        k, M = self._count(first, count), len(self.momenta)
        G = np.zeros((max(k, 0), M, self.nt))
        nm = np.zeros(max(k, 0), dtype=np.int64)
        _lib.call("sq_phi4_ens_pcorr_sums", self._h, int(first), k, _dptr(G),
                  nm.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)))
        return G, nm

    def pcorr_reset(self, first=0, count=None):
        """Zero the momentum accumulators of replicas first .. first + count."""
        _lib.call("sq_phi4_ens_pcorr_reset", self._h, int(first), self._count(first, count))

    def pslices(self, first=0, count=None):
        """One momentum measurement of the current fields, accumulating nothing:
        (AB (count, M, Lz, 2) projections A and B, g (count, M, nt))."""
        k, M = self._count(first, count), len(self.momenta)
        AB = np.zeros((max(k, 0), M, self.shape[2], 2))
        g = np.zeros((max(k, 0), M, self.nt))
        _lib.call("sq_phi4_ens_pslices", self._h, int(first), k, _dptr(AB), _dptr(g))
        return AB, g

    def pcorrelator(self, n=None):
        """(mean (M, n), err (M, n), used): per momentum the replica mean and
        standard error of c_r(m, t) = Gp_r[m][t] / (nmeas_p,r V), as `correlator`
        computes them with connected=False.  Raises StochQuantError (SQ_E_STATE)
        when no replica has a momentum measurement."""
        n, M = (self.nt if n is None else int(n)), len(self.momenta)
        mean, err = np.zeros((M, max(n, 0))), np.zeros((M, max(n, 0)))
        used = ctypes.c_int(0)
        _lib.call("sq_phi4_ens_pcorrelator", self._h, _dptr(mean), _dptr(err), n, ctypes.byref(used))
        return mean, err, used.value

    @staticmethod
    def pcorr_shape_info(shape):
        """The momentum launches' LDS layout for a lattice of `shape`
        (sq_phi4_ens_pcorr_shape_info; no device needed): the keys of
        `corr_shape_info`, "slices_lds_bytes" being the pslices launch's.  Raises
        StochQuantError (SQ_E_ARG) for a shape that cannot hold momenta."""
        dims = (ctypes.c_int * 3)(*(int(s) for s in shape))
        out = (ctypes.c_int * 6)()
        _lib.call("sq_phi4_ens_pcorr_shape_info", dims, out)
        return dict(zip(("images", "lds_bytes", "frames_images", "frames_lds_bytes", "slices_lds_bytes", "nt"),
                        (int(v) for v in out)))

    def set_flow(self, eps, levels=(), m2=None, lam=None):
        """The gradient flow measured by step(flow=True), `flowed` and
        `flow_field`: flow step eps > 0, up to 4 strictly ascending levels
        (numbers of flow steps, 0 = the field itself, at most 4096), and
        optionally the flow's own m² and λ for all replicas (None: each
        replica's own; 0 and 0: the lattice heat equation).  set_flow(None)
        turns the flow off.  Zeroes the flow accumulators of every replica;
        raises, changing nothing, where a replica's flow coefficients would
        break the parameter bound."""
        if eps is None:
            _lib.call("sq_phi4_ens_set_flow", self._h, 0.0, 0, None, None, None)
            return
        lv = np.ascontiguousarray(np.asarray(list(levels), dtype=np.int32).reshape(-1))
        m, l = (None if v is None else ctypes.c_double(float(v)) for v in (m2, lam))
        _lib.call("sq_phi4_ens_set_flow", self._h, float(eps), lv.shape[0],
                  lv.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if lv.size else None,
                  None if m is None else ctypes.byref(m), None if l is None else ctypes.byref(l))

    @property
    def flow(self):
        """The flow set: {"eps", "levels" (tuple), "m2", "lam" (None: each replica's own)}, or None."""
        eps, m, l = ctypes.c_double(0.0), ctypes.c_double(0.0), ctypes.c_double(0.0)
        F = ctypes.c_int(0)
        lv = (ctypes.c_int * _lib.SQ_PHI4_ENS_MAX_FLOW_LEVELS)()
        _lib.call("sq_phi4_ens_get_flow", self._h, ctypes.byref(eps), ctypes.byref(F), lv, ctypes.byref(m),
                  ctypes.byref(l))
        if F.value == 0:
            return None
        return {"eps": eps.value, "levels": tuple(int(v) for v in lv[:F.value]),
                "m2": None if np.isnan(m.value) else m.value, "lam": None if np.isnan(l.value) else l.value}

    def _flow_levels(self):
        f = self.flow
        return len(f["levels"]) if f else 0

    def flowed(self, first=0, count=None):
        """One measurement per flow level of the current fields, accumulating
        nothing and leaving the fields alone: (sums (count, F, 4) = S1, S2, S4,
        NN, S (count, F, Lz) slice sums, g (count, F, nt))."""
        k, F = self._count(first, count), self._flow_levels()
        sums = np.zeros((max(k, 0), F, 4))
        S = np.zeros((max(k, 0), F, self.shape[2]))
        g = np.zeros((max(k, 0), F, self.nt))
        _lib.call("sq_phi4_ens_flowed", self._h, int(first), k, _dptr(sums), _dptr(S), _dptr(g))
        return sums, S, g

    def flow_field(self, nsteps, first=0, count=None):
        """The current fields after `nsteps` flow steps (0 .. 4096) with the
        step, m² and λ of `set_flow`: (count, Lz, Ly, Lx); the stored fields are
        untouched."""
        k = self._count(first, count)
        a = np.empty((max(k, 0),) + self.lattice_shape, dtype=np.float32)
        _lib.call("sq_phi4_ens_flow_field", self._h, int(first), k, int(nsteps), _fptr(a))
        return a

    def fcorr_sums(self, first=0, count=None):
        """The raw flow accumulators of replicas first .. first + count: (G
        (count, F, nt), S1 (count, F), nmeas (count,) int64), per level what
        `corr_sums` holds for the plain correlator."""
        k, F = self._count(first, count), self._flow_levels()
        G = np.zeros((max(k, 0), F, self.nt))
        S1 = np.zeros((max(k, 0), F))
        nm = np.zeros(max(k, 0), dtype=np.int64)
        _lib.call("sq_phi4_ens_fcorr_sums", self._h, int(first), k, _dptr(G), _dptr(S1),
                  nm.ctypes.data_as(ctypes.POINTER(ctypes.c_longlong)))
        return G, S1, nm

    def fcorr_reset(self, first=0, count=None):
        """Zero the flow accumulators of replicas first .. first + count (`set_flow` clears all of them)."""
        _lib.call("sq_phi4_ens_fcorr_reset", self._h, int(first), self._count(first, count))

    def fcorrelator(self, n=None, connected=True):
        """(mean (F, n), err (F, n), used): `correlator`'s statistics per flow level."""
        n, F = (self.nt if n is None else int(n)), self._flow_levels()
        mean, err = np.zeros((F, max(n, 0))), np.zeros((F, max(n, 0)))
        used = ctypes.c_int(0)
        _lib.call("sq_phi4_ens_fcorrelator", self._h, 1 if connected else 0, _dptr(mean), _dptr(err), n,
                  ctypes.byref(used))
        return mean, err, used.value

    @staticmethod
    def flow_shape_info(shape):
        """The flow launches' LDS layout for a lattice of `shape`
        (sq_phi4_ens_flow_shape_info; no device needed): {"images" / "lds_bytes"
        of step(flow=True) without the correlator (the plain step launch's),
        "corr_images" / "corr_lds_bytes" with it (the correlator step launch's),
        "flowed_lds_bytes", "stash": where the un-flowed field waits during a
        flow, 0 = registers, 1 = device memory}."""
        dims = (ctypes.c_int * 3)(*(int(s) for s in shape))
        out = (ctypes.c_int * 6)()
        _lib.call("sq_phi4_ens_flow_shape_info", dims, out)
        return dict(zip(("images", "lds_bytes", "corr_images", "corr_lds_bytes", "flowed_lds_bytes", "stash"),
                        (int(v) for v in out)))

    def flags(self, clear=False, first=0, count=None):
        """(count,) bool array: a step since the last clear clamped a site or met a NaN."""
        k = self._count(first, count)
        f = np.zeros(max(k, 0), dtype=np.int32)
        _lib.call("sq_phi4_ens_flags", self._h, int(first), k, f.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                  1 if clear else 0)
        return f != 0

    def perf(self):
        p = _lib.SqPerf()
        _lib.call("sq_phi4_ens_perf", self._h, ctypes.byref(p))
        return {k: getattr(p, k) for k, _ in p._fields_}

    def digest(self, first=0, count=None):
        """(count,) uint64: the field digest of replicas first .. first + count, computed on the device
        (sq_phi4_ensemble_digest): the wrapping sum over sites i of mix(i << 32 | bits32(phi[i])), mix the
        splitmix64 finaliser.  Two fields have one digest exactly when they agree bit for bit (up to 2^-64);
        nothing is moved but eight bytes per replica, and nothing changes."""
        k = self._count(first, count)
        d = np.zeros(max(k, 0), dtype=np.uint64)
        _lib.call("sq_phi4_ensemble_digest", self._h, int(first), k, d.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)))
        return d

    def save(self, path):
        """Checkpoint the whole ensemble as `path` (.npy: np.load(path) is download()), `path`.state and
        `path`.json (sq_phi4_ensemble_save): fields, seeds, counters, Δτ, parameters, frame state, settings,
        every accumulator and every sampler statistic.  The handle goes on as one that never saved."""
        _lib.call("sq_phi4_ensemble_save", self._h, os.fsencode(path))

    def load(self, path, fields_only=False):
        """Resume from the checkpoint `path` (sq_phi4_ensemble_load): shape, replicas, loops, clamp and adapt_dtau
        must be this ensemble's; everything else, the seeds included, comes from the files, and the run goes on
        bit for bit as the saver would have.  Every file is validated first: a refused load (StochQuantError)
        changes nothing.  fields_only: only shape and replicas must match, and only the fields are taken."""
        _lib.call("sq_phi4_ensemble_load", self._h, os.fsencode(path), 1 if fields_only else 0)
        if not fields_only:
            self._frames_run = self._has_frame_records()  # as on the handle that saved

    def _has_frame_records(self):
        """Whether the handle holds a last frame's records: sq_phi4_ens_stability takes n = 1 exactly then."""
        one = [np.zeros(1, dtype=np.float32) for _ in range(3)]
        rc = _lib.load().sq_phi4_ens_stability(self._h, 0, 0, None, None, *[_fptr(a) for a in one], 1)
        return rc == _lib.SQ_OK

    @staticmethod
    def checkpoint_info(path, verify=False):
        """The identity of the checkpoint `path` (sq_phi4_ensemble_checkpoint_info; no device, no handle):
        {"version", "shape", "replicas", "loops", "adapt_dtau", "sections", "clamp"}.  verify: also read the other
        two files and run every check of a load that needs no handle.  Raises StochQuantError (SQ_E_ARG) for a
        set of files a load would refuse."""
        info = (ctypes.c_longlong * 8)()
        clamp = ctypes.c_double()
        _lib.call("sq_phi4_ensemble_checkpoint_info", os.fsencode(path), 1 if verify else 0, info, ctypes.byref(clamp))
        v = [int(x) for x in info]
        return {"version": v[0], "shape": (v[1], v[2], v[3]), "replicas": v[4], "loops": v[5],
                "adapt_dtau": bool(v[6]), "sections": v[7], "clamp": clamp.value}

    @classmethod
    def restore(cls, path, device=0):
        """A new ensemble of the checkpoint's identity, loaded from it."""
        i = cls.checkpoint_info(path)
        # placeholder parameters any clamp admits; the load brings the saved ones
        e = cls(i["shape"], i["replicas"], dtau=1e-30, m2=0.0, lam=0.0, C=0.0, clamp=i["clamp"], device=device,
                loops=i["loops"], adapt_dtau=i["adapt_dtau"])
        try:
            e.load(path)
        except Exception:
            e.close()
            raise
        return e


def connect_p2p(lat, group=None):
    """All-gather the ranks' P2P handle blobs over torch.distributed and connect."""
    import torch.distributed as dist
    blobs = [None] * dist.get_world_size(group)
    dist.all_gather_object(blobs, lat.p2p_handle(), group=group)
    lat.p2p_connect(blobs)


def unique_id():
    """RCCL unique id (128 bytes) for SQ_COMM_RCCL contexts."""
    buf = (ctypes.c_ubyte * 128)()
    _lib.call("sq_comm_unique_id", buf)
    return bytes(buf)


# --------------------------------------------------------------------------
# Process/CLI contract of the reference (taumain.py:132 -> tauhost.o)
# --------------------------------------------------------------------------
TAUHOST_ARGS = ("n", "deltat", "deltatau", "frames", "potID", "c", "device", "rpf", "intime",
                "loops", "inputf", "outputf", "acco")


def tauhost_argv(n, deltat, deltatau, frames, potID, c, device, rpf, intime, loops, inputf, outputf,
                 acco, exe=None):
    """argv exactly as taumain.py:132 builds it (every value passed through str())."""
    exe = exe or _lib.TAUHOST_PATH
    return [exe] + [str(v) for v in (n, deltat, deltatau, frames, potID, c, device, rpf, intime, loops,
                                     inputf, outputf, acco)]


def run_tauhost(argv, cwd=None, timeout=600, env=None):
    """Run the drop-in executable; returns CompletedProcess with bytes stdout."""
    if not os.path.exists(argv[0]):
        raise _lib.StochQuantUnavailable(f"{argv[0]} not built")
    return subprocess.run(argv, cwd=cwd, capture_output=True, timeout=timeout, env=env)


def parse_frame_line(line):
    """taumain.py:30-41: np.genfromtxt(delimiter='|'); last two fields Δτ, percent."""
    tmp = np.genfromtxt(io.BytesIO(line.strip()), delimiter="|")
    return {"y": tmp[:-2], "dtau": tmp[-2], "percent": tmp[-1]}
