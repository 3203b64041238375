"""Child process of tests/test_gpu_qm1d_forced_k.py: the QM1D kernels under the
SQ_QM1D_K tuning override.

qm1d_wave_shape reads the override once per process, so every value of it needs
a process of its own.  The child is forked by the fork server that conftest.py
starts before the test process touches the GPU (as tests/p2p_ranks.py's ranks),
sets the override before it imports the package, runs the jobs the test gave it
and sends back what it downloaded; the test compares that with the oracle.

A job is a dict.  kind "ens": one Qm1dEnsemble frame of len(seeds) replicas
(f, x, xx0 of shape (N,) or (R, N); omega, runs scalars or (R,); dtau None or
(R,)).  kind "chain": one Qm1dChain frame (seed; f, x, xx0 of shape (N,)).
"""
import os
import sys
import traceback


def _ens(job):
    import numpy as np
    from stochquant_amd import Qm1dEnsemble
    seeds = np.asarray(job["seeds"], dtype=np.uint64)
    with Qm1dEnsemble(job["N"], job["a"], job["h"], len(seeds), seeds=seeds, pot=job["pot"], C=1.0,
                      loops=job["loops"], adapt_dtau=False) as e:
        e.upload(job["f"], job["x"], job["xx0"], job["omega"], job["runs"])
        e.set_scan(job["lrgEl"], job["lrgVl"], job["tick"])
        if job.get("dtau") is not None:
            e.dtau = job["dtau"]
        st = e.run_frame()
        return {"stable": st, "state": e.download(), "scan": e.scan, "dtau": e.dtau, "steps": e.perf()["steps"]}


def _chain(job):
    from stochquant_amd import Qm1dChain
    with Qm1dChain(job["N"], job["a"], job["h"], pot=job["pot"], C=1.0, loops=job["loops"], seed=job["seed"],
                   adapt_dtau=False) as q:
        q.upload(job["f"], job["x"], job["xx0"], job["omega"], job["runs"])
        q.set_scan(job["lrgEl"], job["lrgVl"], job["tick"])
        st = q.run_frame()
        return {"stable": st, "state": q.download(), "scan": q.scan}


def worker_main(conn, k, jobs):
    try:
        os.environ["SQ_QM1D_K"] = str(k)   # before the package, and with it the library, is loaded
        loaded = sys.modules.get("stochquant_amd._lib")
        assert loaded is None or loaded._lib is None, "the library was loaded before the override was set"
        out = [{"ens": _ens, "chain": _chain}[job["kind"]](job) for job in jobs]
        conn.send(("ok", out))
    except Exception:  # reported to the parent, which fails the test
        conn.send(("error", traceback.format_exc()))
    finally:
        conn.close()
