// sq_core.cpp -- C ABI of libstochquant.so (include/stochquant.h): the error
// message, context creation and destruction, the scalar getters and setters,
// the profiling event pool and the perf counters.
//
// Replaces the OpenCL host plumbing of tauhost.c (buffers, kernel args, the
// per-frame launch / read-back / rollback / re-upload, tauhost.c:196-560) with
// a library that owns device memory, HIP streams and RCCL communicators:
//   * QM1D: frame-start state and frame result live in two device buffer sets;
//     a stable frame flips the set, an unstable one simply keeps the old set
//     (rollback without the reference's 3N+1-double host round trip).
//   * PHI4: a slab per process (RCCL) or several slabs per device (loopback),
//     each a padded ping-pong pair; per step the interior planes update on
//     stream A while the halo exchange and the two boundary planes run on
//     stream B, joined by events.
#include <cstring>

#include "sq_ctx.h"

using namespace sq;

namespace {

thread_local std::string g_err;

}  // namespace

int sq::set_error(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

namespace sq {

int flush_events(sq_ctx *c) {
    for (size_t i = 0; i < c->ev_used; ++i) {
        SQ_HIP(hipEventSynchronize(c->evpool[i].b));
        float ms = 0;
        SQ_HIP(hipEventElapsedTime(&ms, c->evpool[i].a, c->evpool[i].b));
        c->perf.step_kernel_ms += ms;
        c->perf.step_kernel_launches += 1;
    }
    c->perf.step_kernel_launches += c->ev_extra_steps;
    c->ev_extra_steps = 0;
    if (c->region_steps > 0) {  // region mode: one pair per sq_step call covering its steps
        c->perf.step_kernel_launches += c->region_steps - (long long)c->ev_used;
        c->region_steps = 0;
    }
    c->ev_used = 0;
    return SQ_OK;
}

int ev_take(sq_ctx *c, EvPair **out) {
    *out = nullptr;
    if (c->ev_used == c->evpool.size()) {
        if (c->evpool.size() >= 8192) {
            int rc = flush_events(c);
            if (rc) return rc;
        } else {
            EvPair e;
            SQ_HIP(hipEventCreate(&e.a));
            SQ_HIP(hipEventCreate(&e.b));
            c->evpool.push_back(e);
        }
    }
    *out = &c->evpool[c->ev_used++];
    return SQ_OK;
}

// Marker-event pair around one launch (QM1D frames; per-launch mode only).
int ev_begin(sq_ctx *c, hipStream_t s, EvPair **out) {
    *out = nullptr;
    if (c->profiling != 1) return SQ_OK;
    int rc = ev_take(c, out);
    if (rc) return rc;
    SQ_HIP(hipEventRecord((*out)->a, s));
    return SQ_OK;
}

void release_events(sq_ctx *c) {
    for (auto &e : c->evpool) {
        (void)hipEventDestroy(e.a);
        (void)hipEventDestroy(e.b);
    }
    c->evpool.clear();
    c->ev_used = 0;
}

}  // namespace sq

extern "C" {

void sq_params_init(sq_params *p) {
    memset(p, 0, sizeof *p);
    p->struct_size = (int)sizeof(sq_params);
    p->model = SQ_MODEL_QM1D;
    p->dims[0] = 200;
    p->dims[1] = 1;
    p->dims[2] = 1;
    p->deltat = 0.02;
    p->deltatau = 0.002;
    p->pot = 3;
    p->C = 1.0;
    p->loops = 1000;
    p->seed = 0x5EEDull;
    p->m2 = 1.0;
    p->lambda = 1.0;
    p->clamp = 1000.0;
    p->device = 0;
    p->adapt_dtau = 1;
    p->comm = SQ_COMM_NONE;
    p->nranks = 1;
    p->rank = 0;
    p->nslabs = 1;
}

const char *sq_last_error(void) { return g_err.c_str(); }
int sq_abi_version(void) { return SQ_ABI_VERSION; }

int sq_device_count(int *n) {
    int k = 0;
    hipError_t e = hipGetDeviceCount(&k);
    if (e != hipSuccess) k = 0;
    *n = k;
    return SQ_OK;
}

int sq_create(const sq_params *p, sq_ctx **out) {
    if (!p || !out) return fail(SQ_E_ARG, "null argument");
    *out = nullptr;
    if (p->struct_size != (int)sizeof(sq_params)) return fail(SQ_E_ARG, "sq_params size mismatch");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SQ_E_NODEV, "no HIP device");
    if (p->device < 0 || p->device >= ndev) return fail(SQ_E_ARG, "device ordinal out of range");
    if (!(p->deltatau > 0)) return fail(SQ_E_ARG, "deltatau must be > 0");
    DeviceGuard g(p->device);
    sq_ctx *c = new sq_ctx();
    c->p = *p;
    c->dev = p->device;
    c->dtau = p->deltatau;
    int rc = p->model == SQ_MODEL_PHI4 ? create_phi4(c) : p->model == SQ_MODEL_QM1D ? create_qm1d(c)
                                                                                      : fail(SQ_E_ARG, "unknown model");
    if (rc) {
        std::string msg = g_err;
        sq_destroy(c);
        g_err = msg;
        return rc;
    }
    *out = c;
    return SQ_OK;
}

int sq_destroy(sq_ctx *c) {
    if (!c) return SQ_OK;
    DeviceGuard g(c->dev);
    if (!p2p_drain(c)) return SQ_OK;  // leak rather than free memory a peer may still read
    for (auto &s : c->slabs) {
        if (s.sA) (void)hipStreamSynchronize(s.sA);
        if (s.sB) (void)hipStreamSynchronize(s.sB);
    }
    p2p_close_peers(c);
    release_p2p(c);
    release_gate(c);
    release_rccl(c);
    release_slabs(c);
    release_qm1d_serial(c);
    release_frames(c);
    release_lattice(c);
    release_qm1d(c);
    release_events(c);
    delete c;
    return SQ_OK;
}

int sq_sync(sq_ctx *c) {
    if (!c) return fail(SQ_E_ARG, "null context");
    DeviceGuard g(c->dev);
    if (c->qstream) SQ_HIP(hipStreamSynchronize(c->qstream));
    int rc = phi4_join(c);
    if (rc) return rc;
    return gate_check(c, true);  // a gated rim chunk gave up waiting for its exchange: sticky
}

int sq_get_params(sq_ctx *c, sq_params *out) {
    if (!c || !out) return fail(SQ_E_ARG, "null argument");
    *out = c->p;
    out->deltatau = c->dtau;
    return SQ_OK;
}

int sq_set_dtau(sq_ctx *c, double dtau) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (!(dtau > 0) || !std::isfinite(dtau) || (is_phi4(c) && dtau > 1e20))
        return fail(SQ_E_ARG, "dtau must be finite, > 0 (and <= 1e20 for PHI4: the guard's drift bound)");
    c->dtau = dtau;
    return SQ_OK;
}
int sq_get_dtau(sq_ctx *c, double *dtau) {
    if (!c || !dtau) return fail(SQ_E_ARG, "null argument");
    *dtau = c->dtau;
    return SQ_OK;
}
int sq_get_step(sq_ctx *c, unsigned long long *step) {
    if (!c || !step) return fail(SQ_E_ARG, "null argument");
    *step = c->step;
    return SQ_OK;
}
int sq_set_step(sq_ctx *c, unsigned long long step) {
    if (!c) return fail(SQ_E_ARG, "null context");
    c->step = step;
    return SQ_OK;
}

int sq_set_profiling(sq_ctx *c, int on) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (on < 0 || on > 2) return fail(SQ_E_ARG, "profiling mode must be 0, 1 or 2");
    int rc = flush_events(c);
    if (rc) return rc;
    c->profiling = on;
    return SQ_OK;
}

int sq_perf(sq_ctx *c, sq_perf_t *out) {
    if (!c || !out) return fail(SQ_E_ARG, "null argument");
    DeviceGuard g(c->dev);
    int rc = flush_events(c);
    if (rc) return rc;
    *out = c->perf;
    return SQ_OK;
}

int sq_perf_reset(sq_ctx *c) {
    if (!c) return fail(SQ_E_ARG, "null context");
    DeviceGuard g(c->dev);
    int rc = flush_events(c);
    if (rc) return rc;
    c->perf = sq_perf_t{};
    c->kstat.clear();
    return SQ_OK;
}

}  // extern "C"
