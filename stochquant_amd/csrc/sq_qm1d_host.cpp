// sq_qm1d_host.cpp -- QM1D contexts: buffers, the Jacobi-order frame
// (sq_qm1d.hip) and the reference's serial order (sq_qm1d_gs.hip), their host
// bookkeeping, and the sq_qm1d_* entry points.
#include <cmath>
#include <cstdio>
#include <cstring>

#include "sq_ctx.h"

using namespace sq;

namespace sq {

double host_intconst(int pot) {  // tau_kernel.cl:196-200,237-246 (float arithmetic)
    if (pot == 3)
        return (double)(sqrtf((float)3.) * powf((float)2., (float)(-5. / 4.)) *
                        powf((float)2., (float)(-1. / 4.)) / sqrtf((float).8));
    return 0.;
}

int create_qm1d(sq_ctx *c) {
    const sq_params &p = c->p;
    if (p.dims[0] < 2 || p.dims[0] > (1 << 30)) return fail(SQ_E_ARG, "QM1D needs N >= 2");
    c->N = (int)p.dims[0];
    if (sq::qm1d_sites_per_thread(c->N) == 0)
        return fail(SQ_E_ARG, "QM1D supports 2 <= N <= 65536 (one work-group per frame)");
    if (p.pot != 0 && p.pot != 3) return fail(SQ_E_ARG, "potID must be 0 or 3 (tau_kernel.cl:215-246)");
    if (!(p.deltat > 0)) return fail(SQ_E_ARG, "deltat must be > 0");
    if (p.loops < 1) return fail(SQ_E_ARG, "loops must be >= 1");
    const size_t bytes = sizeof(double) * (size_t)c->N;
    for (int k = 0; k < 2; ++k) {
        SQ_HIP(hipMalloc(&c->qf[k], bytes));
        SQ_HIP(hipMalloc(&c->qx[k], bytes));
        SQ_HIP(hipMalloc(&c->qxx0[k], bytes));
        SQ_HIP(hipMemset(c->qf[k], 0, bytes));
        SQ_HIP(hipMemset(c->qx[k], 0, bytes));
        SQ_HIP(hipMemset(c->qxx0[k], 0, bytes));
    }
    if (c->N > sq::kQm1dRegMaxN)  // global-memory variant: f ping-pong + scan scratch
        for (int k = 0; k < 3; ++k)  // xs, ds: + the grid kernel's block maxima and scan words
            SQ_HIP(hipMalloc(&c->qscr[k], k == 0 ? bytes : bytes + sizeof(double) * sq::kQm1dGridAux));
    SQ_HIP(hipMalloc(&c->qst, sizeof(sq::Qm1dState)));
    SQ_HIP(hipStreamCreateWithFlags(&c->qstream, hipStreamNonBlocking));
    SQ_HIP(hipDeviceSynchronize());  // the set-up memsets ran on the null stream
    return SQ_OK;
}

void release_qm1d(sq_ctx *c) {
    for (int k = 0; k < 2; ++k) {
        (void)hipFree(c->qf[k]);
        (void)hipFree(c->qx[k]);
        (void)hipFree(c->qxx0[k]);
    }
    (void)hipFree(c->qst);
    for (double *q : c->qscr) (void)hipFree(q);
    (void)hipFree(c->qom);
    (void)hipFree(c->qdd);
    (void)hipFree(c->qxi);
    (void)hipFree(c->qtcl);
    for (int k = 0; k < 2; ++k) c->qf[k] = c->qx[k] = c->qxx0[k] = nullptr;
    for (double *&q : c->qscr) q = nullptr;
    c->qst = nullptr;
    c->qom = c->qdd = nullptr;
    c->qxi = c->qtcl = nullptr;
    if (c->qstream) (void)hipStreamDestroy(c->qstream);
    c->qstream = nullptr;
}

}  // namespace sq

namespace {

// The serial-order buffers by the capacity that sizes them (gs_reserve grows
// each on its own): the per-call draws, the history, the per-step tables.
void gs_free_calls(sq_ctx *c) {
    (void)hipFree(c->g_xi);
    (void)hipFree(c->g_w1);
    (void)hipFree(c->g_w2);
    (void)hipFree(c->g_seeds);
    c->g_xi = nullptr;
    c->g_w1 = c->g_w2 = nullptr;
    c->g_seeds = nullptr;
    c->g_calls = 0;
}

void gs_free_hist(sq_ctx *c) {
    (void)hipFree(c->g_hist_buf);
    c->g_hist_buf = nullptr;
    c->g_hist = 0;
}

void gs_free_loops(sq_ctx *c) {
    (void)hipFree(c->g_om);
    (void)hipFree(c->g_xc);
    (void)hipFree(c->g_cand);
    (void)hipFree(c->g_flags);
    c->g_om = c->g_xc = nullptr;
    c->g_cand = nullptr;
    c->g_flags = nullptr;
    c->g_loops = 0;
}

// Capacity of the serial-order buffers for one full launch.
int gs_reserve(sq_ctx *c) {
    const long long calls = (long long)(c->N + 1) * c->p.loops;
    const long long hist = (long long)c->N * c->p.loops;
    if (calls > c->g_calls) {
        gs_free_calls(c);
        SQ_HIP(hipMalloc(&c->g_xi, sizeof(double) * calls));
        SQ_HIP(hipMalloc(&c->g_w1, sizeof(uint32_t) * calls));
        SQ_HIP(hipMalloc(&c->g_w2, sizeof(uint32_t) * calls));
        SQ_HIP(hipMalloc(&c->g_seeds, sizeof(unsigned long long) * calls));
        c->g_calls = calls;
    }
    if (c->g_lcg_scr == nullptr) SQ_HIP(hipMalloc(&c->g_lcg_scr, sizeof(unsigned long long) * sq::kLcgScratch));
    if (hist > c->g_hist) {
        gs_free_hist(c);
        SQ_HIP(hipMalloc(&c->g_hist_buf, sizeof(double) * hist));
        c->g_hist = hist;
    }
    if (c->p.loops > c->g_loops) {
        gs_free_loops(c);
        SQ_HIP(hipMalloc(&c->g_om, sizeof(double) * (c->p.loops + 1)));
        SQ_HIP(hipMalloc(&c->g_xc, sizeof(double) * 2 * (c->N + 2) * (size_t)c->p.loops));
        SQ_HIP(hipMalloc(&c->g_cand, sq::qm1d_gs_cand_bytes(c->p.loops)));
        SQ_HIP(hipMalloc(&c->g_flags, sizeof(int) * (size_t)c->p.loops));
        SQ_HIP(hipMemset(c->g_flags, 0, sizeof(int) * (size_t)c->p.loops));
        c->gs_tag = 0;
        c->g_loops = c->p.loops;
    }
    if (!c->g_st) SQ_HIP(hipMalloc(&c->g_st, sizeof(sq::Qm1dGsState)));
    return SQ_OK;
}

}  // namespace

namespace sq {

void release_qm1d_serial(sq_ctx *c) {
    gs_free_calls(c);
    gs_free_hist(c);
    gs_free_loops(c);
    (void)hipFree(c->g_nfp);
    (void)hipFree(c->g_lcg_scr);
    (void)hipFree(c->g_st);
    c->g_nfp = nullptr;
    c->g_lcg_scr = nullptr;
    c->g_st = nullptr;
}

}  // namespace sq

namespace {

// One launch of time_dev in the reference's serial order (sq_qm1d_gs.hip);
// host bookkeeping as qm1d_frame, plus the shared seed: it advances by the
// calls the launch made, whether or not the frame was stable (tauhost.c never
// rolls it back).
int qm1d_gs_frame(sq_ctx *c, int *stable) {
    int rc = gs_reserve(c);
    if (rc) return rc;
    const long long calls = (long long)(c->N + 1) * c->p.loops;
    const bool injected = c->inject_pending;
    c->inject_pending = false;
    EvPair *e = nullptr;
    rc = ev_begin(c, c->qstream, &e);
    if (rc) return rc;
    if (!injected)
        SQ_HIP(sq::qm1d_gs_lcg_launch(c->lcg_seed, c->N, calls, c->g_w1, c->g_w2, c->g_seeds, c->g_xi,
                                      c->g_lcg_scr, c->qstream));
    sq::Qm1dGsArgs a{};
    const int k = c->qcur;
    a.f0 = c->qf[k];
    a.x0 = c->qx[k];
    a.xx00 = c->qxx0[k];
    a.nf = c->qf[k ^ 1];
    a.nx = c->qx[k ^ 1];
    a.nxx0 = c->qxx0[k ^ 1];
    a.nfp = c->g_nfp;
    a.xi = c->g_xi;
    a.om = c->g_om;
    a.xc = c->g_xc;
    a.cand = c->g_cand;
    a.flags = c->g_flags;
    c->gs_tag = c->gs_tag == 0x7fffffff ? 1 : c->gs_tag + 1;
    a.tag = c->gs_tag;
    a.hist = c->g_hist_buf;
    a.st = c->g_st;
    a.N = c->N;
    a.pot = c->p.pot;
    a.loops = c->p.loops;
    a.runs = (int)c->runs;
    a.a = c->p.deltat;
    const float fa = (float)c->p.deltat;
    a.a2 = (double)(fa * fa);
    a.h = c->dtau;
    a.sig = c->p.C * (double)sqrtf((float)(2. * c->dtau / c->p.deltat));
    a.sigw = c->p.C * (double)sqrtf((float)(2. * c->dtau));
    a.kconst = host_intconst(c->p.pot);
    sq::Qm1dGsState st{};
    st.omega_in = c->omega;
    st.lrgEl = c->lrgEl;
    st.lrgVl = c->lrgVl;
    SQ_HIP(hipMemcpyAsync(c->g_st, &st, sizeof st, hipMemcpyHostToDevice, c->qstream));
    SQ_HIP(sq::qm1d_gs_frame_launch(a, c->qstream));
    if (e) SQ_HIP(hipEventRecord(e->b, c->qstream));
    SQ_HIP(hipMemcpyAsync(&st, c->g_st, sizeof st, hipMemcpyDeviceToHost, c->qstream));
    SQ_HIP(hipStreamSynchronize(c->qstream));
    if (st.sync_error) return fail(SQ_E_HIP, "serial frame: the scan timed out waiting for the sweep");
    c->consumed = (unsigned long long)st.consumed;
    if (!injected && st.consumed > 0)
        SQ_HIP(hipMemcpy(&c->lcg_seed, c->g_seeds + (st.consumed - 1), sizeof(unsigned long long),
                         hipMemcpyDeviceToHost));
    c->step += (unsigned long long)c->p.loops;
    c->lrgEl = st.lrgEl;
    c->lrgVl = st.lrgVl;
    c->perf.steps += st.steps_done;
    c->perf.site_updates += (long long)st.steps_done * c->N;
    *stable = st.stable;
    if (st.stable == 1) {  // tauhost.c:506-532
        c->qcur ^= 1;
        c->omega = st.omega_out;
        c->runs += c->p.loops;
    }
    return SQ_OK;
}

}  // namespace

namespace sq {

int qm1d_frame(sq_ctx *c, int *stable) {
    if (c->order == SQ_ORDER_SERIAL) return qm1d_gs_frame(c, stable);
    sq::Qm1dArgs a{};
    const int k = c->qcur;
    a.f = c->qf[k];
    a.x = c->qx[k];
    a.xx0 = c->qxx0[k];
    a.nf = c->qf[k ^ 1];
    a.nx = c->qx[k ^ 1];
    a.nxx0 = c->qxx0[k ^ 1];
    a.fs = c->qscr[0];
    a.xs = c->qscr[1];
    a.ds = c->qscr[2];
    a.st = c->qst;
    a.N = c->N;
    a.pot = c->p.pot;
    a.loops = c->p.loops;
    a.runs = (int)c->runs;
    a.a = c->p.deltat;
    const float fa = (float)c->p.deltat;
    a.a2 = (double)(fa * fa);
    a.h = c->dtau;
    a.sig = c->p.C * (double)sqrtf((float)(2. * c->dtau / c->p.deltat));
    a.sigw = c->p.C * (double)sqrtf((float)(2. * c->dtau));
    a.kconst = host_intconst(c->p.pot);
    a.k0 = (uint32_t)c->p.seed;
    a.k1 = (uint32_t)(c->p.seed >> 32);
    a.tick = c->step;
    const bool tables = c->N <= sq::kQm1dRegMaxN;
    if (tables) {  // the field-independent work of the frame, grid-wide ahead of the chain (qm1d_prep_launch)
        const size_t L = (size_t)c->p.loops, nq4 = (size_t)((c->N + 3) & ~3);
        if (!c->qom) {  // all tables as one unit: a failed allocation leaves none behind
            const size_t bxi = sizeof(float) * L * nq4;
            const size_t btcl = c->p.pot == 3 ? sizeof(float) * L * (size_t)(c->N + 2) : 0;
            const size_t bdd = c->p.pot == 3 ? sizeof(double) * L * (size_t)c->N : 0;
            if (bxi + btcl + bdd > sq::kQm1dTableCap)
                return fail(SQ_E_ARG, "QM1D frame tables (loops x N) exceed the device-memory cap "
                                      "(sq::kQm1dTableCap); use fewer loops per frame");
            double *om = nullptr, *dd = nullptr;
            float *xi = nullptr, *tcl = nullptr;
            hipError_t e = hipMalloc(&om, sizeof(double) * (L + 1));
            if (e == hipSuccess) e = hipMalloc(&xi, bxi);
            if (e == hipSuccess && btcl) e = hipMalloc(&tcl, btcl);
            if (e == hipSuccess && bdd) e = hipMalloc(&dd, bdd);
            if (e != hipSuccess) {
                (void)hipFree(om);
                (void)hipFree(xi);
                (void)hipFree(tcl);
                (void)hipFree(dd);
                return fail(SQ_E_HIP, std::string("QM1D frame tables: hipMalloc: ") + hipGetErrorString(e));
            }
            c->qom = om;
            c->qxi = xi;
            c->qtcl = tcl;
            c->qdd = dd;
        }
        a.om = c->qom;
        a.xi = c->qxi;
        a.tcl = c->qtcl;
        a.dd = c->qdd;
    }
    sq::Qm1dState st{};
    st.omega_in = c->omega;
    st.lrgEl = c->lrgEl;
    st.lrgVl = c->lrgVl;
    SQ_HIP(hipMemcpyAsync(c->qst, &st, sizeof st, hipMemcpyHostToDevice, c->qstream));
    // diagnostics (SQ_QM1D_STAMPS=<path>, grid kernel): per-block phase stamps of
    // the frame's first 64 steps, appended to <path> as text (block step t0..t4)
    const char *dpath = getenv("SQ_QM1D_STAMPS");
    const size_t ndbg = (size_t)sq::kQm1dStampBlocks * 64 * 5;  // the kernel stamps no block past these
    struct DbgFree {  // every return path below frees the stamp buffer
        unsigned long long *&p;
        ~DbgFree() {
            if (p) (void)hipFree(p);
        }
    } dbg_free{a.dbg};
    if (dpath && c->N > sq::kQm1dRegMaxN) {
        SQ_HIP(hipMalloc(&a.dbg, ndbg * sizeof(unsigned long long)));
        SQ_HIP(hipMemsetAsync(a.dbg, 0, ndbg * sizeof(unsigned long long), c->qstream));
    }
    EvPair *e = nullptr;
    int rc = ev_begin(c, c->qstream, &e);
    if (rc) return rc;
    if (tables) SQ_HIP(sq::qm1d_prep_launch(a, c->qstream));
    SQ_HIP(sq::qm1d_frame_launch(a, c->qstream));
    if (e) SQ_HIP(hipEventRecord(e->b, c->qstream));
    SQ_HIP(hipMemcpyAsync(&st, c->qst, sizeof st, hipMemcpyDeviceToHost, c->qstream));
    SQ_HIP(hipStreamSynchronize(c->qstream));
    if (a.dbg) {
        std::vector<unsigned long long> h(ndbg);
        SQ_HIP(hipMemcpy(h.data(), a.dbg, ndbg * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (FILE *fp = fopen(dpath, "a")) {
            for (size_t q = 0; q < ndbg / 5; ++q)
                if (h[5 * q])
                    fprintf(fp, "%zu %zu %llu %llu %llu %llu %llu\n", q / 64, q % 64, h[5 * q], h[5 * q + 1],
                            h[5 * q + 2], h[5 * q + 3], h[5 * q + 4]);
            fclose(fp);
        }
    }
    if (st.sync_error)  // qm1d_frame_grid: a grid barrier gave up; nothing of the frame is adopted
        return fail(SQ_E_HIP, "QM1D grid barrier timeout: a block of qm1d_frame_grid never arrived "
                              "(the frame is void, the state is the frame start)");
    c->step += (unsigned long long)c->p.loops;
    c->lrgEl = st.lrgEl;
    c->lrgVl = st.lrgVl;
    c->perf.steps += st.steps_done;
    c->perf.site_updates += (long long)st.steps_done * c->N;
    *stable = st.stable;
    if (st.stable == 1) {  // tauhost.c:506-532
        c->qcur ^= 1;
        c->omega = st.omega_out;
        c->runs += c->p.loops;
    }
    return SQ_OK;
}

}  // namespace sq

extern "C" {

int sq_upload(sq_ctx *c, const double *f, const double *x, const double *xx0, double omega, long runs) {
    if (!c || !f || !x || !xx0) return fail(SQ_E_ARG, "null argument");
    if (is_phi4(c)) return fail(SQ_E_STATE, "sq_upload is for QM1D contexts");
    DeviceGuard g(c->dev);
    const size_t bytes = sizeof(double) * (size_t)c->N;
    SQ_HIP(hipMemcpy(c->qf[c->qcur], f, bytes, hipMemcpyHostToDevice));
    SQ_HIP(hipMemcpy(c->qx[c->qcur], x, bytes, hipMemcpyHostToDevice));
    SQ_HIP(hipMemcpy(c->qxx0[c->qcur], xx0, bytes, hipMemcpyHostToDevice));
    // the reference writes newf = f once, before the first frame (tauhost.c:177-183,319-377)
    if (c->g_nfp) SQ_HIP(hipMemcpy(c->g_nfp, f, bytes, hipMemcpyHostToDevice));
    c->omega = omega;
    c->runs = runs;
    return SQ_OK;
}

int sq_download(sq_ctx *c, double *f, double *x, double *xx0, double *omega, long *runs) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (is_phi4(c)) return fail(SQ_E_STATE, "sq_download is for QM1D contexts");
    DeviceGuard g(c->dev);
    const size_t bytes = sizeof(double) * (size_t)c->N;
    if (f) SQ_HIP(hipMemcpy(f, c->qf[c->qcur], bytes, hipMemcpyDeviceToHost));
    if (x) SQ_HIP(hipMemcpy(x, c->qx[c->qcur], bytes, hipMemcpyDeviceToHost));
    if (xx0) SQ_HIP(hipMemcpy(xx0, c->qxx0[c->qcur], bytes, hipMemcpyDeviceToHost));
    if (omega) *omega = c->omega;
    if (runs) *runs = c->runs;
    return SQ_OK;
}

int sq_qm1d_get_scan(sq_ctx *c, int *lrgEl, double *lrgVl, unsigned long long *tick) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (lrgEl) *lrgEl = c->lrgEl;
    if (lrgVl) *lrgVl = c->lrgVl;
    if (tick) *tick = c->step;
    return SQ_OK;
}

int sq_qm1d_set_scan(sq_ctx *c, int lrgEl, double lrgVl, unsigned long long tick) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (is_phi4(c)) return fail(SQ_E_STATE, "QM1D only");
    if (lrgEl < 0 || lrgEl >= c->N) return fail(SQ_E_ARG, "lrgEl out of range");
    c->lrgEl = lrgEl;
    c->lrgVl = lrgVl;
    c->step = tick;
    return SQ_OK;
}

int sq_qm1d_set_ordering(sq_ctx *c, int ordering) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (is_phi4(c)) return fail(SQ_E_STATE, "QM1D only");
    if (ordering != SQ_ORDER_JACOBI && ordering != SQ_ORDER_SERIAL) return fail(SQ_E_ARG, "unknown ordering");
    if (ordering == SQ_ORDER_SERIAL) {
        if (sq::qm1d_gs_block(c->N) == 0)
            return fail(SQ_E_ARG, "SQ_ORDER_SERIAL supports 2 <= N <= " + std::to_string(sq::kQm1dGsMaxN));
        DeviceGuard g(c->dev);
        if (!c->g_nfp) {
            SQ_HIP(hipMalloc(&c->g_nfp, sizeof(double) * (size_t)c->N));
            SQ_HIP(hipMemcpy(c->g_nfp, c->qf[c->qcur], sizeof(double) * (size_t)c->N, hipMemcpyDeviceToDevice));
        }
    }
    c->order = ordering;
    return SQ_OK;
}

int sq_qm1d_set_lcg_seed(sq_ctx *c, unsigned long long seed) {
    if (!c) return fail(SQ_E_ARG, "null context");
    c->lcg_seed = seed;
    return SQ_OK;
}

int sq_qm1d_get_lcg_seed(sq_ctx *c, unsigned long long *seed) {
    if (!c || !seed) return fail(SQ_E_ARG, "null argument");
    *seed = c->lcg_seed;
    return SQ_OK;
}

int sq_qm1d_inject_noise(sq_ctx *c, const double *xi, size_t n) {
    if (!c || !xi) return fail(SQ_E_ARG, "null argument");
    if (is_phi4(c) || c->order != SQ_ORDER_SERIAL) return fail(SQ_E_STATE, "needs a QM1D context in SQ_ORDER_SERIAL");
    const size_t need = (size_t)(c->N + 1) * (size_t)c->p.loops;
    if (n < need) return fail(SQ_E_ARG, "need (N+1)*loops draws, got " + std::to_string(n));
    DeviceGuard g(c->dev);
    int rc = gs_reserve(c);
    if (rc) return rc;
    SQ_HIP(hipMemcpy(c->g_xi, xi, sizeof(double) * need, hipMemcpyHostToDevice));
    c->inject_pending = true;
    return SQ_OK;
}

int sq_qm1d_noise_consumed(sq_ctx *c, unsigned long long *n) {
    if (!c || !n) return fail(SQ_E_ARG, "null argument");
    *n = c->consumed;
    return SQ_OK;
}

}  // extern "C"
