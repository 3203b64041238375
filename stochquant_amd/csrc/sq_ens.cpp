// sq_ens.cpp -- the QM1D replica ensemble behind the sq_ens_* entry points of
// the C ABI: R chains per launch (sq_qm1d_ens.hip).  The per-replica frame
// scalars live in device records the frame kernel reads and writes itself; the
// host keeps no copy, so the getters and setters move records.
#include <cmath>
#include <cstring>

#include "sq_ctx.h"
#include "sq_ens.h"

using namespace sq;

struct sq_ens {
    sq_params p{};
    int dev = 0, N = 0, R = 0;
    double *f = nullptr, *x = nullptr, *xx0 = nullptr;  // [R][N]
    sq::EnsRec *rec = nullptr;                          // [R]
    int *verdict = nullptr;                             // the last sq_ens_run_frames call's slots
    size_t verdict_cap = 0;
    double *corr = nullptr;  // mean | err (2 N)
    hipStream_t stream = nullptr;
    long long launches = 0;
};

namespace {

int ens_range(const sq_ens *e, int first, int count) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (first < 0 || count < 0 || first > e->R || count > e->R - first)
        return fail(SQ_E_ARG, "replica range outside [0, nrep)");
    return SQ_OK;
}

int ens_get_recs(sq_ens *e, int first, int count, std::vector<sq::EnsRec> &h) {
    h.resize((size_t)count);
    if (count) SQ_HIP(hipMemcpy(h.data(), e->rec + first, sizeof(sq::EnsRec) * (size_t)count, hipMemcpyDeviceToHost));
    return SQ_OK;
}

int ens_put_recs(sq_ens *e, int first, const std::vector<sq::EnsRec> &h) {
    if (!h.empty()) SQ_HIP(hipMemcpy(e->rec + first, h.data(), sizeof(sq::EnsRec) * h.size(), hipMemcpyHostToDevice));
    return SQ_OK;
}

}  // namespace

extern "C" {

int sq_ens_create(const sq_params *p, int nrep, const unsigned long long *seeds, sq_ens **out) {
    if (!p || !out) return fail(SQ_E_ARG, "null argument");
    *out = nullptr;
    if (p->struct_size != (int)sizeof(sq_params)) return fail(SQ_E_ARG, "sq_params size mismatch");
    if (p->model != SQ_MODEL_QM1D) return fail(SQ_E_ARG, "an ensemble needs SQ_MODEL_QM1D");
    if (p->dims[0] < 2 || p->dims[0] > sq::kQm1dRegMaxN)
        return fail(SQ_E_ARG, "an ensemble supports 2 <= N <= 4096 (the register kernel's range)");
    if (p->pot != 0 && p->pot != 3) return fail(SQ_E_ARG, "potID must be 0 or 3 (tau_kernel.cl:215-246)");
    if (nrep < 1) return fail(SQ_E_ARG, "nrep must be >= 1");
    if (p->loops < 1) return fail(SQ_E_ARG, "loops must be >= 1");
    if (!(p->deltat > 0)) return fail(SQ_E_ARG, "deltat must be > 0");
    if (!(p->deltatau > 0) || !std::isfinite(p->deltatau)) return fail(SQ_E_ARG, "deltatau must be finite and > 0");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SQ_E_NODEV, "no HIP device");
    if (p->device < 0 || p->device >= ndev) return fail(SQ_E_ARG, "device ordinal out of range");
    DeviceGuard g(p->device);
    sq_ens *e = new sq_ens();
    e->p = *p;
    e->dev = p->device;
    e->N = (int)p->dims[0];
    e->R = nrep;
    int rc = [&]() -> int {
        const size_t bytes = sizeof(double) * (size_t)e->N * (size_t)nrep;
        SQ_HIP(hipMalloc(&e->f, bytes));
        SQ_HIP(hipMalloc(&e->x, bytes));
        SQ_HIP(hipMalloc(&e->xx0, bytes));
        SQ_HIP(hipMalloc(&e->rec, sizeof(sq::EnsRec) * (size_t)nrep));
        SQ_HIP(hipMalloc(&e->corr, sizeof(double) * 2 * (size_t)e->N));
        SQ_HIP(hipMemset(e->f, 0, bytes));
        SQ_HIP(hipMemset(e->x, 0, bytes));
        SQ_HIP(hipMemset(e->xx0, 0, bytes));
        std::vector<sq::EnsRec> h((size_t)nrep);
        for (int r = 0; r < nrep; ++r) {
            const unsigned long long sd = seeds ? seeds[r] : p->seed + (unsigned long long)r;
            h[r] = sq::EnsRec{};
            h[r].dtau = p->deltatau;
            h[r].k0 = (uint32_t)sd;
            h[r].k1 = (uint32_t)(sd >> 32);
        }
        int rc2 = ens_put_recs(e, 0, h);
        if (rc2) return rc2;
        SQ_HIP(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
        SQ_HIP(hipDeviceSynchronize());  // the set-up memsets ran on the null stream
        return SQ_OK;
    }();
    if (rc) {
        const std::string msg = sq_last_error();
        sq_ens_destroy(e);
        return fail(rc, msg);
    }
    *out = e;
    return SQ_OK;
}

int sq_ens_destroy(sq_ens *e) {
    if (!e) return SQ_OK;
    DeviceGuard g(e->dev);
    if (e->stream) {
        (void)hipStreamSynchronize(e->stream);
        (void)hipStreamDestroy(e->stream);
    }
    (void)hipFree(e->f);
    (void)hipFree(e->x);
    (void)hipFree(e->xx0);
    (void)hipFree(e->rec);
    (void)hipFree(e->verdict);
    (void)hipFree(e->corr);
    delete e;
    return SQ_OK;
}

int sq_ens_upload(sq_ens *e, int first, int count, const double *f, const double *x, const double *xx0,
                  const double *omega, const long *runs) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!f) return fail(SQ_E_ARG, "null argument");
    DeviceGuard g(e->dev);
    const size_t off = (size_t)first * (size_t)e->N, bytes = sizeof(double) * (size_t)count * (size_t)e->N;
    if (count == 0) return SQ_OK;
    SQ_HIP(hipMemcpy(e->f + off, f, bytes, hipMemcpyHostToDevice));
    if (x) SQ_HIP(hipMemcpy(e->x + off, x, bytes, hipMemcpyHostToDevice));
    else SQ_HIP(hipMemset(e->x + off, 0, bytes));
    if (xx0) SQ_HIP(hipMemcpy(e->xx0 + off, xx0, bytes, hipMemcpyHostToDevice));
    else SQ_HIP(hipMemset(e->xx0 + off, 0, bytes));
    std::vector<sq::EnsRec> h;
    rc = ens_get_recs(e, first, count, h);
    if (rc) return rc;
    for (int r = 0; r < count; ++r) {
        h[r].omega = omega ? omega[r] : 0.;
        h[r].runs = runs ? (long long)runs[r] : 0;
    }
    return ens_put_recs(e, first, h);
}

int sq_ens_download(sq_ens *e, int first, int count, double *f, double *x, double *xx0, double *omega, long *runs) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    const size_t off = (size_t)first * (size_t)e->N, bytes = sizeof(double) * (size_t)count * (size_t)e->N;
    if (f) SQ_HIP(hipMemcpy(f, e->f + off, bytes, hipMemcpyDeviceToHost));
    if (x) SQ_HIP(hipMemcpy(x, e->x + off, bytes, hipMemcpyDeviceToHost));
    if (xx0) SQ_HIP(hipMemcpy(xx0, e->xx0 + off, bytes, hipMemcpyDeviceToHost));
    if (omega || runs) {
        std::vector<sq::EnsRec> h;
        rc = ens_get_recs(e, first, count, h);
        if (rc) return rc;
        for (int r = 0; r < count; ++r) {
            if (omega) omega[r] = h[r].omega;
            if (runs) runs[r] = (long)h[r].runs;
        }
    }
    return SQ_OK;
}

int sq_ens_get_scan(sq_ens *e, int first, int count, int *lrgEl, double *lrgVl, unsigned long long *tick) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    DeviceGuard g(e->dev);
    std::vector<sq::EnsRec> h;
    rc = ens_get_recs(e, first, count, h);
    if (rc) return rc;
    for (int r = 0; r < count; ++r) {
        if (lrgEl) lrgEl[r] = h[r].lrgEl;
        if (lrgVl) lrgVl[r] = h[r].lrgVl;
        if (tick) tick[r] = h[r].tick;
    }
    return SQ_OK;
}

int sq_ens_set_scan(sq_ens *e, int first, int count, const int *lrgEl, const double *lrgVl,
                    const unsigned long long *tick) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!lrgEl || !lrgVl || !tick) return fail(SQ_E_ARG, "null argument");
    for (int r = 0; r < count; ++r)  // the kernel reads X' at lrgEl: it must name a site
        if (lrgEl[r] < 0 || lrgEl[r] >= e->N) return fail(SQ_E_ARG, "lrgEl out of range");
    DeviceGuard g(e->dev);
    std::vector<sq::EnsRec> h;
    rc = ens_get_recs(e, first, count, h);
    if (rc) return rc;
    for (int r = 0; r < count; ++r) {
        h[r].lrgEl = lrgEl[r];
        h[r].lrgVl = lrgVl[r];
        h[r].tick = tick[r];
    }
    return ens_put_recs(e, first, h);
}

int sq_ens_get_dtau(sq_ens *e, int first, int count, double *dtau) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!dtau) return fail(SQ_E_ARG, "null argument");
    DeviceGuard g(e->dev);
    std::vector<sq::EnsRec> h;
    rc = ens_get_recs(e, first, count, h);
    if (rc) return rc;
    for (int r = 0; r < count; ++r) dtau[r] = h[r].dtau;
    return SQ_OK;
}

int sq_ens_set_dtau(sq_ens *e, int first, int count, const double *dtau) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!dtau) return fail(SQ_E_ARG, "null argument");
    for (int r = 0; r < count; ++r)
        if (!(dtau[r] > 0) || !std::isfinite(dtau[r])) return fail(SQ_E_ARG, "dtau must be finite and > 0");
    DeviceGuard g(e->dev);
    std::vector<sq::EnsRec> h;
    rc = ens_get_recs(e, first, count, h);
    if (rc) return rc;
    for (int r = 0; r < count; ++r) h[r].dtau = dtau[r];
    return ens_put_recs(e, first, h);
}

int sq_ens_run_frames(sq_ens *e, int nframes, int *stable) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nframes < 0) return fail(SQ_E_ARG, "nframes must be >= 0");
    if (nframes == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    const size_t nv = (size_t)nframes * (size_t)e->R;
    if (stable && nv > e->verdict_cap) {
        (void)hipFree(e->verdict);
        e->verdict = nullptr;
        e->verdict_cap = 0;
        SQ_HIP(hipMalloc(&e->verdict, sizeof(int) * nv));
        e->verdict_cap = nv;
    }
    sq::EnsArgs a{};
    a.f = e->f;
    a.x = e->x;
    a.xx0 = e->xx0;
    a.rec = e->rec;
    a.N = e->N;
    a.pot = e->p.pot;
    a.loops = e->p.loops;
    a.adapt = e->p.adapt_dtau ? 1 : 0;
    a.a = e->p.deltat;
    const float fa = (float)e->p.deltat;
    a.a2 = (double)(fa * fa);
    a.C = e->p.C;
    a.kconst = host_intconst(e->p.pot);
    for (int fr = 0; fr < nframes; ++fr) {
        a.verdict = stable ? e->verdict + (size_t)fr * (size_t)e->R : nullptr;
        SQ_HIP(sq::ens_frame_launch(a, e->R, e->stream));
        e->launches++;
    }
    if (stable) SQ_HIP(hipMemcpyAsync(stable, e->verdict, sizeof(int) * nv, hipMemcpyDeviceToHost, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_ens_correlator(sq_ens *e, double *mean, double *err, int n) {
    if (!e || !mean) return fail(SQ_E_ARG, "null argument");
    if (n < 1 || n > e->N) return fail(SQ_E_ARG, "n out of range");
    DeviceGuard g(e->dev);
    SQ_HIP(sq::ens_correlator_launch(e->x, e->xx0, e->N, e->R, n, e->corr, err ? e->corr + e->N : nullptr, e->stream));
    SQ_HIP(hipMemcpyAsync(mean, e->corr, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, e->stream));
    if (err) SQ_HIP(hipMemcpyAsync(err, e->corr + e->N, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_ens_perf(sq_ens *e, sq_perf_t *out) {
    if (!e || !out) return fail(SQ_E_ARG, "null argument");
    DeviceGuard g(e->dev);
    std::vector<sq::EnsRec> h;
    int rc = ens_get_recs(e, 0, e->R, h);
    if (rc) return rc;
    memset(out, 0, sizeof *out);
    for (const sq::EnsRec &r : h) out->steps += r.steps_total;
    out->site_updates = out->steps * e->N;
    out->kernel_launches = e->launches;
    return SQ_OK;
}

}  // extern "C"
