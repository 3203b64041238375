// sq_phi4_ens.cpp -- the phi^4 lattice ensemble behind the sq_phi4_ens_* entry
// points of the C ABI: R lattices per launch (sq_phi4_ens.hip).  The host
// keeps every replica's parameters and step counter; the device records hold
// the coefficients derived from them and are rewritten before the next launch
// whenever a setter changed something.  Frames (sq_phi4_ens_run_frames) are
// decided in the kernel; the host mirrors every replica's frame state between
// calls and uploads it before each one.
#include <cmath>
#include <cstring>
#include <vector>

#include "sq_ctx.h"
#include "sq_phi4_ens.h"

using namespace sq;

struct sq_phi4_ens {
    sq_params p{};
    int dev = 0, Lx = 0, Ly = 0, Lz = 0, R = 0;
    size_t sites = 0;
    struct Rep {
        double dtau, m2, lambda, C;
        unsigned long long seed, step;
    };
    std::vector<Rep> rep;                // [R]
    float *field = nullptr;              // [R][Lz][Ly][Lx]
    sq::Phi4EnsRec *rec = nullptr;       // [R]
    int *flags = nullptr;                // [R]
    double *series = nullptr;            // the last step call's records: pinned host memory the kernel writes
    size_t series_cap = 0;               // ... in doubles
    double *mom = nullptr;               // [R][5]
    bool rec_dirty = true;               // the device records are behind rep[]
    std::vector<sq::Phi4EnsFrameState> fst;  // [R] frame state, current between calls
    sq::Phi4EnsFrameState *fst_dev = nullptr;
    float *frecs = nullptr;              // [R][3][loops] the last frame's records (first frames call on)
    int *fr_stable = nullptr;            // [fr_cap][R] a frames call's verdicts ...
    double *fr_dtau = nullptr;           // ... and Δτ
    size_t fr_cap = 0;                   // ... in frames
    unsigned long long adv = 0;          // steps run since the records were written
    int nt = 0;                          // Lz / 2 + 1 correlator distances
    double *cG = nullptr;                // [R][nt] correlator accumulators: zero at creation, cleared by
    double *cS1 = nullptr;               // [R]     sq_phi4_ens_corr_reset only
    long long *cN = nullptr;             // [R]
    double *ctmp = nullptr;              // sq_phi4_ens_slices' device buffer: [count][Lz] then [count][nt]
    size_t ctmp_cap = 0;                 // ... in replicas
    hipStream_t stream = nullptr;
    long long steps_total = 0, launches = 0;
};

namespace {

int ens_range(const sq_phi4_ens *e, int first, int count) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (first < 0 || count < 0 || first > e->R || count > e->R - first)
        return fail(SQ_E_ARG, "replica range outside [0, nrep)");
    return SQ_OK;
}

// What is wrong with a lattice shape, nullptr for a legal one (sq_phi4_ens_create, sq_phi4_ens_shape_info).
const char *ens_dims_error(long long Lx, long long Ly, long long Lz) {
    if (Lx != 8 && Lx != 16 && Lx != 32 && Lx != 64) return "a phi^4 ensemble needs Lx in {8, 16, 32, 64}";
    if (Ly < 2 || Lz < 2) return "a phi^4 ensemble needs Ly >= 2 and Lz >= 2";
    if (Ly > sq::kPhi4EnsMaxSites || Lz > sq::kPhi4EnsMaxSites || Lx * Ly * Lz > sq::kPhi4EnsMaxSites)
        return "a phi^4 ensemble needs Lx Ly Lz <= 32768 sites (one LDS image per lattice)";
    return nullptr;
}

// create_phi4's parameter bound, per replica (the guard needs every update of a
// field inside [-clamp, clamp] to be finite or an infinity, never NaN)
bool ens_params_ok(double cl, double h, double m2, double lambda, double C) {
    const double drift = 12.0 * cl + std::fabs(m2) * cl + std::fabs(lambda) / 6.0 * cl * cl * cl;
    const float clf = (float)cl;
    return std::isfinite(cl) && cl > 0 && std::isfinite(m2) && std::isfinite(lambda) && std::isfinite(C) &&
           std::isfinite(h) && h > 0 && std::isfinite(clf * clf) &&
           h * drift + cl + 16.0 * sqrt(2.0 * h) * std::fabs(C) < 1e30;
}

// phi4_base_args' coefficients (sq_phi4_steps.cpp)
sq::Phi4EnsRec ens_rec(const sq_phi4_ens::Rep &r) {
    sq::Phi4EnsRec d{};
    const float h = (float)r.dtau;
    d.h = h;
    d.m2 = (float)r.m2;
    d.lam6 = (float)((double)(float)r.lambda / 6.0);
    d.sig = (float)(sqrt(2.0 * (double)h) * r.C);
    d.sigq = (float)(sqrt(2.0 * (double)h) * r.C * sq::kSqrt2Ln2);
    d.k0 = (uint32_t)r.seed;
    d.k1 = (uint32_t)(r.seed >> 32);
    d.step = r.step;
    return d;
}

// Bring the device records up to rep[] (the stream is idle: every entry point synchronises it).
int ens_sync_recs(sq_phi4_ens *e) {
    if (!e->rec_dirty) return SQ_OK;
    std::vector<sq::Phi4EnsRec> h((size_t)e->R);
    for (int r = 0; r < e->R; ++r) h[r] = ens_rec(e->rep[r]);
    SQ_HIP(hipMemcpy(e->rec, h.data(), sizeof(sq::Phi4EnsRec) * h.size(), hipMemcpyHostToDevice));
    e->rec_dirty = false;
    e->adv = 0;
    return SQ_OK;
}

sq::Phi4EnsArgs ens_args(const sq_phi4_ens *e) {
    sq::Phi4EnsArgs a{};
    a.field = e->field;
    a.rec = e->rec;
    a.flags = e->flags;
    a.Lx = e->Lx;
    a.Ly = e->Ly;
    a.Lz = e->Lz;
    a.clampv = (float)e->p.clamp;
    a.adv = e->adv;
    return a;
}

void release_phi4_ens(sq_phi4_ens *e) {
    if (e->stream) {
        (void)hipStreamSynchronize(e->stream);
        (void)hipStreamDestroy(e->stream);
        e->stream = nullptr;
    }
    (void)hipFree(e->field);
    (void)hipFree(e->rec);
    (void)hipFree(e->flags);
    (void)hipHostFree(e->series);
    (void)hipFree(e->mom);
    (void)hipFree(e->fst_dev);
    (void)hipFree(e->frecs);
    (void)hipFree(e->fr_stable);
    (void)hipFree(e->fr_dtau);
    (void)hipFree(e->cG);
    (void)hipFree(e->cS1);
    (void)hipFree(e->cN);
    (void)hipFree(e->ctmp);
    e->cG = e->cS1 = e->ctmp = nullptr;
    e->cN = nullptr;
    e->ctmp_cap = 0;
    e->fst_dev = nullptr;
    e->frecs = nullptr;
    e->fr_stable = nullptr;
    e->fr_dtau = nullptr;
    e->fr_cap = 0;
    e->field = nullptr;
    e->rec = nullptr;
    e->flags = nullptr;
    e->series = e->mom = nullptr;
    e->series_cap = 0;
}

sq::Phi4EnsCorrArgs ens_corr_args(const sq_phi4_ens *e) {
    sq::Phi4EnsCorrArgs c{};
    c.G = e->cG;
    c.S1 = e->cS1;
    c.nmeas = e->cN;
    return c;
}

// sq_phi4_ens_step (corr = false) and sq_phi4_ens_step_corr (corr = true; every >= 1 checked by the caller)
int ens_step(sq_phi4_ens *e, int nsteps, int every, double *series, bool corr) {
    if (nsteps == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    int rc = ens_sync_recs(e);
    if (rc) return rc;
    const size_t nrec = (every > 0 && series) ? (size_t)(nsteps / every) : 0;
    const size_t nd = nrec * (size_t)e->R * 4;
    if (nd > e->series_cap) {
        // the records go straight to pinned host memory (32 B per replica and record, posted writes), visible
        // once the stream is idle: a device buffer and its copy back cost a fixed 15-20 us per call (a 200-step
        // call of one 8^3 lattice with every = 20: 24 % over every = 0 with the copy, 13 % without)
        (void)hipHostFree(e->series);
        e->series = nullptr;
        e->series_cap = 0;
        SQ_HIP(hipHostMalloc(&e->series, sizeof(double) * nd, hipHostMallocDefault));
        e->series_cap = nd;
    }
    sq::Phi4EnsArgs a = ens_args(e);
    a.nsteps = nsteps;
    a.every = (nd || corr) ? every : 0;
    a.series = nd ? e->series : nullptr;
    if (corr) SQ_HIP(sq::phi4_ens_step_corr_launch(a, ens_corr_args(e), e->R, e->stream));
    else SQ_HIP(sq::phi4_ens_step_launch(a, e->R, e->stream));
    e->launches++;
    SQ_HIP(hipStreamSynchronize(e->stream));
    if (nd) memcpy(series, e->series, sizeof(double) * nd);
    e->adv += (unsigned long long)nsteps;
    for (auto &r : e->rep) r.step += (unsigned long long)nsteps;
    e->steps_total += (long long)nsteps * e->R;
    return SQ_OK;
}

}  // namespace

extern "C" {

int sq_phi4_ens_create(const sq_params *p, int nrep, const unsigned long long *seeds, sq_phi4_ens **out) {
    if (!p || !out) return fail(SQ_E_ARG, "null argument");
    *out = nullptr;
    if (p->struct_size != (int)sizeof(sq_params)) return fail(SQ_E_ARG, "sq_params size mismatch");
    if (p->model != SQ_MODEL_PHI4) return fail(SQ_E_ARG, "a phi^4 ensemble needs SQ_MODEL_PHI4");
    if (p->comm != SQ_COMM_NONE) return fail(SQ_E_ARG, "a phi^4 ensemble needs SQ_COMM_NONE");
    const long long Lx = p->dims[0], Ly = p->dims[1], Lz = p->dims[2];
    if (const char *why = ens_dims_error(Lx, Ly, Lz)) return fail(SQ_E_ARG, why);
    if (nrep < 1) return fail(SQ_E_ARG, "nrep must be >= 1");
    if (!ens_params_ok(p->clamp, p->deltatau, p->m2, p->lambda, p->C))
        return fail(SQ_E_ARG, "PHI4 parameters must be finite with dtau > 0, clamp^2 finite in fp32 and "
                              "dtau * drift(clamp) < 1e30");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SQ_E_NODEV, "no HIP device");
    if (p->device < 0 || p->device >= ndev) return fail(SQ_E_ARG, "device ordinal out of range");
    DeviceGuard g(p->device);
    sq_phi4_ens *e = new sq_phi4_ens();
    e->p = *p;
    e->dev = p->device;
    e->Lx = (int)Lx;
    e->Ly = (int)Ly;
    e->Lz = (int)Lz;
    e->R = nrep;
    e->sites = (size_t)(Lx * Ly * Lz);
    e->rep.resize((size_t)nrep);
    e->fst.assign((size_t)nrep, sq::Phi4EnsFrameState{});
    for (auto &f : e->fst) f.fired = -1;
    for (int r = 0; r < nrep; ++r)
        e->rep[r] = sq_phi4_ens::Rep{p->deltatau, p->m2, p->lambda, p->C,
                                     seeds ? seeds[r] : p->seed + (unsigned long long)r, 0ull};
    int rc = [&]() -> int {
        const size_t bytes = sizeof(float) * e->sites * (size_t)nrep;
        SQ_HIP(hipMalloc(&e->field, bytes));
        SQ_HIP(hipMalloc(&e->rec, sizeof(sq::Phi4EnsRec) * (size_t)nrep));
        SQ_HIP(hipMalloc(&e->flags, sizeof(int) * (size_t)nrep));
        SQ_HIP(hipMalloc(&e->mom, sizeof(double) * 5 * (size_t)nrep));
        SQ_HIP(hipMalloc(&e->fst_dev, sizeof(sq::Phi4EnsFrameState) * (size_t)nrep));
        e->nt = e->Lz / 2 + 1;
        SQ_HIP(hipMalloc(&e->cG, sizeof(double) * (size_t)e->nt * (size_t)nrep));
        SQ_HIP(hipMalloc(&e->cS1, sizeof(double) * (size_t)nrep));
        SQ_HIP(hipMalloc(&e->cN, sizeof(long long) * (size_t)nrep));
        SQ_HIP(hipMemset(e->cG, 0, sizeof(double) * (size_t)e->nt * (size_t)nrep));
        SQ_HIP(hipMemset(e->cS1, 0, sizeof(double) * (size_t)nrep));
        SQ_HIP(hipMemset(e->cN, 0, sizeof(long long) * (size_t)nrep));
        SQ_HIP(hipMemset(e->field, 0, bytes));
        SQ_HIP(hipMemset(e->flags, 0, sizeof(int) * (size_t)nrep));
        SQ_HIP(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
        SQ_HIP(hipDeviceSynchronize());  // the set-up memsets ran on the null stream
        return ens_sync_recs(e);
    }();
    if (rc) {
        const std::string msg = sq_last_error();
        sq_phi4_ens_destroy(e);
        return fail(rc, msg);
    }
    *out = e;
    return SQ_OK;
}

int sq_phi4_ens_shape_info(const int dims[3], int out[8]) {
    if (!dims || !out) return fail(SQ_E_ARG, "null argument");
    if (const char *why = ens_dims_error(dims[0], dims[1], dims[2])) return fail(SQ_E_ARG, why);
    const sq::Phi4EnsShape s = sq::phi4_ens_shape(dims[0] * dims[1] * dims[2]);
    out[0] = s.K;
    out[1] = s.T;
    out[2] = s.two ? 2 : 1;
    out[3] = s.lds_bytes;
    out[4] = s.fr_two ? 2 : 1;
    out[5] = s.fr_lds_bytes;
    out[6] = s.mom_lds_bytes;
    out[7] = sq::kPhi4EnsLdsBytes;
    return SQ_OK;
}

int sq_phi4_ens_destroy(sq_phi4_ens *e) {
    if (!e) return SQ_OK;
    DeviceGuard g(e->dev);
    release_phi4_ens(e);
    delete e;
    return SQ_OK;
}

int sq_phi4_ens_upload(sq_phi4_ens *e, int first, int count, const float *phi) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!phi) return fail(SQ_E_ARG, "null argument");
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    SQ_HIP(hipMemcpy(e->field + (size_t)first * e->sites, phi, sizeof(float) * (size_t)count * e->sites,
                     hipMemcpyHostToDevice));
    return SQ_OK;
}

int sq_phi4_ens_download(sq_phi4_ens *e, int first, int count, float *phi) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!phi) return fail(SQ_E_ARG, "null argument");
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    SQ_HIP(hipMemcpy(phi, e->field + (size_t)first * e->sites, sizeof(float) * (size_t)count * e->sites,
                     hipMemcpyDeviceToHost));
    return SQ_OK;
}

int sq_phi4_ens_init_field(sq_phi4_ens *e, float amp) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    DeviceGuard g(e->dev);
    int rc = ens_sync_recs(e);
    if (rc) return rc;
    SQ_HIP(sq::phi4_ens_init_launch(ens_args(e), e->R, amp, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_set_params(sq_phi4_ens *e, int first, int count, const double *dtau, const double *m2,
                           const double *lambda, const double *C) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    for (int r = 0; r < count; ++r) {  // all of the range or none of it
        const sq_phi4_ens::Rep &o = e->rep[(size_t)(first + r)];
        if (!ens_params_ok(e->p.clamp, dtau ? dtau[r] : o.dtau, m2 ? m2[r] : o.m2, lambda ? lambda[r] : o.lambda,
                           C ? C[r] : o.C))
            return fail(SQ_E_ARG, "PHI4 parameters must be finite with dtau > 0 and dtau * drift(clamp) < 1e30");
    }
    for (int r = 0; r < count; ++r) {
        sq_phi4_ens::Rep &o = e->rep[(size_t)(first + r)];
        if (dtau) o.dtau = dtau[r];
        if (m2) o.m2 = m2[r];
        if (lambda) o.lambda = lambda[r];
        if (C) o.C = C[r];
    }
    if (count && (dtau || m2 || lambda || C)) e->rec_dirty = true;
    return SQ_OK;
}

int sq_phi4_ens_get_params(sq_phi4_ens *e, int first, int count, double *dtau, double *m2, double *lambda,
                           double *C) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    for (int r = 0; r < count; ++r) {
        const sq_phi4_ens::Rep &o = e->rep[(size_t)(first + r)];
        if (dtau) dtau[r] = o.dtau;
        if (m2) m2[r] = o.m2;
        if (lambda) lambda[r] = o.lambda;
        if (C) C[r] = o.C;
    }
    return SQ_OK;
}

int sq_phi4_ens_get_step(sq_phi4_ens *e, int first, int count, unsigned long long *step) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!step) return fail(SQ_E_ARG, "null argument");
    for (int r = 0; r < count; ++r) step[r] = e->rep[(size_t)(first + r)].step;
    return SQ_OK;
}

int sq_phi4_ens_set_step(sq_phi4_ens *e, int first, int count, const unsigned long long *step) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!step) return fail(SQ_E_ARG, "null argument");
    for (int r = 0; r < count; ++r) e->rep[(size_t)(first + r)].step = step[r];
    if (count) e->rec_dirty = true;
    return SQ_OK;
}

int sq_phi4_ens_step(sq_phi4_ens *e, int nsteps, int every, double *series) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nsteps < 0) return fail(SQ_E_ARG, "nsteps must be >= 0");
    if (every < 0) return fail(SQ_E_ARG, "every must be >= 0");
    return ens_step(e, nsteps, every, series, false);
}

int sq_phi4_ens_step_corr(sq_phi4_ens *e, int nsteps, int every, double *series) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nsteps < 0) return fail(SQ_E_ARG, "nsteps must be >= 0");
    if (every < 1) return fail(SQ_E_ARG, "a correlator measurement needs every >= 1");
    return ens_step(e, nsteps, every, series, true);
}

namespace {
int ens_run_frames(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series, bool corr);
}

int sq_phi4_ens_run_frames(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series) {
    return ens_run_frames(e, nframes, stable, dtau, series, false);
}

int sq_phi4_ens_run_frames_corr(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series) {
    return ens_run_frames(e, nframes, stable, dtau, series, true);
}

}  // extern "C"

namespace {

int ens_run_frames(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series, bool corr) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nframes < 0) return fail(SQ_E_ARG, "nframes < 0");
    if (e->p.loops < 1) return fail(SQ_E_ARG, "frames need loops >= 1");
    if (nframes == 0) return SQ_OK;
    if (!stable || !dtau) return fail(SQ_E_ARG, "null argument");
    DeviceGuard g(e->dev);
    const int L = e->p.loops;
    const size_t R = (size_t)e->R, n = (size_t)nframes;
    int rc = ens_sync_recs(e);
    if (rc) return rc;
    if (!e->frecs) {
        SQ_HIP(hipMalloc(&e->frecs, sizeof(float) * 3 * (size_t)L * R));
        SQ_HIP(hipMemset(e->frecs, 0, sizeof(float) * 3 * (size_t)L * R));
        SQ_HIP(hipDeviceSynchronize());  // the memset ran on the null stream
    }
    if (n > e->fr_cap) {
        (void)hipFree(e->fr_stable);
        (void)hipFree(e->fr_dtau);
        e->fr_stable = nullptr;
        e->fr_dtau = nullptr;
        e->fr_cap = 0;
        SQ_HIP(hipMalloc(&e->fr_stable, sizeof(int) * n * R));
        SQ_HIP(hipMalloc(&e->fr_dtau, sizeof(double) * n * R));
        e->fr_cap = n;
    }
    const size_t nd = series ? n * R * 4 : 0;
    if (nd > e->series_cap) {  // pinned, written by the kernel (sq_phi4_ens_step)
        (void)hipHostFree(e->series);
        e->series = nullptr;
        e->series_cap = 0;
        SQ_HIP(hipHostMalloc(&e->series, sizeof(double) * nd, hipHostMallocDefault));
        e->series_cap = nd;
    }
    for (size_t r = 0; r < R; ++r) {  // a setter may have changed them since the last call
        e->fst[r].dtau = e->rep[r].dtau;
        e->fst[r].C = e->rep[r].C;
    }
    SQ_HIP(hipMemcpyAsync(e->fst_dev, e->fst.data(), sizeof(sq::Phi4EnsFrameState) * R, hipMemcpyHostToDevice,
                          e->stream));
    sq::Phi4EnsArgs a = ens_args(e);
    a.series = nd ? e->series : nullptr;
    sq::Phi4EnsFrameArgs f{};
    f.st = e->fst_dev;
    f.stable = e->fr_stable;
    f.dtau = e->fr_dtau;
    f.recs = e->frecs;
    f.nframes = nframes;
    f.loops = L;
    f.adapt = e->p.adapt_dtau ? 1 : 0;
    if (corr) SQ_HIP(sq::phi4_ens_frames_corr_launch(a, f, ens_corr_args(e), e->R, e->stream));
    else SQ_HIP(sq::phi4_ens_frames_launch(a, f, e->R, e->stream));
    e->launches++;
    SQ_HIP(hipMemcpyAsync(e->fst.data(), e->fst_dev, sizeof(sq::Phi4EnsFrameState) * R, hipMemcpyDeviceToHost,
                          e->stream));
    SQ_HIP(hipMemcpyAsync(stable, e->fr_stable, sizeof(int) * n * R, hipMemcpyDeviceToHost, e->stream));
    SQ_HIP(hipMemcpyAsync(dtau, e->fr_dtau, sizeof(double) * n * R, hipMemcpyDeviceToHost, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    if (nd) memcpy(series, e->series, sizeof(double) * nd);
    for (size_t r = 0; r < R; ++r) {
        e->rep[r].dtau = e->fst[r].dtau;
        e->rep[r].step += (unsigned long long)nframes * (unsigned long long)L;  // rolled-back frames too
        e->steps_total += e->fst[r].exec;
    }
    e->rec_dirty = true;  // Δτ and the counters moved
    return SQ_OK;
}

}  // namespace

extern "C" {

int sq_phi4_ens_corr_sums(sq_phi4_ens *e, int first, int count, double *G, double *S1, long long *nmeas) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    const size_t nt = (size_t)e->nt, n = (size_t)count, f = (size_t)first;
    if (G) SQ_HIP(hipMemcpy(G, e->cG + f * nt, sizeof(double) * n * nt, hipMemcpyDeviceToHost));
    if (S1) SQ_HIP(hipMemcpy(S1, e->cS1 + f, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (nmeas) SQ_HIP(hipMemcpy(nmeas, e->cN + f, sizeof(long long) * n, hipMemcpyDeviceToHost));
    return SQ_OK;
}

int sq_phi4_ens_corr_reset(sq_phi4_ens *e, int first, int count) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    const size_t nt = (size_t)e->nt, n = (size_t)count, f = (size_t)first;
    SQ_HIP(hipMemsetAsync(e->cG + f * nt, 0, sizeof(double) * n * nt, e->stream));
    SQ_HIP(hipMemsetAsync(e->cS1 + f, 0, sizeof(double) * n, e->stream));
    SQ_HIP(hipMemsetAsync(e->cN + f, 0, sizeof(long long) * n, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_slices(sq_phi4_ens *e, int first, int count, double *S, double *g) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0 || (!S && !g)) return SQ_OK;
    DeviceGuard dg(e->dev);
    const size_t nt = (size_t)e->nt, Lz = (size_t)e->Lz, n = (size_t)count;
    if (n > e->ctmp_cap) {
        (void)hipFree(e->ctmp);
        e->ctmp = nullptr;
        e->ctmp_cap = 0;
        SQ_HIP(hipMalloc(&e->ctmp, sizeof(double) * n * (Lz + nt)));
        e->ctmp_cap = n;
    }
    double *devS = e->ctmp, *devg = e->ctmp + n * Lz;
    SQ_HIP(sq::phi4_ens_slices_launch(ens_args(e), first, count, devS, devg, e->stream));
    if (S) SQ_HIP(hipMemcpyAsync(S, devS, sizeof(double) * n * Lz, hipMemcpyDeviceToHost, e->stream));
    if (g) SQ_HIP(hipMemcpyAsync(g, devg, sizeof(double) * n * nt, hipMemcpyDeviceToHost, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_correlator(sq_phi4_ens *e, int connected, double *mean, double *err, int n, int *used) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (n < 0 || n > e->nt) return fail(SQ_E_ARG, "n must lie in [0, Lz / 2 + 1]");
    if (!mean && n > 0) return fail(SQ_E_ARG, "null argument");
    const size_t R = (size_t)e->R, nt = (size_t)e->nt;
    std::vector<double> G(R * nt), S1(R);
    std::vector<long long> N(R);
    int rc = sq_phi4_ens_corr_sums(e, 0, e->R, G.data(), S1.data(), N.data());
    if (rc) return rc;
    int u = 0;
    for (size_t r = 0; r < R; ++r) u += N[r] > 0 ? 1 : 0;
    if (used) *used = u;
    if (u == 0) return fail(SQ_E_STATE, "no replica has a correlator measurement");
    const double V = (double)e->sites, Lz = (double)e->Lz;
    std::vector<double> c((size_t)u);
    for (int t = 0; t < n; ++t) {
        size_t k = 0;
        double sum = 0.0;
        for (size_t r = 0; r < R; ++r) {
            if (N[r] <= 0) continue;
            const double nm = (double)N[r];
            double v = G[r * nt + (size_t)t] / (nm * V);
            if (connected) {
                const double sb = S1[r] / nm;
                v -= sb * sb / (Lz * V);
            }
            c[k++] = v;
            sum += v;
        }
        const double m = sum / (double)u;
        mean[t] = m;
        if (err) {
            double q = 0.0;
            for (int i = 0; i < u; ++i) q += (c[(size_t)i] - m) * (c[(size_t)i] - m);
            err[t] = u > 1 ? sqrt(q / ((double)u * (double)(u - 1))) : 0.0;
        }
    }
    return SQ_OK;
}

int sq_phi4_ens_corr_shape_info(const int dims[3], int out[6]) {
    if (!dims || !out) return fail(SQ_E_ARG, "null argument");
    if (const char *why = ens_dims_error(dims[0], dims[1], dims[2])) return fail(SQ_E_ARG, why);
    const sq::Phi4EnsShape s = sq::phi4_ens_shape(dims[0] * dims[1] * dims[2], dims[2]);
    out[0] = s.co_two ? 2 : 1;
    out[1] = s.co_lds_bytes;
    out[2] = s.co_fr_two ? 2 : 1;
    out[3] = s.co_fr_lds_bytes;
    out[4] = s.sl_lds_bytes;
    out[5] = dims[2] / 2 + 1;
    return SQ_OK;
}

int sq_phi4_ens_stability(sq_phi4_ens *e, int first, int count, double *TV, int *fired, float *M, float *D, float *A,
                          int n) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!M || !D || !A))) return fail(SQ_E_ARG, "bad record arguments");
    if (n > (e->frecs ? e->p.loops : 0)) return fail(SQ_E_ARG, "n exceeds the last frame's steps");
    for (int r = 0; r < count; ++r) {
        const sq::Phi4EnsFrameState &f = e->fst[(size_t)(first + r)];
        if (TV) {
            TV[2 * r] = f.T;
            TV[2 * r + 1] = f.V;
        }
        if (fired) fired[r] = f.fired;
    }
    if (n == 0 || count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    const size_t L = (size_t)e->p.loops;
    std::vector<float> h((size_t)count * 3 * L);
    SQ_HIP(hipMemcpy(h.data(), e->frecs + (size_t)first * 3 * L, sizeof(float) * h.size(), hipMemcpyDeviceToHost));
    float *rows[3] = {M, D, A};
    for (int r = 0; r < count; ++r)
        for (int k = 0; k < 3; ++k)
            memcpy(rows[k] + (size_t)r * (size_t)n, h.data() + ((size_t)r * 3 + (size_t)k) * L, sizeof(float) * (size_t)n);
    return SQ_OK;
}

int sq_phi4_ens_set_stability(sq_phi4_ens *e, int first, int count, const double *T, const double *V) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!T || !V) return fail(SQ_E_ARG, "null argument");
    for (int r = 0; r < count; ++r) {
        sq::Phi4EnsFrameState &f = e->fst[(size_t)(first + r)];
        f.T = (float)T[r];
        f.V = (float)V[r];
        f.init = 1;
    }
    return SQ_OK;
}

int sq_phi4_ens_moments(sq_phi4_ens *e, int first, int count, double *out5) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!out5) return fail(SQ_E_ARG, "null argument");
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    SQ_HIP(sq::phi4_ens_moments_launch(ens_args(e), first, count, e->mom, e->stream));
    SQ_HIP(hipMemcpyAsync(out5, e->mom, sizeof(double) * 5 * (size_t)count, hipMemcpyDeviceToHost, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_flags(sq_phi4_ens *e, int first, int count, int *flags, int clear) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    if (flags) SQ_HIP(hipMemcpy(flags, e->flags + first, sizeof(int) * (size_t)count, hipMemcpyDeviceToHost));
    if (clear) SQ_HIP(hipMemset(e->flags + first, 0, sizeof(int) * (size_t)count));
    if (clear) SQ_HIP(hipDeviceSynchronize());  // the memset ran on the null stream
    return SQ_OK;
}

int sq_phi4_ens_perf(sq_phi4_ens *e, sq_perf_t *out) {
    if (!e || !out) return fail(SQ_E_ARG, "null argument");
    memset(out, 0, sizeof *out);
    out->steps = e->steps_total;
    out->site_updates = e->steps_total * (long long)e->sites;
    out->kernel_launches = e->launches;
    return SQ_OK;
}

}  // extern "C"
