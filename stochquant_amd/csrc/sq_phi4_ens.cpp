// sq_phi4_ens.cpp -- the phi^4 lattice ensemble behind the sq_phi4_ens_* entry
// points of the C ABI: R lattices per launch (sq_phi4_ens.hip).  The host
// keeps every replica's parameters and step counter; the device records hold
// the coefficients derived from them and are rewritten before the next launch
// whenever a setter changed something.  This file: the handle, its fields and
// parameters, the Euler and Heun steps, and the helpers every subsystem's file
// uses (sq_phi4_ens_host.h).
#include "sq_phi4_ens_host.h"

#include "sq_phi4_ens_ckpt_format.h"

using namespace sq;

namespace {

// What is wrong with a lattice shape, nullptr for a legal one (sq_phi4_ens_create, the *_shape_info): the rule a
// checkpoint's reader applies as well.
static_assert(sq::ckpt::kMaxSites == sq::kPhi4EnsMaxSites, "one site limit");
const char *ens_dims_error(long long Lx, long long Ly, long long Lz) { return sq::ckpt::dims_error(Lx, Ly, Lz); }

}  // namespace

namespace sq {

int ens_alloc_failed(const char *call) {
    return fail(SQ_E_HIP, std::string(call) + ": " + hipGetErrorString(hipPeekAtLastError()));
}

int ens_range(const sq_phi4_ens *e, int first, int count) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (first < 0 || count < 0 || first > e->R || count > e->R - first)
        return fail(SQ_E_ARG, "replica range outside [0, nrep)");
    return SQ_OK;
}

int ens_shape_dims(const int dims[3], const void *out) {
    if (!dims || !out) return fail(SQ_E_ARG, "null argument");
    if (const char *why = ens_dims_error(dims[0], dims[1], dims[2])) return fail(SQ_E_ARG, why);
    return SQ_OK;
}

bool ens_params_ok(double cl, double h, double m2, double lambda, double C) {
    const double drift = 12.0 * cl + std::fabs(m2) * cl + std::fabs(lambda) / 6.0 * cl * cl * cl;
    const float clf = (float)cl;
    return std::isfinite(cl) && cl > 0 && std::isfinite(m2) && std::isfinite(lambda) && std::isfinite(C) &&
           std::isfinite(h) && h > 0 && std::isfinite(clf * clf) &&
           h * drift + cl + 16.0 * sqrt(2.0 * h) * std::fabs(C) < 1e30;
}

// phi4_base_args' coefficients (sq_phi4_steps.cpp)
Phi4EnsRec ens_rec(const sq_phi4_ens::Rep &r) {
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

int ens_sync_recs(sq_phi4_ens *e) {
    if (!e->rec_dirty) return SQ_OK;
    std::vector<sq::Phi4EnsRec> h((size_t)e->R);
    for (int r = 0; r < e->R; ++r) h[r] = ens_rec(e->rep[r]);
    SQ_HIP(hipMemcpy(e->rec.data(), h.data(), sizeof(sq::Phi4EnsRec) * h.size(), hipMemcpyHostToDevice));
    e->rec_dirty = false;
    e->adv = 0;
    return SQ_OK;
}

Phi4EnsArgs ens_args(const sq_phi4_ens *e) {
    sq::Phi4EnsArgs a{};
    a.field = e->field.data();
    a.rec = e->rec.data();
    a.flags = e->flags.data();
    a.Lx = e->Lx;
    a.Ly = e->Ly;
    a.Lz = e->Lz;
    a.clampv = (float)e->p.clamp;
    a.adv = e->adv;
    return a;
}

int ens_needs_noise(const sq_phi4_ens *e, const char *subject, const char *reason) {
    for (const auto &r : e->rep)
        if (ens_rec(r).sig == 0.0f)
            return fail(SQ_E_STATE, std::string(subject) + " needs C != 0 in every replica (sig = sqrt(2 dtau) C is "
                                                           "zero in fp32): " + reason);
    return SQ_OK;
}

void ens_advance(sq_phi4_ens *e, unsigned long long n) {
    e->adv += n;
    for (auto &r : e->rep) r.step += n;
    e->steps_total += (long long)n * e->R;
}

int ens_read_rows(sq_phi4_ens *e, DevBuf<long long> sq_phi4_ens::*tab, int w, int first, int count, long long *out) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!out) return fail(SQ_E_ARG, "null argument");
    if (count == 0) return SQ_OK;
    const size_t n = (size_t)w * (size_t)count;
    const long long *t = (e->*tab).data();
    if (!t) {
        memset(out, 0, sizeof(long long) * n);
        return SQ_OK;
    }
    DeviceGuard g(e->dev);
    SQ_HIP(hipMemcpy(out, t + (size_t)w * (size_t)first, sizeof(long long) * n, hipMemcpyDeviceToHost));
    return SQ_OK;
}

int ens_clear_rows(sq_phi4_ens *e, DevBuf<long long> sq_phi4_ens::*tab, int w, int first, int count) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0 || !(e->*tab).data()) return SQ_OK;
    DeviceGuard g(e->dev);
    SQ_HIP(hipMemset((e->*tab).data() + (size_t)w * (size_t)first, 0, sizeof(long long) * (size_t)w * (size_t)count));
    SQ_HIP(hipDeviceSynchronize());  // the memset ran on the null stream
    return SQ_OK;
}

int ens_step(sq_phi4_ens *e, int nsteps, int every, double *series, int measure, int scheme) {
    if (nsteps == 0) return SQ_OK;
    const bool corr = (measure & kEnsCorr) != 0, pcorr = (measure & kEnsMom) != 0;
    DeviceGuard g(e->dev);
    int rc = ens_sync_recs(e);
    if (rc) return rc;
    const size_t nrec = (every > 0 && series) ? (size_t)(nsteps / every) : 0;
    const size_t nd = nrec * (size_t)e->R * 4;
    rc = ens_reserve(e->series, nd);
    if (rc) return rc;
    sq::Phi4EnsArgs a = ens_args(e);
    a.nsteps = nsteps;
    a.every = (nd || measure) ? every : 0;
    a.series = nd ? e->series.data() : nullptr;
    if (scheme == SQ_SCHEME_HEUN) {
        const sq::Phi4EnsCorrArgs c = ens_corr_args(e);
        const sq::Phi4EnsPCorrArgs p = pcorr ? ens_pcorr_args(e, corr) : sq::Phi4EnsPCorrArgs{};
        SQ_HIP(sq::phi4_ens_heun_launch(a, (corr && !pcorr) ? &c : nullptr, pcorr ? &p : nullptr, e->R, e->stream));
    } else if (pcorr) SQ_HIP(sq::phi4_ens_step_pcorr_launch(a, ens_pcorr_args(e, corr), e->R, e->stream));
    else if (corr) SQ_HIP(sq::phi4_ens_step_corr_launch(a, ens_corr_args(e), e->R, e->stream));
    else SQ_HIP(sq::phi4_ens_step_launch(a, e->R, e->stream));
    e->launches++;
    SQ_HIP(hipStreamSynchronize(e->stream));
    if (nd) memcpy(series, e->series.data(), sizeof(double) * nd);
    ens_advance(e, (unsigned long long)nsteps);
    return SQ_OK;
}

}  // namespace sq

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
    e->nt = e->Lz / 2 + 1;
    e->rep.resize((size_t)nrep);
    e->fst.assign((size_t)nrep, sq::Phi4EnsFrameState{});
    for (auto &f : e->fst) f.fired = -1;
    for (int r = 0; r < nrep; ++r)
        e->rep[r] = sq_phi4_ens::Rep{p->deltatau, p->m2, p->lambda, p->C,
                                     seeds ? seeds[r] : p->seed + (unsigned long long)r, 0ull};
    int rc = [&]() -> int {
        const size_t R = (size_t)nrep, nf = e->sites * R, nG = (size_t)e->nt * R;
        int rc;
        if ((rc = ens_reserve(e->field, nf)) || (rc = ens_reserve(e->rec, R)) || (rc = ens_reserve(e->flags, R)) ||
            (rc = ens_reserve(e->mom, 5 * R)) || (rc = ens_reserve(e->fst_dev, R)) || (rc = ens_reserve(e->cG, nG)) ||
            (rc = ens_reserve(e->cS1, R)) || (rc = ens_reserve(e->cN, R)))
            return rc;
        SQ_HIP(hipMemset(e->cG.data(), 0, sizeof(double) * nG));
        SQ_HIP(hipMemset(e->cS1.data(), 0, sizeof(double) * R));
        SQ_HIP(hipMemset(e->cN.data(), 0, sizeof(long long) * R));
        if ((rc = ens_reserve(e->pN, R))) return rc;
        SQ_HIP(hipMemset(e->pN.data(), 0, sizeof(long long) * R));
        if ((rc = ens_reserve(e->xstat, 2 * R))) return rc;
        SQ_HIP(hipMemset(e->xstat.data(), 0, sizeof(long long) * 2 * R));
        if ((rc = ens_reserve(e->cstat, 5 * R))) return rc;
        SQ_HIP(hipMemset(e->cstat.data(), 0, sizeof(long long) * 5 * R));
        if ((rc = ens_reserve(e->walker, R))) return rc;
        {
            std::vector<int> id(R);
            for (int r = 0; r < nrep; ++r) id[(size_t)r] = r;
            SQ_HIP(hipMemcpy(e->walker.data(), id.data(), sizeof(int) * R, hipMemcpyHostToDevice));
        }
        SQ_HIP(hipMemset(e->field.data(), 0, sizeof(float) * nf));
        SQ_HIP(hipMemset(e->flags.data(), 0, sizeof(int) * R));
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
    int rc = ens_shape_dims(dims, out);
    if (rc) return rc;
    const sq::Phi4EnsShape s = sq::phi4_ens_shape(dims[0] * dims[1] * dims[2]);
    out[0] = s.K;
    out[1] = s.T;
    const sq::Phi4EnsLds st = s.lds(sq::kPhi4EnsLdsStep), fr = s.lds(sq::kPhi4EnsLdsFrames);
    out[2] = st.images;
    out[3] = st.bytes;
    out[4] = fr.images;
    out[5] = fr.bytes;
    out[6] = s.lds(sq::kPhi4EnsLdsStored).bytes;
    out[7] = sq::kPhi4EnsLdsBytes;
    return SQ_OK;
}

int sq_phi4_ens_destroy(sq_phi4_ens *e) {
    if (!e) return SQ_OK;
    DeviceGuard g(e->dev);
    if (e->stream) {
        (void)hipStreamSynchronize(e->stream);
        (void)hipStreamDestroy(e->stream);
    }
    delete e;  // frees every buffer, on the handle's device
    return SQ_OK;
}

int sq_phi4_ens_upload(sq_phi4_ens *e, int first, int count, const float *phi) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!phi) return fail(SQ_E_ARG, "null argument");
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    SQ_HIP(hipMemcpy(e->field.data() + (size_t)first * e->sites, phi, sizeof(float) * (size_t)count * e->sites,
                     hipMemcpyHostToDevice));
    return SQ_OK;
}

int sq_phi4_ens_download(sq_phi4_ens *e, int first, int count, float *phi) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!phi) return fail(SQ_E_ARG, "null argument");
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    SQ_HIP(hipMemcpy(phi, e->field.data() + (size_t)first * e->sites, sizeof(float) * (size_t)count * e->sites,
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
        // the replica's flow coefficients follow its m² and λ where the flow has none of its own
        if (e->fF > 0 && !ens_params_ok(e->p.clamp, e->feps, std::isnan(e->fm2) ? (m2 ? m2[r] : o.m2) : e->fm2,
                                        std::isnan(e->flam) ? (lambda ? lambda[r] : o.lambda) : e->flam, 0.0))
            return fail(SQ_E_ARG, "the parameters would make the replica's flow coefficients illegal "
                                  "(sq_phi4_ens_set_flow)");
    }
    for (int r = 0; r < count; ++r) {
        sq_phi4_ens::Rep &o = e->rep[(size_t)(first + r)];
        if (dtau) o.dtau = dtau[r];
        if (m2) o.m2 = m2[r];
        if (lambda) o.lambda = lambda[r];
        if (C) o.C = C[r];
    }
    if (count && (dtau || m2 || lambda || C)) e->rec_dirty = true;
    if (count && (m2 || lambda)) e->frec_dirty = true;
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
    return ens_step(e, nsteps, every, series, 0, SQ_SCHEME_EULER);
}

int sq_phi4_ens_step_corr(sq_phi4_ens *e, int nsteps, int every, double *series) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nsteps < 0) return fail(SQ_E_ARG, "nsteps must be >= 0");
    if (every < 1) return fail(SQ_E_ARG, "a correlator measurement needs every >= 1");
    return ens_step(e, nsteps, every, series, kEnsCorr, SQ_SCHEME_EULER);
}

int sq_phi4_ens_step_pcorr(sq_phi4_ens *e, int nsteps, int every, double *series, int correlate) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nsteps < 0) return fail(SQ_E_ARG, "nsteps must be >= 0");
    if (every < 1) return fail(SQ_E_ARG, "a momentum measurement needs every >= 1");
    if (e->pM == 0) return fail(SQ_E_STATE, "no momenta set (sq_phi4_ens_set_momenta)");
    return ens_step(e, nsteps, every, series, kEnsMom | (correlate ? kEnsCorr : 0), SQ_SCHEME_EULER);
}

int sq_phi4_ens_step_heun(sq_phi4_ens *e, int nsteps, int every, double *series, int measure) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nsteps < 0) return fail(SQ_E_ARG, "nsteps must be >= 0");
    if (measure & ~3) return fail(SQ_E_ARG, "measure holds bit 0 (correlator) and bit 1 (momenta) only");
    if (measure ? every < 1 : every < 0)
        return fail(SQ_E_ARG, measure ? "a correlator or momentum measurement needs every >= 1" : "every must be >= 0");
    if ((measure & 2) && e->pM == 0) return fail(SQ_E_STATE, "no momenta set (sq_phi4_ens_set_momenta)");
    return ens_step(e, nsteps, every, series, measure, SQ_SCHEME_HEUN);
}

int sq_phi4_ens_moments(sq_phi4_ens *e, int first, int count, double *out5) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!out5) return fail(SQ_E_ARG, "null argument");
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    SQ_HIP(sq::phi4_ens_moments_launch(ens_args(e), first, count, e->mom.data(), e->stream));
    SQ_HIP(hipMemcpyAsync(out5, e->mom.data(), sizeof(double) * 5 * (size_t)count, hipMemcpyDeviceToHost, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_flags(sq_phi4_ens *e, int first, int count, int *flags, int clear) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    if (flags) SQ_HIP(hipMemcpy(flags, e->flags.data() + first, sizeof(int) * (size_t)count, hipMemcpyDeviceToHost));
    if (clear) SQ_HIP(hipMemset(e->flags.data() + first, 0, sizeof(int) * (size_t)count));
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
