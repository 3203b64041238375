// sq_phi4_ens_flow.cpp -- the phi^4 ensemble's gradient-flow measurements (sq_phi4_ens_flow.hip).  The flow in
// frames is sq_phi4_ens_run_frames_flow (sq_phi4_ens_frames.cpp).
#include "sq_phi4_ens_host.h"

#include "sq_phi4_ens_ckpt_format.h"

using namespace sq;

namespace {

// Replica r's flow coefficients: phi4_base_args' expressions of (eps, m², λ), sig = 0.
sq::Phi4EnsFlowRec ens_flow_rec(const sq_phi4_ens *e, const sq_phi4_ens::Rep &r) {
    sq::Phi4EnsFlowRec d{};
    d.h = (float)e->feps;
    d.m2 = (float)(std::isnan(e->fm2) ? r.m2 : e->fm2);
    d.lam6 = (float)((double)(float)(std::isnan(e->flam) ? r.lambda : e->flam) / 6.0);
    return d;
}

// sq_phi4_ens_step_flow, and with SQ_SCHEME_HEUN sq_phi4_ens_step_flow_heun: the same call with the Heun kernels.
int ens_step_flow(sq_phi4_ens *e, int nsteps, int every, double *series, int correlate, int scheme) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nsteps < 0) return fail(SQ_E_ARG, "nsteps must be >= 0");
    if (every < 1) return fail(SQ_E_ARG, "a flow measurement needs every >= 1");
    if (e->fF == 0) return fail(SQ_E_STATE, "no flow set (sq_phi4_ens_set_flow)");
    if (nsteps == 0) return SQ_OK;
    if (!series && !correlate) return ens_step(e, nsteps, 0, nullptr, 0, scheme);  // nothing to measure
    DeviceGuard g(e->dev);
    int rc = ens_sync_recs(e);
    if (!rc) rc = ens_sync_flow(e);
    if (rc) return rc;
    const size_t nrec = series ? (size_t)(nsteps / every) : 0;
    const size_t nd = nrec * (size_t)e->fF * (size_t)e->R * 4;
    rc = ens_reserve(e->series, nd);
    if (rc) return rc;
    if (!nd && !correlate) return ens_step(e, nsteps, 0, nullptr, 0, scheme);  // an incomplete tail only
    sq::Phi4EnsArgs a = ens_args(e);
    a.nsteps = nsteps;
    a.every = every;
    a.series = nd ? e->series.data() : nullptr;
    if (scheme == SQ_SCHEME_HEUN)
        SQ_HIP(sq::phi4_ens_heun_flow_launch(a, ens_flow_args(e), correlate != 0, e->R, e->stream));
    else SQ_HIP(sq::phi4_ens_step_flow_launch(a, ens_flow_args(e), correlate != 0, e->R, e->stream));
    e->launches++;
    SQ_HIP(hipStreamSynchronize(e->stream));
    if (nd) memcpy(series, e->series.data(), sizeof(double) * nd);
    ens_advance(e, (unsigned long long)nsteps);
    return SQ_OK;
}

}  // namespace

namespace sq {

Phi4EnsFlowArgs ens_flow_args(const sq_phi4_ens *e) {
    sq::Phi4EnsFlowArgs w{};
    w.rec = e->frec.data();
    w.nlev = e->fF;
    for (int l = 0; l < e->fF; ++l) w.lev[l] = e->flev[l];
    w.G = e->fG.data();
    w.S1 = e->fS1.data();
    w.nmeas = e->fN.data();
    return w;
}

int ens_sync_flow(sq_phi4_ens *e) {
    if (e->frec.data() && !e->frec_dirty) return SQ_OK;
    int rc = ens_reserve(e->frec, (size_t)e->R);
    if (rc) return rc;
    std::vector<sq::Phi4EnsFlowRec> h((size_t)e->R);
    for (int r = 0; r < e->R; ++r) h[(size_t)r] = ens_flow_rec(e, e->rep[(size_t)r]);
    SQ_HIP(hipMemcpy(e->frec.data(), h.data(), sizeof(sq::Phi4EnsFlowRec) * h.size(), hipMemcpyHostToDevice));
    e->frec_dirty = false;
    return SQ_OK;
}

int ens_apply_flow(sq_phi4_ens *e, double eps, int nlevels, const int *levels, double fm2, double flam) {
    DeviceGuard g(e->dev);
    const size_t R = (size_t)e->R, nt = (size_t)e->nt, F = (size_t)nlevels;
    if (nlevels > 0) {
        if (R * F * nt > e->fG.cap()) {  // all three or none: a failure leaves the handle as it was
            DevBuf<double> G, S1;
            DevBuf<long long> N;
            if (!G.reserve(R * F * nt) || !S1.reserve(R * F) || !N.reserve(R * F))
                return fail(SQ_E_HIP, "hipMalloc of the flow accumulators failed");
            e->fG = std::move(G);
            e->fS1 = std::move(S1);
            e->fN = std::move(N);
        }
        e->feps = eps;
        e->fm2 = fm2;
        e->flam = flam;
        for (int l = 0; l < nlevels; ++l) e->flev[l] = levels[l];
    }
    e->fF = nlevels;  // the accumulators' layout is [R][F][...] from here on: all of them start over
    e->frec_dirty = true;
    if (F > 0) {
        SQ_HIP(hipMemsetAsync(e->fG.data(), 0, sizeof(double) * R * F * nt, e->stream));
        SQ_HIP(hipMemsetAsync(e->fS1.data(), 0, sizeof(double) * R * F, e->stream));
        SQ_HIP(hipMemsetAsync(e->fN.data(), 0, sizeof(long long) * R * F, e->stream));
        SQ_HIP(hipStreamSynchronize(e->stream));
    }
    return SQ_OK;
}

}  // namespace sq

extern "C" {

int sq_phi4_ens_set_flow(sq_phi4_ens *e, double eps, int nlevels, const int *levels, const double *m2,
                         const double *lambda) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nlevels < 0 || nlevels > SQ_PHI4_ENS_MAX_FLOW_LEVELS)
        return fail(SQ_E_ARG, sq::ckpt::flow_levels_error(nlevels, nullptr));
    const double fm2 = m2 ? *m2 : NAN, flam = lambda ? *lambda : NAN;
    if (nlevels > 0) {
        if (const char *why = sq::ckpt::flow_levels_error(nlevels, levels)) return fail(SQ_E_ARG, why);
        if ((m2 && !std::isfinite(fm2)) || (lambda && !std::isfinite(flam)))
            return fail(SQ_E_ARG, "the flow's m2 and lambda must be finite");
        for (const auto &r : e->rep)  // every replica's flow coefficients or none
            if (!ens_params_ok(e->p.clamp, eps, m2 ? fm2 : r.m2, lambda ? flam : r.lambda, 0.0))
                return fail(SQ_E_ARG, "flow parameters must be finite with eps > 0 and eps * drift(clamp) < 1e30");
    }
    return ens_apply_flow(e, eps, nlevels, levels, fm2, flam);
}

int sq_phi4_ens_get_flow(sq_phi4_ens *e, double *eps, int *nlevels, int *levels, double *m2, double *lambda) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (!nlevels) return fail(SQ_E_ARG, "null argument");
    *nlevels = e->fF;
    if (eps) *eps = e->fF ? e->feps : 0.0;
    if (levels)
        for (int l = 0; l < e->fF; ++l) levels[l] = e->flev[l];
    if (m2) *m2 = e->fF ? e->fm2 : NAN;
    if (lambda) *lambda = e->fF ? e->flam : NAN;
    return SQ_OK;
}

int sq_phi4_ens_step_flow(sq_phi4_ens *e, int nsteps, int every, double *series, int correlate) {
    return ens_step_flow(e, nsteps, every, series, correlate, SQ_SCHEME_EULER);
}

int sq_phi4_ens_step_flow_heun(sq_phi4_ens *e, int nsteps, int every, double *series, int correlate) {
    return ens_step_flow(e, nsteps, every, series, correlate, SQ_SCHEME_HEUN);
}

int sq_phi4_ens_flowed(sq_phi4_ens *e, int first, int count, double *sums, double *S, double *gt) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (e->fF == 0) return fail(SQ_E_STATE, "no flow set (sq_phi4_ens_set_flow)");
    if (count == 0 || (!sums && !S && !gt)) return SQ_OK;
    DeviceGuard dg(e->dev);
    rc = ens_sync_flow(e);
    if (rc) return rc;
    const size_t n = (size_t)count * (size_t)e->fF, Lz = (size_t)e->Lz, nt = (size_t)e->nt;
    rc = ens_reserve(e->ftmp, sizeof(double) * n * (4 + Lz + nt));
    if (rc) return rc;
    double *dsum = reinterpret_cast<double *>(e->ftmp.data()), *dS = dsum + 4 * n, *dg_ = dS + n * Lz;
    SQ_HIP(sq::phi4_ens_flowed_launch(ens_args(e), ens_flow_args(e), first, count, dsum, dS, dg_, e->stream));
    if (sums) SQ_HIP(hipMemcpyAsync(sums, dsum, sizeof(double) * 4 * n, hipMemcpyDeviceToHost, e->stream));
    if (S) SQ_HIP(hipMemcpyAsync(S, dS, sizeof(double) * n * Lz, hipMemcpyDeviceToHost, e->stream));
    if (gt) SQ_HIP(hipMemcpyAsync(gt, dg_, sizeof(double) * n * nt, hipMemcpyDeviceToHost, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_flow_field(sq_phi4_ens *e, int first, int count, int nsteps, float *phi) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (nsteps < 0 || nsteps > SQ_PHI4_ENS_MAX_FLOW_STEPS)
        return fail(SQ_E_ARG, "0 <= nsteps <= SQ_PHI4_ENS_MAX_FLOW_STEPS flow steps");
    if (!phi) return fail(SQ_E_ARG, "null argument");
    if (e->fF == 0) return fail(SQ_E_STATE, "no flow set (sq_phi4_ens_set_flow)");
    if (count == 0) return SQ_OK;
    DeviceGuard dg(e->dev);
    rc = ens_sync_flow(e);
    if (rc) return rc;
    const size_t bytes = sizeof(float) * (size_t)count * e->sites;
    rc = ens_reserve(e->ftmp, bytes);
    if (rc) return rc;
    float *out = reinterpret_cast<float *>(e->ftmp.data());
    SQ_HIP(sq::phi4_ens_flow_field_launch(ens_args(e), ens_flow_args(e), first, count, nsteps, out, e->stream));
    SQ_HIP(hipMemcpyAsync(phi, out, bytes, hipMemcpyDeviceToHost, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_fcorr_sums(sq_phi4_ens *e, int first, int count, double *G, double *S1, long long *nmeas) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (e->fF == 0) return fail(SQ_E_STATE, "no flow set (sq_phi4_ens_set_flow)");
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    const size_t F = (size_t)e->fF, nt = (size_t)e->nt, n = (size_t)count, f = (size_t)first;
    if (G) SQ_HIP(hipMemcpy(G, e->fG.data() + f * F * nt, sizeof(double) * n * F * nt, hipMemcpyDeviceToHost));
    if (S1) SQ_HIP(hipMemcpy(S1, e->fS1.data() + f * F, sizeof(double) * n * F, hipMemcpyDeviceToHost));
    if (nmeas) {  // every level of a replica has the same count: the first one's
        std::vector<long long> N(n * F);
        SQ_HIP(hipMemcpy(N.data(), e->fN.data() + f * F, sizeof(long long) * n * F, hipMemcpyDeviceToHost));
        for (size_t r = 0; r < n; ++r) nmeas[r] = N[r * F];
    }
    return SQ_OK;
}

int sq_phi4_ens_fcorr_reset(sq_phi4_ens *e, int first, int count) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0 || e->fF == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    const size_t F = (size_t)e->fF, nt = (size_t)e->nt, n = (size_t)count, f = (size_t)first;
    SQ_HIP(hipMemsetAsync(e->fG.data() + f * F * nt, 0, sizeof(double) * n * F * nt, e->stream));
    SQ_HIP(hipMemsetAsync(e->fS1.data() + f * F, 0, sizeof(double) * n * F, e->stream));
    SQ_HIP(hipMemsetAsync(e->fN.data() + f * F, 0, sizeof(long long) * n * F, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_fcorrelator(sq_phi4_ens *e, int connected, double *mean, double *err, int n, int *used) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (n < 0 || n > e->nt) return fail(SQ_E_ARG, "n must lie in [0, Lz / 2 + 1]");
    if (!mean && n > 0) return fail(SQ_E_ARG, "null argument");
    if (e->fF == 0) return fail(SQ_E_STATE, "no flow set (sq_phi4_ens_set_flow)");
    const size_t R = (size_t)e->R, nt = (size_t)e->nt, F = (size_t)e->fF;
    std::vector<double> G(R * F * nt), S1(R * F), s1(R);
    std::vector<long long> N(R);
    int rc = sq_phi4_ens_fcorr_sums(e, 0, e->R, G.data(), S1.data(), N.data()), u;
    if (!rc) rc = ens_replicas_used(N, "flow correlator", used, &u);
    if (rc) return rc;
    for (size_t l = 0; l < F; ++l) {  // sq_phi4_ens_correlator's rule, level by level
        for (size_t r = 0; r < R; ++r) s1[r] = S1[r * F + l];
        ens_replica_stats(e, G.data() + l * nt, F * nt, connected ? s1.data() : nullptr, N.data(), u, n,
                          mean + l * (size_t)n, err ? err + l * (size_t)n : nullptr);
    }
    return SQ_OK;
}

int sq_phi4_ens_flow_shape_info(const int dims[3], int out[6]) {
    int rc = ens_shape_dims(dims, out);
    if (rc) return rc;
    const sq::Phi4EnsFlowShape s = sq::phi4_ens_flow_shape(dims[0] * dims[1] * dims[2], dims[2]);
    const sq::Phi4EnsLds st = s.lds(sq::kPhi4EnsLdsStep);
    const sq::Phi4EnsLds co = s.lds(sq::kPhi4EnsLdsStep, sq::phi4_ens_corr_bytes(dims[2]));
    out[0] = st.images;
    out[1] = st.bytes;
    out[2] = co.images;
    out[3] = co.bytes;
    out[4] = co.bytes;  // the flowed launch takes the correlator launch's layout
    out[5] = s.stash;
    return SQ_OK;
}

}  // extern "C"
