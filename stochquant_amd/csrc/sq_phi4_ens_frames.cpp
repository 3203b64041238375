// sq_phi4_ens_frames.cpp -- the phi^4 ensemble's frames (sq_phi4_ens_run_frames*).  Frames are decided in the
// kernel; the host mirrors every replica's frame state between calls and uploads it before each one.
#include "sq_phi4_ens_host.h"

using namespace sq;

namespace sq {

int ens_run_frames(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series, int measure, int scheme) {
    const bool corr = (measure & kEnsCorr) != 0, pcorr = (measure & kEnsMom) != 0, flow = (measure & kEnsFlow) != 0;
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nframes < 0) return fail(SQ_E_ARG, "nframes < 0");
    if (e->p.loops < 1) return fail(SQ_E_ARG, "frames need loops >= 1");
    if (pcorr && e->pM == 0) return fail(SQ_E_STATE, "no momenta set (sq_phi4_ens_set_momenta)");
    if (nframes == 0) return SQ_OK;
    if (!stable || !dtau) return fail(SQ_E_ARG, "null argument");
    DeviceGuard g(e->dev);
    const bool heun = scheme == SQ_SCHEME_HEUN;
    const int L = e->p.loops;
    const size_t R = (size_t)e->R, n = (size_t)nframes;
    int rc = ens_sync_recs(e);
    if (!rc && flow) rc = ens_sync_flow(e);
    if (!rc) rc = ens_zeroed(e->frecs, 3 * (size_t)L * R);
    if (!rc) rc = ens_reserve(e->fr_stable, n * R);
    if (!rc) rc = ens_reserve(e->fr_dtau, n * R);
    const size_t nd = series ? n * (flow ? (size_t)e->fF : 1) * R * 4 : 0;
    if (!rc) rc = ens_reserve(e->series, nd);
    if (rc) return rc;
    for (size_t r = 0; r < R; ++r) {  // a setter may have changed them since the last call
        e->fst[r].dtau = e->rep[r].dtau;
        e->fst[r].C = e->rep[r].C;
    }
    SQ_HIP(hipMemcpyAsync(e->fst_dev.data(), e->fst.data(), sizeof(sq::Phi4EnsFrameState) * R, hipMemcpyHostToDevice,
                          e->stream));
    sq::Phi4EnsArgs a = ens_args(e);
    a.series = nd ? e->series.data() : nullptr;
    sq::Phi4EnsFrameArgs f{};
    f.st = e->fst_dev.data();
    f.stable = e->fr_stable.data();
    f.dtau = e->fr_dtau.data();
    f.recs = e->frecs.data();
    f.nframes = nframes;
    f.loops = L;
    f.adapt = e->p.adapt_dtau ? 1 : 0;
    if (flow) {
        SQ_HIP(sq::phi4_ens_frames_flow_launch(a, f, ens_flow_args(e), corr, heun, e->R, e->stream));
    } else if (heun) {
        const sq::Phi4EnsCorrArgs c = ens_corr_args(e);
        const sq::Phi4EnsPCorrArgs p = pcorr ? ens_pcorr_args(e, corr) : sq::Phi4EnsPCorrArgs{};
        SQ_HIP(sq::phi4_ens_heun_frames_launch(a, f, (corr && !pcorr) ? &c : nullptr, pcorr ? &p : nullptr, e->R,
                                               e->stream));
    } else if (pcorr) SQ_HIP(sq::phi4_ens_frames_pcorr_launch(a, f, ens_pcorr_args(e, corr), e->R, e->stream));
    else if (corr) SQ_HIP(sq::phi4_ens_frames_corr_launch(a, f, ens_corr_args(e), e->R, e->stream));
    else SQ_HIP(sq::phi4_ens_frames_launch(a, f, e->R, e->stream));
    e->launches++;
    SQ_HIP(hipMemcpyAsync(e->fst.data(), e->fst_dev.data(), sizeof(sq::Phi4EnsFrameState) * R, hipMemcpyDeviceToHost,
                          e->stream));
    SQ_HIP(hipMemcpyAsync(stable, e->fr_stable.data(), sizeof(int) * n * R, hipMemcpyDeviceToHost, e->stream));
    SQ_HIP(hipMemcpyAsync(dtau, e->fr_dtau.data(), sizeof(double) * n * R, hipMemcpyDeviceToHost, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    if (nd) memcpy(series, e->series.data(), sizeof(double) * nd);
    for (size_t r = 0; r < R; ++r) {
        e->rep[r].dtau = e->fst[r].dtau;
        e->rep[r].step += (unsigned long long)nframes * (unsigned long long)L;  // rolled-back frames too
        e->steps_total += e->fst[r].exec;
    }
    e->rec_dirty = true;  // Δτ and the counters moved
    return SQ_OK;
}

}  // namespace sq

extern "C" {

int sq_phi4_ens_run_frames(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series) {
    return ens_run_frames(e, nframes, stable, dtau, series, 0, SQ_SCHEME_EULER);
}

int sq_phi4_ens_run_frames_corr(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series) {
    return ens_run_frames(e, nframes, stable, dtau, series, kEnsCorr, SQ_SCHEME_EULER);
}

int sq_phi4_ens_run_frames_pcorr(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series,
                                 int correlate) {
    return ens_run_frames(e, nframes, stable, dtau, series, kEnsMom | (correlate ? kEnsCorr : 0), SQ_SCHEME_EULER);
}

int sq_phi4_ens_run_frames_heun(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series,
                                int measure) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (measure & ~3) return fail(SQ_E_ARG, "measure holds bit 0 (correlator) and bit 1 (momenta) only");
    return ens_run_frames(e, nframes, stable, dtau, series, measure, SQ_SCHEME_HEUN);
}

int sq_phi4_ens_run_frames_flow(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series, int correlate,
                                int scheme) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (scheme != SQ_SCHEME_EULER && scheme != SQ_SCHEME_HEUN)
        return fail(SQ_E_ARG, "scheme must be SQ_SCHEME_EULER or SQ_SCHEME_HEUN");
    if (nframes < 0) return fail(SQ_E_ARG, "nframes < 0");
    if (e->p.loops < 1) return fail(SQ_E_ARG, "frames need loops >= 1");
    if (e->fF == 0) return fail(SQ_E_STATE, "no flow set (sq_phi4_ens_set_flow)");
    if (!series && !correlate) return ens_run_frames(e, nframes, stable, dtau, nullptr, 0, scheme);
    const bool heun = scheme == SQ_SCHEME_HEUN;
    const sq::Phi4EnsFramesFlowShape sh = sq::phi4_ens_frames_flow_shape((int)e->sites, e->Lz);
    if (!((sh.mask >> (2 * (heun ? 1 : 0) + (correlate ? 1 : 0))) & 1))
        return fail(SQ_E_ARG, "the lattice shape has no frames-flow launch of this scheme and correlator choice "
                              "(sq_phi4_ens_frames_flow_shape_info)");
    return ens_run_frames(e, nframes, stable, dtau, series, kEnsFlow | (correlate ? kEnsCorr : 0), scheme);
}

int sq_phi4_ens_stability(sq_phi4_ens *e, int first, int count, double *TV, int *fired, float *M, float *D, float *A,
                          int n) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!M || !D || !A))) return fail(SQ_E_ARG, "bad record arguments");
    if (n > (e->frecs.data() ? e->p.loops : 0)) return fail(SQ_E_ARG, "n exceeds the last frame's steps");
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
    SQ_HIP(hipMemcpy(h.data(), e->frecs.data() + (size_t)first * 3 * L, sizeof(float) * h.size(),
                     hipMemcpyDeviceToHost));
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

int sq_phi4_ens_heun_frames_shape_info(const int dims[3], int out[4]) {
    int rc = ens_shape_dims(dims, out);
    if (rc) return rc;
    const sq::Phi4EnsShape s = sq::phi4_ens_shape(dims[0] * dims[1] * dims[2], dims[2]);
    const sq::Phi4EnsLds fr = s.lds(sq::kPhi4EnsLdsFrames);
    out[0] = fr.images;
    out[1] = fr.bytes;
    out[2] = s.pc_ok ? 0xf : 0x3;  // bit m: measure = m runs on this shape; momenta need their LDS region
    out[3] = 0;
    return SQ_OK;
}

int sq_phi4_ens_frames_flow_shape_info(const int dims[3], int out[8]) {
    int rc = ens_shape_dims(dims, out);
    if (rc) return rc;
    const sq::Phi4EnsFramesFlowShape s = sq::phi4_ens_frames_flow_shape(dims[0] * dims[1] * dims[2], dims[2]);
    const int sl = sq::phi4_ens_corr_bytes(dims[2]);
    const sq::Phi4EnsLds fr = s.lds(sq::kPhi4EnsLdsFrames), cofr = s.lds(sq::kPhi4EnsLdsFrames, sl);
    const sq::Phi4EnsLds hs = s.lds(sq::kPhi4EnsLdsStep), cohs = s.lds(sq::kPhi4EnsLdsStep, sl);  // the Heun steps
    out[0] = fr.images;
    out[1] = fr.bytes;
    out[2] = cofr.images;
    out[3] = cofr.bytes;
    out[4] = hs.images | (cohs.images << 8);
    out[5] = cohs.bytes;
    out[6] = s.fr_stash | (s.hfr_stash << 1) | (s.hs_stash << 2);
    out[7] = s.mask;
    return SQ_OK;
}

}  // extern "C"
