// sq_phi4_fields.cpp -- PHI4 field transfer and initialisation, and the
// observables (moments, correlator).
#include <cmath>
#include <cstring>

#include "sq_ctx.h"

using namespace sq;

namespace {

// Before an observable's kernels on stream A: one slab without an exchange
// puts every step on stream A, so stream order suffices; otherwise join.
int observe_join(sq_ctx *c) {
    if (c->slabs.size() == 1 && c->p.comm == SQ_COMM_NONE) return SQ_OK;
    return phi4_join(c);
}

}  // namespace

extern "C" {

int sq_upload_field(sq_ctx *c, const float *phi, size_t count) {
    if (!c || !phi) return fail(SQ_E_ARG, "null argument");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "PHI4 only");
    DeviceGuard g(c->dev);
    const size_t plane = plane_floats(c);
    size_t need = 0;
    for (auto &s : c->slabs) need += (size_t)s.nz * plane;
    if (count != need) return fail(SQ_E_ARG, "field size mismatch");
    SQ_HIP(hipDeviceSynchronize());
    {
        int rc = gate_reset(c);
        if (rc) return rc;
    }
    size_t off = 0;
    for (auto &s : c->slabs) {
        SQ_HIP(hipMemcpy(plane0(c, s, c->cur), phi + off, (size_t)s.nz * plane * sizeof(float),
                         hipMemcpyHostToDevice));
        off += (size_t)s.nz * plane;
    }
    c->field_finite = false;  // the caller's values (NaN / inf / beyond the clamp allowed) meet the full guard
    c->fin_sync = true;
    return SQ_OK;
}

int sq_download_field(sq_ctx *c, float *phi, size_t count) {
    if (!c || !phi) return fail(SQ_E_ARG, "null argument");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "PHI4 only");
    DeviceGuard g(c->dev);
    const size_t plane = plane_floats(c);
    size_t need = 0;
    for (auto &s : c->slabs) need += (size_t)s.nz * plane;
    if (count != need) return fail(SQ_E_ARG, "field size mismatch");
    int rc = phi4_join(c);
    if (!rc) rc = gate_check(c, true);
    if (rc) return rc;
    size_t off = 0;
    for (auto &s : c->slabs) {
        SQ_HIP(hipMemcpy(phi + off, plane0(c, s, c->cur), (size_t)s.nz * plane * sizeof(float),
                         hipMemcpyDeviceToHost));
        off += (size_t)s.nz * plane;
    }
    return SQ_OK;
}

int sq_init_field(sq_ctx *c, float amp) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "PHI4 only");
    DeviceGuard g(c->dev);
    int rc = phi4_join(c);
    if (!rc) rc = gate_reset(c);
    if (rc) return rc;
    for (auto &s : c->slabs)
        SQ_HIP(sq::phi4_init_launch(plane0(c, s, c->cur), c->Lx, c->Ly, s.nz, s.z0, (uint32_t)c->p.seed,
                                    (uint32_t)(c->p.seed >> 32), amp, s.sA));
    c->field_finite = std::isfinite(amp) && std::fabs(amp) * 8.0f < (float)c->p.clamp;
    c->fin_sync = true;
    return phi4_join(c);
}

int sq_init_field_hash(sq_ctx *c, double amp, unsigned long long key) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "PHI4 only");
    if (!std::isfinite(amp) || std::fabs(amp) > 1e30) return fail(SQ_E_ARG, "amp must be finite");
    DeviceGuard g(c->dev);
    int rc = phi4_join(c);
    if (!rc) rc = gate_reset(c);
    if (rc) return rc;
    for (auto &s : c->slabs)
        SQ_HIP(sq::phi4_init_hash_launch(plane0(c, s, c->cur), c->Lx, c->Ly, s.nz, s.z0, key, amp, s.sA));
    c->field_finite = std::fabs(amp) < c->p.clamp;  // |phi| <= |amp| < clamp: every site finite and unclamped
    c->fin_sync = true;
    return phi4_join(c);
}

int sq_moments(sq_ctx *c, double out[3]) {
    if (!c || !out) return fail(SQ_E_ARG, "null argument");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "PHI4 only");
    DeviceGuard g(c->dev);
    int rc = observe_join(c);
    if (rc) return rc;
    const size_t plane = plane_floats(c);
    out[0] = out[1] = out[2] = 0;
    for (auto &s : c->slabs) {
        SQ_HIP(sq::phi4_moments_launch(plane0(c, s, c->cur), (long long)s.nz * (long long)plane,
                                       c->dacc, c->dmax, c->dpart, s.sA));
        double acc[2];
        unsigned int mx;
        SQ_HIP(hipMemcpyAsync(acc, c->dacc, sizeof acc, hipMemcpyDeviceToHost, s.sA));
        SQ_HIP(hipMemcpyAsync(&mx, c->dmax, sizeof mx, hipMemcpyDeviceToHost, s.sA));
        SQ_HIP(hipStreamSynchronize(s.sA));
        float fm;
        memcpy(&fm, &mx, sizeof fm);
        out[0] += acc[0];
        out[1] += acc[1];
        out[2] = std::max(out[2], (double)fm);
    }
    return SQ_OK;
}

int sq_correlator(sq_ctx *c, double *out, int n) {
    if (!c || !out || n < 0) return fail(SQ_E_ARG, "bad argument");
    DeviceGuard g(c->dev);
    if (!is_phi4(c)) {
        if (n > c->N) return fail(SQ_E_ARG, "n > N");
        std::vector<double> x(c->N), xx0(c->N);
        int rc = sq_download(c, nullptr, x.data(), xx0.data(), nullptr, nullptr);
        if (rc) return rc;
        const int mid = c->N / 2;
        for (int i = 0; i < n; ++i) out[i] = xx0[i] - x[i] * x[mid];  // tauhost.c:519-521
        return SQ_OK;
    }
    if (n > c->Lz) return fail(SQ_E_ARG, "n > Lz");
    if (c->p.comm == SQ_COMM_P2P && !c->p2p_ready)
        return fail(SQ_E_STATE, "SQ_COMM_P2P context not connected (sq_p2p_connect)");
    int rc = observe_join(c);
    if (rc) return rc;
    // slice sums S(z) of the whole lattice: every slab writes its planes into a
    // zeroed global-length array; across ranks one RCCL sum all-reduce (the
    // per-frame collective of SURVEY.md §8e)
    const long long Lz = c->Lz;
    std::vector<double> S((size_t)Lz, 0.0);
    if (!c->dslice) SQ_HIP(hipMalloc(&c->dslice, sizeof(double) * (size_t)Lz));
    double *d = c->dslice;
    hipStream_t s0 = c->slabs[0].sA;
    hipError_t e = hipMemsetAsync(d, 0, sizeof(double) * (size_t)Lz, s0);
    for (auto &s : c->slabs) {  // one slab: stream order alone, one synchronisation below
        if (e == hipSuccess && s.sA != s0) e = hipStreamSynchronize(s0);
        if (e == hipSuccess) e = sq::phi4_slices_launch(plane0(c, s, c->cur), c->Lx, c->Ly, s.nz, d + s.z0, s.sA);
        if (e == hipSuccess && s.sA != s0) e = hipStreamSynchronize(s.sA);
    }
    if (e == hipSuccess && per_rank(c->p.comm) && c->p.nranks > 1) {
        // disjoint z ranges, zeros elsewhere: the sum is exact in any order
        if (int rc = rank_allreduce(c, d, (size_t)Lz, sq::P2pRed::kSumF64, s0)) return rc;
    }
    if (e == hipSuccess) e = hipMemcpyAsync(S.data(), d, sizeof(double) * (size_t)Lz, hipMemcpyDeviceToHost, s0);
    if (e == hipSuccess) e = hipStreamSynchronize(s0);
    if (e != hipSuccess) return fail(SQ_E_HIP, hipGetErrorString(e));
    const double vol = (double)c->Lx * c->Ly * (double)Lz;
    for (int t = 0; t < n; ++t) {  // z ascending, the wrap without a modulo per term
        double acc = 0;
        for (long long z = 0; z < Lz - t; ++z) acc += S[z] * S[z + t];
        for (long long z = Lz - t; z < Lz; ++z) acc += S[z] * S[z + t - Lz];
        out[t] = acc / vol;
    }
    return SQ_OK;
}

}  // extern "C"
