// sq_phi4_hmc.hip -- hybrid Monte Carlo trajectories of the single phi^4 lattice
// (sq_phi4_step_hmc): the ensemble's trajectory
// (include/stochquant.h, the block above sq_phi4_ens_step_hmc) for a field that
// lives in device memory instead of registers and LDS.
//
// Three buffers of the context's padded layout.  F holds phi_0 and is written
// only by the commit; P and Q are the trajectory's two.
//   first step   phi_1 = E_s(phi_0): the context's single Euler step, F -> P
//                (phi4_step_kernel, launched by sq_phi4_steps.cpp; not here).
//   interior     phi4_hmc_leap_kernel, k = 1 .. L - 1: g = guard(fma(2h,
//                d(phi_k), phi_k)) is site_update4<false> at step size 2h, then
//                phi_{k+1} = guard(g + (phi_k - phi_{k-1})).  The stencil reads
//                phi_k only; phi_{k-1} is read at the site itself by the lane
//                that writes phi_{k+1} there, so phi_{k+1} goes IN PLACE over
//                phi_{k-1}: no third trajectory buffer, no hazard between
//                blocks, 12 bytes per site (read phi_k, read phi_{k-1}, write).
//   dH terms     phi4_hmc_term_kernel<SUB>: -2 t(phi_0, phi_1) behind the first
//                step (SUB, which also takes max |phi_1| for the trip word) and
//                +2 t(phi_L, phi_{L-1}) behind the last one, mala_site per site.
//   verdict      phi4_hmc_verdict_kernel, one work-group: dH, the Philox block,
//                the verdict, the record row, the statistics, one accept word.
//   commit       phi4_hmc_commit_kernel: phi_L -> F where the accept word says so.
// The host enqueues all of it for every trajectory of a call without reading
// anything back: the verdict stays on the device, which is why the commit is a
// conditional copy and not an exchange of pointers.
//
// The march is phi4_step_kernel's: a wave owns an x-span of 4 QX V sites by R
// rows per lane and marches a z-chunk with planes z-1, z, z+1 of the stencil
// field in a register queue (Slot, load_slot), x-neighbours by DPP, segment
// edges and y-halo rows loaded as that kernel loads them, one buffer descriptor
// per plane with loop-invariant lane offsets.  The other field's float4 at the
// site comes by one 16-byte buffer load per quad, issued ahead of the next
// plane's loads; outputs go out by bstore4 with the offset in the VGPR.
//
// Summation order (what differs from the ensemble's).  A lane adds its sites'
// terms to one double in march order: planes ascending, rows, segments, x
// ascending within a quad.  The wave's 64 lanes by ens_wave_sum (DPP, fixed
// order); the block's 4 waves through LDS in wave order; one double per block
// to partials[block] by a plain store.  The verdict folds each of the two
// arrays in 256 contiguous runs, block index ascending within a run, then the
// runs in order, then SUB + ADD.  No atomics anywhere: the bits of dH depend on
// the shape alone, not on the call or on how calls are split.
//
// The trip word: a lane whose running max of |g| and |phi_{k+1}| (or |phi_1|)
// reaches the clamp stores 1 to it, a plain store of the same value by every
// such lane.  The verdict reads and clears it.  No kernel here draws normals.
#include "sq_phi4_ens_mala_dev.h"  // mala_quad, mala_coef, mala_verdict; sq_phi4.hip's device functions through sq_phi4_ens_dev.h
#include "sq_phi4_hmc.h"
#include "sq_phi4_march_dev.h"  // hmc_march, hmc_plane, hmc_unit

namespace sq {

namespace {

__device__ __forceinline__ float max_abs4(const float4 &v) {
    return fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w)));
}

// One interior leapfrog step.  A.in: phi_k; prev: phi_{k-1}; A.out: phi_{k+1};
// A.h: the float h doubled; A.flag: the trip word.  prev == A.out from the
// second interior step on (in place); the first one reads phi_0 from F, which
// nothing but the commit may write, and starts the second trajectory buffer.
template <int QX, int R, int V, bool MS>
struct LeapBody {
    const Phi4StepArgs &A;
    float am;
    __device__ __forceinline__ void operator()(const Lane<QX, R, V> &L, const Slot<R, V> &P, const Slot<R, V> &C,
                                               const Slot<R, V> &N, const float4 (&prev)[R * V], int z, size_t plane,
                                               uint32_t pbytes) {
        const __amdgpu_buffer_rsrc_t ws = plane_rsrc(A.out, padded_index(A, z), plane, pbytes);
        const float cl = A.clampv;
        auto site = [&](int k, const float4 &c, float lft, float rgt, const float4 &up, const float4 &dn,
                        const float4 &zm, const float4 &zp) {
            float mg;
            const float4 g = site_update4<false>(c, lft, rgt, up, dn, zm, zp, f32x4n{}, A, false, f32x2{A.m2, A.m2}, &mg);
            float4 o;
            o.x = ens_guard(g.x + (c.x - prev[k].x), cl);
            o.y = ens_guard(g.y + (c.y - prev[k].y), cl);
            o.z = ens_guard(g.z + (c.z - prev[k].z), cl);
            o.w = ens_guard(g.w + (c.w - prev[k].w), cl);
            am = fmaxf(fmaxf(am, mg), max_abs4(o));  // after the guards: never NaN
            if (L.rows_ok) bstore4(ws, L.voff[k], o);
        };
        hmc_plane<QX, R, V, MS>(A, L, P, C, N, z, plane, pbytes, site);
    }
};

template <int QX, int R, int V, bool MS>
__global__ __launch_bounds__(256) void phi4_hmc_leap_kernel(const Phi4StepArgs A, const float *prev) {
    const int unit = hmc_unit();
    if (unit >= A.nunits) return;
    LeapBody<QX, R, V, MS> body{A, 0.f};
    hmc_march<QX, R, V, MS>(A, prev, unit, body);
    if (body.am >= A.clampv) *A.flag = 1;
}

// The sites' terms of 2 sig^2 dH: f = A.in with its stencil, o = A.out at the site.
template <int QX, int R, int V, bool MS, bool SUB>
struct TermBody {
    const MalaCoef &M;
    const Phi4StepArgs &A;
    double acc;
    float am;
    __device__ __forceinline__ void operator()(const Lane<QX, R, V> &L, const Slot<R, V> &P, const Slot<R, V> &C,
                                               const Slot<R, V> &N, const float4 (&o)[R * V], int z, size_t plane,
                                               uint32_t pbytes) {
        auto site = [&](int k, const float4 &c, float lft, float rgt, const float4 &up, const float4 &dn,
                        const float4 &zm, const float4 &zp) {
            if (L.rows_ok) mala_quad<SUB>(M, acc, c, o[k], lft, rgt, up, dn, zm, zp);
            if constexpr (SUB) am = fmaxf(am, max_abs4(o[k]));  // phi_1 left the guard: never NaN
        };
        hmc_plane<QX, R, V, MS>(A, L, P, C, N, z, plane, pbytes, site);
    }
};

template <int QX, int R, int V, bool MS, bool SUB>
__global__ __launch_bounds__(256) void phi4_hmc_term_kernel(const Phi4StepArgs A, double *partials) {
    __shared__ double sw[4];
    const int unit = hmc_unit();
    Phi4EnsRec rc{};
    rc.h = A.h;
    rc.m2 = A.m2;
    rc.lam6 = A.lam6;
    const MalaCoef M = mala_coef(rc);
    TermBody<QX, R, V, MS, SUB> body{M, A, 0.0, 0.f};
    if (unit < A.nunits) hmc_march<QX, R, V, MS>(A, A.out, unit, body);
    if (SUB && body.am >= A.clampv) *A.flag = 1;
    const double w = ens_wave_sum(body.acc);
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((sw[0] + sw[1]) + sw[2]) + sw[3];
}

constexpr int kVerdictLanes = 256;

// sum of p[0 .. n) in kVerdictLanes contiguous runs, then the runs in order; every lane returns the total
__device__ __forceinline__ double verdict_fold(const double *p, int n, double *lds) {
    const int t = threadIdx.x, run = (n + kVerdictLanes - 1) / kVerdictLanes;
    double a = 0.0;
    for (int i = t * run; i < min((t + 1) * run, n); ++i) a += p[i];
    __syncthreads();  // the previous fold's readers are done
    lds[t] = a;
    __syncthreads();
    double tot = 0.0;
    for (int k = 0; k < kVerdictLanes; ++k) tot += lds[k];
    return tot;
}

__global__ __launch_bounds__(kVerdictLanes) void phi4_hmc_verdict_kernel(const Phi4HmcVerdictArgs W) {
    __shared__ double lds[kVerdictLanes];
    const double sub = verdict_fold(W.part_sub, W.nblocks, lds);
    const double add = verdict_fold(W.part_add, W.nblocks, lds);
    if (threadIdx.x != 0) return;
    const double sig2 = (double)W.sig * (double)W.sig;
    const double dH = 0.5 * (sub + add) / sig2;
    double u;
    const int v = mala_verdict(dH, [&] { return W.st->trip != 0; }, W.s_lo, W.s_hi, W.k0, W.k1, u);
    if (W.rec != nullptr) {
        W.rec[0] = dH;
        W.rec[1] = u;
        W.rec[2] = (double)v;
        W.rec[3] = (double)W.L;
    }
    W.st->stat[0] += 1;
    W.st->stat[1] += v == 1;
    W.st->stat[2] += v == 2;
    W.st->stat[3] += W.L;
    if (v == 2) W.st->flag = 1;
    W.st->accept = v == 1;
    W.st->trip = 0;
}

// phi_L over phi_0 where the verdict accepted: every block reads the accept word.
__global__ __launch_bounds__(256) void phi4_hmc_commit_kernel(const float4 *src, float4 *dst, size_t n4,
                                                             const Phi4HmcState *st) {
    if (st->accept != 1) return;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) dst[i] = src[i];
}

// KIND 0 the leap kernel, 1 the SUB term kernel, 2 the ADD term kernel
template <int QX, int R, int V, bool MS, int KIND>
const void *hmc_fn() {
    if constexpr (KIND == 0) return (const void *)&phi4_hmc_leap_kernel<QX, R, V, MS>;
    else return (const void *)&phi4_hmc_term_kernel<QX, R, V, MS, KIND == 1>;
}
template <int QX, int V, bool MS, int KIND>
const void *hmc_fn_r(int r) {
    return r == 4 ? hmc_fn<QX, 4, V, MS, KIND>() : r == 2 ? hmc_fn<QX, 2, V, MS, KIND>() : hmc_fn<QX, 1, V, MS, KIND>();
}
// phi4_step_launch's choice of the tile instance
template <int KIND>
const void *hmc_pick(const Phi4Geom &g, bool ms) {
    switch (g.qx) {
    case 64:
        if (g.v == 2) return ms ? hmc_fn_r<64, 2, true, KIND>(g.r) : hmc_fn_r<64, 2, false, KIND>(g.r);
        return ms ? hmc_fn_r<64, 1, true, KIND>(g.r) : hmc_fn_r<64, 1, false, KIND>(g.r);
    case 32: return hmc_fn_r<32, 1, false, KIND>(g.r);
    case 16: return hmc_fn_r<16, 1, false, KIND>(g.r);
    case 8: return hmc_fn_r<8, 1, false, KIND>(g.r);
    case 4: return hmc_fn_r<4, 1, false, KIND>(g.r);
    case 2: return hmc_fn_r<2, 1, false, KIND>(g.r);
    default: return nullptr;
    }
}

bool hmc_args_ok(const Phi4StepArgs &a) {
    return a.in != nullptr && a.out != nullptr && a.in != a.out && a.periodic && a.nunits > 0 && a.zlo == 0 &&
           a.zhi == a.nz && a.zstep == a.zc && a.zc >= 1 && (long long)a.zc * a.nzc >= a.nz && a.gz >= 1 &&
           a.flag != nullptr;
}

}  // namespace

int phi4_hmc_blocks(const Phi4StepArgs &a) { return (a.nunits + 3) / 4; }

hipError_t phi4_hmc_leap_launch(const Phi4StepArgs &a, const Phi4Geom &g, const float *prev, hipStream_t s) {
    const void *fn = hmc_pick<0>(g, a.nxseg > 1);
    if (!hmc_args_ok(a) || fn == nullptr || a.sig != 0.0f || prev == nullptr || prev == a.in) return hipErrorInvalidValue;
    Phi4StepArgs q = a;
    void *args[] = {&q, &prev};
    return hipLaunchKernel(fn, dim3((unsigned)phi4_hmc_blocks(a)), dim3(256), args, 0, s);
}

hipError_t phi4_hmc_term_launch(const Phi4StepArgs &a, const Phi4Geom &g, bool sub, double *partials, hipStream_t s) {
    const void *fn = sub ? hmc_pick<1>(g, a.nxseg > 1) : hmc_pick<2>(g, a.nxseg > 1);
    if (!hmc_args_ok(a) || fn == nullptr || partials == nullptr) return hipErrorInvalidValue;
    Phi4StepArgs q = a;
    void *args[] = {&q, &partials};
    return hipLaunchKernel(fn, dim3((unsigned)phi4_hmc_blocks(a)), dim3(256), args, 0, s);
}

hipError_t phi4_hmc_verdict_launch(const Phi4HmcVerdictArgs &w, hipStream_t s) {
    if (w.part_sub == nullptr || w.part_add == nullptr || w.nblocks < 1 || w.st == nullptr || w.sig == 0.0f || w.L < 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(phi4_hmc_verdict_kernel, dim3(1), dim3(kVerdictLanes), 0, s, w);
    return hipGetLastError();
}

hipError_t phi4_hmc_commit_launch(const float *src, float *dst, size_t n, const Phi4HmcState *st, hipStream_t s) {
    if (src == nullptr || dst == nullptr || st == nullptr || (n & 3) != 0) return hipErrorInvalidValue;
    const size_t n4 = n / 4;
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((n4 + 1023) / 1024, 2048));
    hipLaunchKernelGGL(phi4_hmc_commit_kernel, dim3(grid), dim3(256), 0, s, reinterpret_cast<const float4 *>(src),
                       reinterpret_cast<float4 *>(dst), n4, st);
    return hipGetLastError();
}

}  // namespace sq
