// sq_phi4_ens_hmc.hip -- hybrid Monte Carlo trajectories of the phi^4 lattice
// ensemble, in the resident kernel.
//
// One trajectory of replica r at counter s (include/stochquant.h has the
// definition): L leapfrog steps of step length sig with force -dS / C^2, in
// displacement form, and one Metropolis test.
//   phi_1     = E_s(phi_0), the Euler update of ens_step at s (MALA's proposal);
//   g         = guard(fma(2h, d(phi_k), phi_k)), the noise-off update at 2h,
//   phi_{k+1} = guard(g + (phi_k - phi_{k-1})),  k = 1 .. L - 1;
//   dH = [2 h (S(phi_L) - S(phi_0)) + 1/2 (sum b^2 - sum a^2)] / sig^2,
//   a = phi_1 - phi_0 - h d(phi_0),  b = phi_{L-1} - phi_L - h d(phi_L).
// The uniform u and, with `randomize`, L = 1 + (o.y nleap >> 32) come from the
// one Philox block o at {0, kStreamAccept << 24, s lo, s hi}.  L = 1 is
// phi4_ens_mala_kernel's step, operation for operation.
//
// Where the fields live.  Throughout a trajectory the lane's registers c hold
// its own quads of phi_{k-1} and an LDS image holds phi_k whole: the update of
// a quad reads phi_k -- the quad itself and its six neighbours -- from the
// image, exactly as MALA's stage 2 does, and has phi_{k-1} at hand for the
// displacement.  No instance carries a third field in registers, so the K = 8
// instances need no more of them than MALA's.  phi_0 lies in the replica's row
// of the field in device memory: it is there at the start of the call; a lane
// reads and writes only its own quads of it (no barrier); the row is brought up
// to the field held (`dirty`) in front of the first interior step of a
// trajectory, where c still holds phi_0, and read back by a rejected one.
// Calls with L = 1 throughout never touch the row before the final store.
//
// Barriers and LDS hazards per trajectory.  Two images (cur holds phi_0):
//   stage 1 reads cur, writes the lane's own quads of oth = X   | barrier A
//   interior step k: reads X (phi_k), c <- own quads of phi_k, writes
//     phi_{k+1} to the lane's own quads of Y (which held phi_{k-1}; its last
//     readers sat in front of the barrier of step k - 1, or of A) | barrier,
//     X <-> Y: one barrier per interior step, as a step of ens_step
//   stage 2 reads X (phi_L) against c (phi_{L-1}); wave totals   | barrier B
//   fold, verdict.  Accept: c <- own quads of X, cur = X.  Reject, L = 1:
//   nothing moves.  Reject, L > 1: c <- the row, own quads into X, cur = X
//                                                                 | barrier
// One image: stage 1 as MALA (p in registers | barrier | exchange | barrier A);
// interior step: phi_{k+1} formed into c from the image and c | barrier (every
// read of phi_k is done) | the lane exchanges its own quads, phi_k into c,
// phi_{k+1} into the image | barrier: two per interior step, as ens_step.
// Stage 2, B, fold; accept: c <- own quads of the image; reject: c (L = 1) or
// the row (L > 1) over the lane's own quads | barrier.
//
// Summation order: MALA's.  The lane's one double takes -2 t(phi_0, phi_1) in
// stage 1 and +2 t(phi_L, phi_{L-1}) in stage 2 (mala_site), j ascending and x
// ascending within a quad; nothing is added in between; the wave by
// ens_wave_sum; the waves' totals in wave order.  The guard maximum runs over
// phi_1, every g and every phi_k.
#include "sq_phi4_ens_launch.h"
#include "sq_phi4_ens_mala_dev.h"  // MalaCoef, mala_quad, mala_coef

namespace sq {

namespace {

// Stage 1 (ens_mala_stages' first half): phi_1 from the image of phi_0 and the lane's phi_0 in c, the sites of
// phi_0 subtracted.  On return, behind a barrier, phi_1 lies in oth (TWO) or in cur (one image); c holds phi_0.
template <int K, bool TWO>
__device__ __forceinline__ void ens_hmc_first(const Phi4StepArgs &A, const MalaCoef &M, const EnsGeo &g,
                                              float4 (&c)[K], const EnsFlagsPk<K> &fl, float *cur, float *oth,
                                              uint32_t slo, uint32_t shi, double &acc, float &am) {
    const int T = blockDim.x;
    {
        const float *img = cur;
        const float4 *img4 = reinterpret_cast<const float4 *>(img);
        float4 *oth4 = reinterpret_cast<float4 *>(oth);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            uint32_t f = fl.get(j);
            int q = (int)threadIdx.x + j * T;
            asm volatile("" : "+v"(f), "+v"(q));  // as ens_step
            if (f & kEnsValid) {
                const EnsNbr n = ens_nbr(g, q, f);
                const float4 up = img4[n.up], dn = img4[n.dn], zm = img4[n.zm], zp = img4[n.zp];
                const float lft = img[n.lf], rgt = img[n.rg];
                const f32x4n xi = tb_noise<true>(A, 0u, (uint32_t)q, slo, shi);
                float mp;
                const float4 p = site_update4<true>(c[j], lft, rgt, up, dn, zm, zp, xi, A, false, f32x2{A.m2, A.m2}, &mp);
                am = fmaxf(am, mp);  // after the guard: never NaN
                mala_quad<true>(M, acc, c[j], p, lft, rgt, up, dn, zm, zp);
                if constexpr (TWO) oth4[q] = p;
                else c[j] = p;
            }
        }
    }
    if constexpr (!TWO) {
        __syncthreads();  // every wave has read phi_0
        float4 *cur4 = reinterpret_cast<float4 *>(cur);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            uint32_t f = fl.get(j);
            int q = (int)threadIdx.x + j * T;
            asm volatile("" : "+v"(f), "+v"(q));
            if (f & kEnsValid) {
                const float4 phi = cur4[q];
                cur4[q] = c[j];
                c[j] = phi;
            }
        }
    }
    __syncthreads();  // phi_1 is in its image
}

// One interior step: x holds phi_k, c the lane's phi_{k-1}.  On return, behind a barrier, c holds the lane's
// phi_k and phi_{k+1} lies in y (TWO; the caller swaps the two) or in x (one image).  B: A at step size 2h.
template <int K, bool TWO>
__device__ __forceinline__ void ens_hmc_inner(const Phi4StepArgs &B, const EnsGeo &g, float4 (&c)[K],
                                              const EnsFlagsPk<K> &fl, float *x, float *y, float &am) {
    const int T = blockDim.x;
    const float cl = B.clampv;
    {
        const float *img = x;
        const float4 *img4 = reinterpret_cast<const float4 *>(img);
        float4 *y4 = reinterpret_cast<float4 *>(y);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            uint32_t f = fl.get(j);
            int q = (int)threadIdx.x + j * T;
            asm volatile("" : "+v"(f), "+v"(q));
            if (f & kEnsValid) {
                const EnsNbr n = ens_nbr(g, q, f);
                const float4 p = img4[q];
                const float4 up = img4[n.up], dn = img4[n.dn], zm = img4[n.zm], zp = img4[n.zp];
                const float lft = img[n.lf], rgt = img[n.rg];
                float mp;
                const float4 u = site_update4<false>(p, lft, rgt, up, dn, zm, zp, f32x4n{}, B, false, f32x2{B.m2, B.m2}, &mp);
                float4 o;
                o.x = ens_guard(u.x + (p.x - c[j].x), cl);
                o.y = ens_guard(u.y + (p.y - c[j].y), cl);
                o.z = ens_guard(u.z + (p.z - c[j].z), cl);
                o.w = ens_guard(u.w + (p.w - c[j].w), cl);
                // after the guards: never NaN
                am = fmaxf(fmaxf(am, mp), fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fmaxf(fabsf(o.z), fabsf(o.w))));
                if constexpr (TWO) {
                    y4[q] = o;
                    c[j] = p;
                } else {
                    c[j] = o;
                }
            }
        }
    }
    if constexpr (!TWO) {
        __syncthreads();  // every wave has read phi_k
        float4 *x4 = reinterpret_cast<float4 *>(x);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            uint32_t f = fl.get(j);
            int q = (int)threadIdx.x + j * T;
            asm volatile("" : "+v"(f), "+v"(q));
            if (f & kEnsValid) {
                const float4 phi = x4[q];
                x4[q] = c[j];
                c[j] = phi;
            }
        }
    }
    __syncthreads();  // phi_{k+1} is in its image
}

// Stage 2 (ens_mala_stages' second half): the sites of phi_L, in img, added against the lane's phi_{L-1} in c;
// the waves' totals of 2 sig^2 dH and of the guard maximum to the scratch, not yet behind a barrier.
template <int K>
__device__ __forceinline__ void ens_hmc_last(const MalaCoef &M, const EnsGeo &g, const float4 (&c)[K],
                                             const EnsFlagsPk<K> &fl, const float *img, double acc, float am,
                                             double *scr) {
    const int T = blockDim.x;
    const float4 *img4 = reinterpret_cast<const float4 *>(img);
#pragma unroll
    for (int j = 0; j < K; ++j) {
        uint32_t f = fl.get(j);
        int q = (int)threadIdx.x + j * T;
        asm volatile("" : "+v"(f), "+v"(q));
        if (f & kEnsValid) {
            const EnsNbr n = ens_nbr(g, q, f);
            const float4 p = img4[q];
            const float4 up = img4[n.up], dn = img4[n.dn], zm = img4[n.zm], zp = img4[n.zp];
            const float lft = img[n.lf], rgt = img[n.rg];
            mala_quad<false>(M, acc, p, c[j], lft, rgt, up, dn, zm, zp);
        }
    }
    acc = ens_wave_sum(acc);
    am = dpp_all_max_f(am);
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        scr[w] = acc;
        reinterpret_cast<float *>(scr + 16)[w] = am;
    }
}

// n trajectories of replica blockIdx.x (sq_phi4_ens_step_hmc): phi4_ens_mala_kernel's arguments, LDS layout and
// work-group shape with W in place of the MALA record.  Every replica has sig != 0 (the launcher's caller checks).
// The measurement code behind the verdict is that kernel's, of the field held after the verdict.
template <int K, typename... CA>
__global__ __launch_bounds__(kPhi4EnsMaxLanes) void phi4_ens_hmc_kernel(const Phi4EnsArgs E, const Phi4EnsHmcArgs W,
                                                                         const int two, const CA... ca) {
    constexpr bool CORR = sizeof...(CA) != 0;
    const int r = blockIdx.x;
    const EnsGeo g = ens_geo(E);
    const Phi4EnsRec rc = E.rec[r];
    const Phi4StepArgs A = ens_step_args(rc, E.clampv);
    Phi4StepArgs B = A;  // the interior steps' noise-off update at 2h
    B.h = rc.h + rc.h;
    B.sig = 0.f;
    B.sigq = 0.f;
    const MalaCoef M = mala_coef(rc);
    const double sig2 = readlane_d((double)rc.sig * (double)rc.sig, 0);
    float *cur = reinterpret_cast<float *>(ens_smem);
    float *oth = two ? cur + 4 * g.Q : cur;
    double *scr = reinterpret_cast<double *>(ens_smem + (size_t)(two ? 2 : 1) * 16 * (size_t)g.Q);
    float4 c[K];
    EnsFlagsPk<K> fl;
    {
        uint32_t f[K];
        ens_load<K>(E, g, r, c, f, cur);
        fl.pack(f);
    }
    const int T = blockDim.x;
    const int nw = T >> 6;
    float4 *gf = reinterpret_cast<float4 *>(E.field + (size_t)r * (size_t)(4 * g.Q));
    const unsigned long long s0 = rc.step + E.adv;
    int left = E.every;  // trajectories until the next measurement
    int rec = 0;
    int nacc = 0, ngrd = 0;  // block-uniform: every lane counts
    long long nlf = 0;
    bool dirty = false;  // the replica's row is behind the field held
    for (int t = 0; t < E.nsteps; ++t) {
        const unsigned long long s = s0 + (unsigned long long)t;
        const uint32_t slo = (uint32_t)s, shi = (uint32_t)(s >> 32);
        int L = W.nleap;
        if (W.randomize) {
            const u32x4 o = philox4x32_10(u32x4{0u, kStreamAccept << 24, slo, shi}, rc.k0, rc.k1);
            L = 1 + (int)(((unsigned long long)o.y * (unsigned long long)(uint32_t)W.nleap) >> 32);
        }
        L = __builtin_amdgcn_readfirstlane(L);
        nlf += L;
        double acc = 0.0;
        float am = 0.f;
        float *x = oth;  // the image of phi_k
        if (two) ens_hmc_first<K, true>(A, M, g, c, fl, cur, oth, slo, shi, acc, am);
        else ens_hmc_first<K, false>(A, M, g, c, fl, cur, oth, slo, shi, acc, am);
        if (L > 1) {
            if (dirty) {  // c holds phi_0
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    uint32_t f = fl.get(j);
                    int q = (int)threadIdx.x + j * T;
                    asm volatile("" : "+v"(f), "+v"(q));
                    if (f & kEnsValid) gf[q] = c[j];
                }
                dirty = false;
            }
            float *y = cur;
            for (int k = 1; k < L; ++k) {
                if (two) {
                    ens_hmc_inner<K, true>(B, g, c, fl, x, y, am);
                    float *z = x;
                    x = y;
                    y = z;
                } else {
                    ens_hmc_inner<K, false>(B, g, c, fl, x, y, am);
                }
            }
        }
        ens_hmc_last<K>(M, g, c, fl, x, acc, am, scr);
        __syncthreads();  // the waves' totals are in the scratch
        double tot = 0.0;
        float mx = 0.f;
        {
            const float *scm = reinterpret_cast<const float *>(scr + 16);
            for (int k = 0; k < nw; ++k) {
                tot += scr[k];
                mx = fmaxf(mx, scm[k]);
            }
        }
        // every lane holds the same values: scalars, so that the branches below are the block's
        const double dH = readlane_d(0.5 * tot / sig2, 0);
        mx = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(mx)));
        const u32x4 o = philox4x32_10(u32x4{0u, kStreamAccept << 24, slo, shi}, rc.k0, rc.k1);
        const double u = ((double)o.x + 0.5) * 0x1p-32;
        int v = 0;
        if (mx >= E.clampv) v = 2;
        else if (dH <= 0.0) v = 1;
        else if (u < exp(-dH)) v = 1;  // false for a NaN dH
        v = __builtin_amdgcn_readfirstlane(v);
        nacc += v == 1;
        ngrd += v == 2;
        if (threadIdx.x == 0 && W.rec != nullptr) {
            double *o4 = W.rec + 4 * ((size_t)t * gridDim.x + (size_t)r);
            o4[0] = dH;
            o4[1] = u;
            o4[2] = (double)v;
            o4[3] = (double)L;
        }
        float4 *x4 = reinterpret_cast<float4 *>(x);
        if (v == 1) {
            // phi_L is in x
            if (two) {
                oth = x == cur ? oth : cur;
                cur = x;
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                uint32_t f = fl.get(j);
                int q = (int)threadIdx.x + j * T;
                asm volatile("" : "+v"(f), "+v"(q));
                if (f & kEnsValid) c[j] = x4[q];
            }
            dirty = true;
        } else if (L > 1) {
            // phi_0 from the row over the lane's own quads of x, which becomes the image of the field held
            if (two) {
                oth = x == cur ? oth : cur;
                cur = x;
            }
#pragma unroll
            for (int j = 0; j < K; ++j) {
                uint32_t f = fl.get(j);
                int q = (int)threadIdx.x + j * T;
                asm volatile("" : "+v"(f), "+v"(q));
                if (f & kEnsValid) {
                    c[j] = gf[q];
                    x4[q] = c[j];
                }
            }
            __syncthreads();  // phi_0 is back in the image
        } else if (!two) {
            // L = 1, one image: c holds phi_0, the image phi_1
#pragma unroll
            for (int j = 0; j < K; ++j) {
                uint32_t f = fl.get(j);
                int q = (int)threadIdx.x + j * T;
                asm volatile("" : "+v"(f), "+v"(q));
                if (f & kEnsValid) x4[q] = c[j];
            }
            __syncthreads();  // phi_0 is back in the image
        }
        if ((CORR || E.series != nullptr) && --left == 0) {
            left = E.every;
            __syncthreads();  // every wave has folded the trajectory's totals: the scratch is free
            if (!CORR || E.series != nullptr) {
                double sm[4];
                float mxs;
                uint32_t f[K];
#pragma unroll
                for (int j = 0; j < K; ++j) f[j] = fl.get(j);
                ens_sums<K>(g, c, f, cur, sm, mxs);
                ens_fold(sm, mxs, scr, E.series + 4 * ((size_t)rec * gridDim.x + (size_t)r), false);
                ++rec;
            }
            if constexpr (CORR) {
                const Phi4EnsCorrArgs C = ens_corr_args(ca...);
                ens_corr<true>(g, E.Lz, cur, scr + kPhi4EnsScratchBytes / 8, C.G + (size_t)r * (size_t)(E.Lz / 2 + 1),
                               C.S1 + r, C.nmeas + r, nullptr);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
        uint32_t f = fl.get(j);
        int q = (int)threadIdx.x + j * T;
        asm volatile("" : "+v"(f), "+v"(q));  // the row's addresses are formed where they are used, not kept
        if (f & kEnsValid) gf[q] = c[j];
    }
    if (threadIdx.x == 0) {
        long long *st = W.stat + 4 * (size_t)r;
        st[0] += (long long)E.nsteps;
        st[1] += (long long)nacc;
        st[2] += (long long)ngrd;
        st[3] += nlf;
        if (ngrd != 0) E.flags[r] = 1;
    }
}

}  // namespace

hipError_t phi4_ens_hmc_launch(const Phi4EnsArgs &a, const Phi4EnsHmcArgs &w, const Phi4EnsCorrArgs *c, int nrep,
                               hipStream_t s) {
    if (!ens_step_ok(a, nrep, c != nullptr) || w.stat == nullptr || w.nleap < 1 || w.nleap > kPhi4EnsMaxLeap)
        return hipErrorInvalidValue;
    if (c != nullptr && !ens_corr_ok(*c)) return hipErrorInvalidValue;
    // the step launches' layouts, each by its own rule
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz, c != nullptr ? a.Lz : 0);
    const Phi4EnsLds l = sh.lds(kPhi4EnsLdsStep, c ? phi4_ens_corr_bytes(a.Lz) : 0);
    int two = l.images == 2;
    Phi4EnsArgs q = a;
    Phi4EnsHmcArgs wq = w;
    Phi4EnsCorrArgs cq = c ? *c : Phi4EnsCorrArgs{};
    void *args[] = {&q, &wq, &two, &cq};  // the plain instances take the first three
    const void *fn = c ? SQ_ENS_KERNEL(sh.K, phi4_ens_hmc_kernel, Phi4EnsCorrArgs)
                       : SQ_ENS_KERNEL(sh.K, phi4_ens_hmc_kernel);
    return ens_launch(fn, nrep, sh.T, l.bytes, args, s);
}

}  // namespace sq
