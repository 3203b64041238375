// sq_phi4_ens_mala.hip -- the Metropolis-adjusted Langevin step of the phi^4
// lattice ensemble, in the resident kernel.
//
// One MALA step of replica r at counter s (include/stochquant.h has the
// definition): the proposal p = E(phi) is the Euler update of ens_step at s,
// bit for bit; the energy difference
//   dH = [2 h (S(p) - S(phi)) + 1/2 (sum b^2 - sum a^2)] / sig^2,
//   a = p - phi - h d(phi),  b = phi - p - h d(p),
//   d(f)_x = sum_nb f - 6 f_x - f_x (m2 + lam6 f_x^2),
//   S(f) = (3 + m2 / 2) S2(f) - NN(f) + lam6 / 4 S4(f)
// is formed in double from the two float fields and the float record; the
// uniform u comes from Philox at {0, kStreamAccept << 24, s lo, s hi} under the
// replica's key; the replica then holds p (dH <= 0 or u < exp(-dH)) or keeps
// phi bit for bit.  A proposal whose guard touched a site is rejected, the
// replica's guard flag set.  The counter advances by one whatever the verdict.
//
// The structure is ens_heun's: the lane keeps phi in its registers throughout,
// p lives in an image.  Stage 1 forms p from the phi image, where phi's six
// neighbours are at hand, and takes the lane's share of phi's terms; stage 2
// reads the p image -- the lane's own quad and its six neighbours -- and takes
// p's terms; it needs no noise and writes no field.
//
// Summation order (fixed: the same bits on every call, for any R and however
// the steps are split over calls).  Per site twice the term
//   t(f, o) = 2 h [(3 + m2 / 2) f^2 - f (f_x+ + f_y+ + f_z+) + lam6 / 4 f^4] + 1/2 (o - f - h d(f))^2
// (f the field, o the other one) goes into the lane's one double by two fused
// multiply-adds (mala_site, which states every operation):
//   fw = (f_x+ + f_y+) + f_z+,  nb = ((f_x- + f_y-) + f_z-) + fw,
//   d = fma(-f, fma(lam6, f^2, m2), fma(-6, f, nb)),
//   e = fma(lam6 / 4, f^2 f^2, fma(3 + m2 / 2, f^2, -(f fw))),  r = fma(-h, d, o - f),
//   acc = fma(r, r, acc), acc = fma(4 h, e, acc)
// with both signs flipped for phi.  A lane subtracts the sites of phi in stage
// 1 and adds those of p in stage 2, j ascending and x ascending within a quad;
// the wave by ens_wave_sum; the waves' totals in wave order.  2 sig^2 dH is
// that total: the differences S(p) - S(phi) and b^2 - a^2 are taken lane by
// lane, where both sides are of one size, not between two lattice totals.
//
// The decision needs no round trip through one lane: behind the barrier that
// publishes the waves' totals EVERY lane folds them in the same order, draws
// the same u and reaches the same verdict, so the block branches uniformly and
// nothing is posted or waited for.  Every lane keeps the replica's counts (they
// are block-uniform, scalars); lane 0 writes the step's record and, at the end,
// adds the counts to the replica's counters.
//
// Barriers and LDS hazards per step.  Two images (cur holds phi, oth takes p):
//   stage 1 reads cur, writes the lane's own quads of oth       | barrier A
//   stage 2 reads oth; wave totals to the scratch                | barrier B
//   fold, verdict; accept: the lane reloads its own quads from oth, and the
//   two pointers swap; reject: nothing moves.
// oth is written by stage 1 only, after the barrier B of the step before, which
// every reader of it -- stage 2, the accepting lanes' own-quad reload (the
// lane's own quads, which only that lane writes) -- sits in front of; the
// scratch is written behind barrier A, which every lane passes only after it
// has folded the step before.  Three barriers per step.
// One image: stage 1 forms p in registers from the image of phi | barrier (every
// phi neighbour read is done) | the lane exchanges its own quads, phi back into
// registers, p into the image | barrier A | stage 2, totals | barrier B | fold,
// verdict; accept: own quads reloaded from the image, which already holds p;
// reject: phi written back over the lane's own quads (every p read is in front
// of B) | barrier.  Three barriers per accepted step, four per rejected one.
// A measurement point puts one more barrier in front of its own use of the
// scratch (ens_fold), since a slow wave may still be folding the step's totals.
#include "sq_phi4_ens_launch.h"
#include "sq_phi4_ens_mala_dev.h"  // MalaCoef, mala_site, mala_quad

namespace sq {

namespace {

// Stages 1 and 2 of one MALA step of the lane's K quads.  On return the waves' totals of 2 sig^2 dH and of
// max |p| after the guard lie in the scratch (doubles scr[w], floats behind them), not yet behind a barrier;
// the lane holds phi in c, and p lies in oth (TWO) or in cur (one image, cur == oth).
template <int K, bool TWO>
__device__ __forceinline__ void ens_mala_stages(const Phi4StepArgs &A, const MalaCoef &M, const EnsGeo &g,
                                                float4 (&c)[K], const EnsFlagsPk<K> &fl, float *cur, float *oth,
                                                uint32_t slo, uint32_t shi, double *scr) {
    const int T = blockDim.x;
    double acc = 0.0;
    float am = 0.f;
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
        __syncthreads();  // every wave has read phi
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
    __syncthreads();  // p is in its image
    {
        const float *img = TWO ? oth : cur;
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
    }
    acc = ens_wave_sum(acc);
    am = dpp_all_max_f(am);
    if ((threadIdx.x & 63) == 0) {
        const int w = threadIdx.x >> 6;
        scr[w] = acc;
        reinterpret_cast<float *>(scr + 16)[w] = am;
    }
}

// n MALA steps of replica blockIdx.x (sq_phi4_ens_step_mala): phi4_ens_heun_kernel's arguments, LDS layout and
// work-group shape with W, the counts and the per-step record.  Every replica has sig != 0 (the launcher's
// caller checks).  The measurement code behind the step is that kernel's, of the field held after the verdict.
template <int K, typename... CA>
__global__ __launch_bounds__(kPhi4EnsMaxLanes) void phi4_ens_mala_kernel(const Phi4EnsArgs E, const Phi4EnsMalaArgs W,
                                                                          const int two, const CA... ca) {
    constexpr bool CORR = sizeof...(CA) != 0;
    const int r = blockIdx.x;
    const EnsGeo g = ens_geo(E);
    const Phi4EnsRec rc = E.rec[r];
    const Phi4StepArgs A = ens_step_args(rc, E.clampv);
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
    const unsigned long long s0 = rc.step + E.adv;
    int left = E.every;  // steps until the next measurement
    int rec = 0;
    int nacc = 0, ngrd = 0;  // block-uniform: every lane counts
    for (int t = 0; t < E.nsteps; ++t) {
        const unsigned long long s = s0 + (unsigned long long)t;
        const uint32_t slo = (uint32_t)s, shi = (uint32_t)(s >> 32);
        if (two) ens_mala_stages<K, true>(A, M, g, c, fl, cur, oth, slo, shi, scr);
        else ens_mala_stages<K, false>(A, M, g, c, fl, cur, oth, slo, shi, scr);
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
            double *o3 = W.rec + 3 * ((size_t)t * gridDim.x + (size_t)r);
            o3[0] = dH;
            o3[1] = u;
            o3[2] = (double)v;
        }
        if (two) {
            if (v == 1) {
                float *x = cur;
                cur = oth;
                oth = x;
                const float4 *cur4 = reinterpret_cast<const float4 *>(cur);
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    uint32_t f = fl.get(j);
                    int q = (int)threadIdx.x + j * T;
                    asm volatile("" : "+v"(f), "+v"(q));
                    if (f & kEnsValid) c[j] = cur4[q];
                }
            }
        } else {
            float4 *cur4 = reinterpret_cast<float4 *>(cur);
            if (v == 1) {
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    uint32_t f = fl.get(j);
                    int q = (int)threadIdx.x + j * T;
                    asm volatile("" : "+v"(f), "+v"(q));
                    if (f & kEnsValid) c[j] = cur4[q];
                }
            } else {
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    uint32_t f = fl.get(j);
                    int q = (int)threadIdx.x + j * T;
                    asm volatile("" : "+v"(f), "+v"(q));
                    if (f & kEnsValid) cur4[q] = c[j];
                }
                __syncthreads();  // phi is back in the image
            }
        }
        if ((CORR || E.series != nullptr) && --left == 0) {
            left = E.every;
            __syncthreads();  // every wave has folded the step's totals: the scratch is free
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
    float4 *gf = reinterpret_cast<float4 *>(E.field + (size_t)r * (size_t)(4 * g.Q));
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (fl.get(j) & kEnsValid) gf[(int)threadIdx.x + j * T] = c[j];
    if (threadIdx.x == 0) {
        long long *st = W.stat + 3 * (size_t)r;
        st[0] += (long long)E.nsteps;
        st[1] += (long long)nacc;
        st[2] += (long long)ngrd;
        if (ngrd != 0) E.flags[r] = 1;
    }
}

}  // namespace

hipError_t phi4_ens_mala_launch(const Phi4EnsArgs &a, const Phi4EnsMalaArgs &w, const Phi4EnsCorrArgs *c, int nrep,
                                hipStream_t s) {
    if (!ens_step_ok(a, nrep, c != nullptr) || w.stat == nullptr) return hipErrorInvalidValue;
    if (c != nullptr && !ens_corr_ok(*c)) return hipErrorInvalidValue;
    // the step launches' layouts, each by its own rule
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz, c != nullptr ? a.Lz : 0);
    const Phi4EnsLds l = sh.lds(kPhi4EnsLdsStep, c ? phi4_ens_corr_bytes(a.Lz) : 0);
    int two = l.images == 2;
    Phi4EnsArgs q = a;
    Phi4EnsMalaArgs wq = w;
    Phi4EnsCorrArgs cq = c ? *c : Phi4EnsCorrArgs{};
    void *args[] = {&q, &wq, &two, &cq};  // the plain instances take the first three
    const void *fn = c ? SQ_ENS_KERNEL(sh.K, phi4_ens_mala_kernel, Phi4EnsCorrArgs)
                       : SQ_ENS_KERNEL(sh.K, phi4_ens_mala_kernel);
    return ens_launch(fn, nrep, sh.T, l.bytes, args, s);
}

}  // namespace sq
