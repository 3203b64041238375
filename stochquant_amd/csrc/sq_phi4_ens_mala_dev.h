// sq_phi4_ens_mala_dev.h -- the device functions the Metropolis kernels share
// (sq_phi4_ens_mala.hip, sq_phi4_ens_hmc.hip): the per-site
// term of 2 sig^2 dH in double.  The head of sq_phi4_ens_mala.hip states the
// term and the order of summation.
#pragma once
#include "sq_phi4_ens_dev.h"

namespace sq {

namespace {

struct MalaCoef {  // block-uniform, the float record in double
    double h, h4, km, l4, m2, lam6;
};

// acc +- 2 t(f, o), the site's term of 2 sig^2 dH (see the head of sq_phi4_ens_mala.hip); o: the other field at
// the site.  Fused multiply-adds where that head writes them: 17 double operations per site (the vector fp64
// rate is what a MALA step costs beyond a Heun step).
template <bool SUB>
__device__ __forceinline__ void mala_site(const MalaCoef &M, double &acc, double f, double o, double xm, double xp,
                                          double ym, double yp, double zm, double zp) {
#pragma clang fp contract(off)
    const double f2 = f * f;
    const double fw = (xp + yp) + zp;
    const double nb = ((xm + ym) + zm) + fw;
    const double lap = __builtin_fma(-6.0, f, nb);
    const double g = __builtin_fma(M.lam6, f2, M.m2);
    const double d = __builtin_fma(-f, g, lap);
    const double e = __builtin_fma(M.l4, f2 * f2, __builtin_fma(M.km, f2, -(f * fw)));
    const double t = __builtin_fma(-M.h, d, o - f);
    acc = __builtin_fma(SUB ? -t : t, t, acc);
    acc = __builtin_fma(SUB ? -M.h4 : M.h4, e, acc);
}

template <bool SUB>
__device__ __forceinline__ void mala_quad(const MalaCoef &M, double &acc, const float4 &f, const float4 &o, float lft,
                                          float rgt, const float4 &up, const float4 &dn, const float4 &zm,
                                          const float4 &zp) {
    // one site after the other (the scheduler would otherwise convert the quad's 26 floats at once and keep
    // four sites' doubles in flight: the K = 8 instances have no registers for that)
    __builtin_amdgcn_sched_barrier(0);
    mala_site<SUB>(M, acc, f.x, o.x, lft, f.y, up.x, dn.x, zm.x, zp.x);
    __builtin_amdgcn_sched_barrier(0);
    mala_site<SUB>(M, acc, f.y, o.y, f.x, f.z, up.y, dn.y, zm.y, zp.y);
    __builtin_amdgcn_sched_barrier(0);
    mala_site<SUB>(M, acc, f.z, o.z, f.y, f.w, up.z, dn.z, zm.z, zp.z);
    __builtin_amdgcn_sched_barrier(0);
    mala_site<SUB>(M, acc, f.w, o.w, f.z, rgt, up.w, dn.w, zm.w, zp.w);
    __builtin_amdgcn_sched_barrier(0);
}

// The block-uniform doubles of a replica's record, held in scalar registers (the compiler leaves the results of
// v_cvt / v_mul in vector ones: 14 per lane for the whole call).
__device__ __forceinline__ MalaCoef mala_coef(const Phi4EnsRec &rc) {
    MalaCoef M;
    M.h = readlane_d((double)rc.h, 0);
    M.h4 = readlane_d(4.0 * M.h, 0);
    M.m2 = readlane_d((double)rc.m2, 0);
    M.lam6 = readlane_d((double)rc.lam6, 0);
    M.km = readlane_d(3.0 + 0.5 * M.m2, 0);
    M.l4 = readlane_d(0.25 * M.lam6, 0);
    return M;
}

}  // namespace

}  // namespace sq
