// sq_qm1d_math.h -- the QM1D chain's per-site expressions shared by the frame
// kernels (sq_qm1d.hip: one chain per launch; sq_qm1d_ens.hip: one chain per
// work-group): the potential's x_cl / ddPot, the shared-divisor fp64 division
// and small register helpers.  Device code; expressions keep the reference's
// order and the including files are built with -ffp-contract=off.
#pragma once
#include <hip/hip_runtime.h>

#include "sq_glibcf.h"

namespace sq {
namespace {

constexpr double kEta = .8;  // tau_kernel.cl:19-22
constexpr double kV0 = 2.;
constexpr double kM = 1.;

__device__ __forceinline__ double xcl(double t, double w, int pot) {  // clas(), :184-189,215-226
    if (pot == 3) {
        const double s = 2.0;  // (double)sqrtf((float)(2.*V0/m)) == 2 exactly
        return kEta * (double)sq_glibc_tanhf((float)(s * (t - w) / kEta));  // glibc's tanhf, bit for bit
    }
    return 0.;
}
__device__ __forceinline__ double ddpot(double x, int pot) {  // ddPot(), :190-195,227-236
    if (pot == 3) return (12. * kV0 * x * x / (kEta * kEta) - 4. * kV0) / (kEta * kEta);
    return 2.;
}
__device__ __forceinline__ double absol(double v) { return v <= 0 ? -v : v; }
// potID 3: the float tanhf inside clas() (x_cl = kEta * (double) of it)
__device__ __forceinline__ float xcl_tanh(double t, double w) {
    const double s = 2.0;  // (double)sqrtf((float)(2.*V0/m)) == 2 exactly
    return sq_glibc_tanhf((float)(s * (t - w) / kEta));
}

// a / b for a divisor b shared by many quotients (a2 for the frame, the step's
// den), bit-identical to the compiler's fp64 division.  That expansion is
//   r = rcp(b'); two Newton steps R = fma(r1, fma(-b', r1, 1), r1) with
//   r1 = fma(r, fma(-b', r, 1), r); m = a' R; q = fixup(fmas(fma(-b', m, a'), R, m))
// where b', a' are v_div_scale's operands: b and a themselves, with vcc clear,
// unless an exponent is extreme.  With b in [2^-60, 2^60] (UDiv::ok) and
// 2^-960 < |a| < 2^700 nothing is scaled, div_fmas is a plain fma and
// div_fixup returns its (finite, normal) input, so R is computed once per
// divisor and a quotient is a multiply and two fmas instead of 10 instructions
// with a quarter-rate v_rcp_f64.  Any other a (0, -0, inf, NaN, tiny or huge)
// takes the full division (udiv_step).
struct UDiv {
    double b, r;
    bool ok;  // b in [2^-60, 2^60]: otherwise every quotient takes the full division
};
__device__ __forceinline__ UDiv udiv_prep(double b) {
    const double r0 = __builtin_amdgcn_rcp(b);
    const double r1 = __builtin_fma(r0, __builtin_fma(-b, r0, 1.0), r0);
    return UDiv{b, __builtin_fma(r1, __builtin_fma(-b, r1, 1.0), r1), b >= 0x1p-60 && b <= 0x1p+60};
}
__device__ __forceinline__ bool udiv_range(double a) {  // false for 0, NaN, inf, tiny, huge
    const double x = __builtin_fabs(a);
    return x > 0x1p-960 && x < 0x1p+700;
}
__device__ __forceinline__ double udiv_fast(double a, const UDiv &d) {
    const double m = a * d.r;
    return __builtin_fma(__builtin_fma(-d.b, m, a), d.r, m);
}
// The quotients of one step: the fast form unless some lane of the wave has a
// numerator outside its range (one wave-uniform branch per step, not one per
// quotient: per-quotient branches cost more than the division they skip).
template <int M, bool FAST>
__device__ __forceinline__ void udiv_step(const double (&n)[M], const UDiv &d, double (&q)[M], bool bad) {
    if (!FAST || __ballot(bad || !d.ok) != 0ull) {
        asm volatile("");  // a real branch: an fdiv is one IR instruction, cheap enough to speculate
#pragma unroll
        for (int k = 0; k < M; ++k) q[k] = n[k] / d.b;
    } else {
#pragma unroll
        for (int k = 0; k < M; ++k) q[k] = udiv_fast(n[k], d);
    }
}

template <int K>
__device__ __forceinline__ double pick(const double (&v)[K], int k) {  // v[k], k wave-uniform
    double r = v[0];
#pragma unroll
    for (int q = 1; q < K; ++q)
        if (q == k) r = v[q];
    return r;
}

}  // namespace
}  // namespace sq
