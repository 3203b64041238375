// sq_noise_consts.h -- the words of a field-noise Philox4x32-10 evaluation that
// depend only on (key, step).  Plain C++ (no HIP needed): the host computes
// them once per launch (Phi4StepArgs::nw0 / nw1), the kernels that advance the
// step themselves once per pair, and tests/noise_consts_check.c restates them.
//
// The counter of a site's quad is {quad, stream, step_lo, step_hi} with the
// field stream's word 1 equal to 0, so in the first three rounds every
// combination of words 1..3 and the key is the same for all sites:
//   round 0:  u0 = hi(M1 step_lo) ^ k0,  u1 = lo(M1 step_lo),  a0 = step_hi ^ k1
//             per site: p0 = M0 quad, n2 = hi(p0) ^ a0, n3 = lo(p0)
//   round 1:  b0 = u1 ^ (k0 + W0),  b2 = hi(M0 u0) ^ (k1 + W1),  u3 = lo(M0 u0)
//             per site: p1 = M1 n2, state {hi(p1) ^ b0, lo(p1), b2 ^ n3, u3}
//   round 2:  d2 = u3 ^ (k1 + 2 W1)
//             per site: word 2 of the new state is hi(M0 x) ^ d2
// A site's work before round 1's xors -- hi(p1), lo(p1), n3 -- depends on the
// step only through a0, i.e. through step_hi: steps s and s+1 share it unless
// s_lo = 0xFFFFFFFF.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SQ_HD __host__ __device__
#else
#define SQ_HD
#endif

namespace sq {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u;
constexpr uint32_t kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u;
constexpr uint32_t kPhiloxW1 = 0xBB67AE85u;
// M1's inverse modulo 2^32 (M1 is odd): Newton's x <- x (2 - M1 x) doubles the correct low bits, from 3
constexpr uint32_t inv_u32(uint32_t a) {
    uint32_t x = a;
    for (int i = 0; i < 5; ++i) x *= 2u - a * x;
    return x;
}
constexpr uint32_t kPhiloxM1Inv = inv_u32(kPhiloxM1);
static_assert(kPhiloxM1 * kPhiloxM1Inv == 1u, "M1 inverse");

// Noise streams (bits 24..31 of counter word 1).
constexpr uint32_t kStreamField = 0;  // per-site field noise
constexpr uint32_t kStreamOmega = 1;  // QM1D collective coordinate
constexpr uint32_t kStreamInit = 2;   // initial field
constexpr uint32_t kStreamAccept = 3; // the MALA step's accept/reject uniform (quad 0, one draw per replica and step)

struct Phi4NoiseConsts {
    uint32_t u0, u1, a0, b0, b2, u3, d2;
};

SQ_HD inline Phi4NoiseConsts phi4_noise_consts(uint32_t k0, uint32_t k1, uint64_t step) {
    const uint32_t cy = kStreamField << 24, cz = (uint32_t)step, cw = (uint32_t)(step >> 32);
    Phi4NoiseConsts w;
    const uint64_t p1u = (uint64_t)kPhiloxM1 * cz;
    w.u0 = (uint32_t)(p1u >> 32) ^ cy ^ k0;
    w.u1 = (uint32_t)p1u;
    w.a0 = cw ^ k1;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
    const uint64_t p0u = (uint64_t)kPhiloxM0 * w.u0;
    w.b0 = w.u1 ^ k0;
    w.b2 = (uint32_t)(p0u >> 32) ^ k1;
    w.u3 = (uint32_t)p0u;
    k1 += kPhiloxW1;
    w.d2 = w.u3 ^ k1;
    return w;
}

}  // namespace sq
