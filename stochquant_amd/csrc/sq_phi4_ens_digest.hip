// sq_phi4_ens_digest.hip -- the phi^4 ensemble's field digest (include/stochquant.h, "Checkpoints of the phi^4
// ensemble"): per replica D_r = sum over sites i of mix((i << 32) | bits32(phi_r[i])) mod 2^64, mix the
// splitmix64 finaliser.  The sum is a wrapping integer sum, exact in any lane order.  One work-group per replica
// of the range; it reads the replica's row and writes eight bytes, nothing else: no atomics, no global scratch,
// and no phi4_ens_shape, since the kernel keeps nothing on chip.
#include "sq_phi4_ens.h"

namespace sq {

namespace {

// a * b mod 2^64 from 32-bit multiplies: the low product whole, the two cross products' low halves.
__device__ inline uint64_t mul64(uint64_t a, uint64_t b) {
    const uint32_t al = (uint32_t)a, ah = (uint32_t)(a >> 32), bl = (uint32_t)b, bh = (uint32_t)(b >> 32);
    const uint32_t lo = al * bl;
    const uint32_t hi = __umulhi(al, bl) + al * bh + ah * bl;
    return ((uint64_t)hi << 32) | lo;
}

__device__ inline uint64_t digest_mix(uint64_t x) {
    x ^= x >> 30;
    x = mul64(x, 0xBF58476D1CE4E5B9ull);
    x ^= x >> 27;
    x = mul64(x, 0x94D049BB133111EBull);
    x ^= x >> 31;
    return x;
}

__device__ inline uint64_t digest_site(uint32_t i, uint32_t bits) { return digest_mix(((uint64_t)i << 32) | bits); }

__global__ __launch_bounds__(kPhi4EnsMaxLanes) void phi4_ens_digest_kernel(const float *field, const int sites,
                                                                            const int first,
                                                                            unsigned long long *out) {
    const uint32_t *row = reinterpret_cast<const uint32_t *>(field) + (size_t)(first + (int)blockIdx.x) * (size_t)sites;
    const int T = (int)blockDim.x, t = (int)threadIdx.x;
    // 16-byte loads while whole quads remain: every row starts on a 16-byte boundary when sites is a multiple of
    // 4 (an ensemble's always is: Lx is a multiple of 8); the rest, and any other row length, site by site
    const int nq = (sites & 3) ? 0 : sites >> 2;
    const uint4 *quads = reinterpret_cast<const uint4 *>(row);
    uint64_t acc = 0;
#pragma unroll 4
    for (int q = t; q < nq; q += T) {
        const uint4 v = quads[q];
        const uint32_t i = 4u * (uint32_t)q;
        acc += digest_site(i, v.x) + digest_site(i + 1, v.y) + digest_site(i + 2, v.z) + digest_site(i + 3, v.w);
    }
    for (int i = 4 * nq + t; i < sites; i += T) acc += digest_site((uint32_t)i, row[i]);
    // the wave's sum, then the waves' through LDS
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_down((int)(uint32_t)acc, o, 64);
        const uint32_t hi = (uint32_t)__shfl_down((int)(uint32_t)(acc >> 32), o, 64);
        acc += ((uint64_t)hi << 32) | lo;
    }
    __shared__ uint64_t part[kPhi4EnsMaxLanes / 64];
    if ((t & 63) == 0) part[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        uint64_t d = 0;
        for (int w = 0; w < (T >> 6); ++w) d += part[w];
        out[blockIdx.x] = d;
    }
}

}  // namespace

hipError_t phi4_ens_digest_launch(const float *field, int sites, int first, int count, unsigned long long *out,
                                  hipStream_t s) {
    if (!field || !out || sites < 1 || first < 0 || count < 1) return hipErrorInvalidValue;
    // one lane per quad up to the work-group limit, whole waves
    int T = ((sites + 3) / 4 + 63) / 64 * 64;
    if (T > kPhi4EnsMaxLanes) T = kPhi4EnsMaxLanes;
    void *args[] = {(void *)&field, (void *)&sites, (void *)&first, (void *)&out};
    return hipLaunchKernel((const void *)&phi4_ens_digest_kernel, dim3((unsigned)count), dim3((unsigned)T), args, 0, s);
}

}  // namespace sq
