// sq_phi4_ens.hip -- R small phi^4 lattices per launch, each on-chip in one
// work-group for every step of the call.
//
// The step kernels of sq_phi4.hip stream one large lattice through HBM, one
// launch per step (or pair); a lattice of <= 32,768 sites fills a few CUs and
// pays a launch per step.  Here work-group r owns replica r: it loads its
// lattice once, keeps it in registers (each lane a fixed set of K float4
// quads, quad q = lane + j T of the lattice's linear order, j < K) and in one
// LDS image that serves the neighbour reads, runs all the call's steps, and
// stores the lattice once.  Nothing else touches HBM during the call; the
// measurement records (4 doubles per replica per `every` steps) go to a
// pinned host buffer.
//
// Per step and quad: four ds_read_b128 (y-1, y+1, z-1, z+1 quads) and two
// ds_read_b32 (x-1 of the quad's first site, x+1 of its last) from the image,
// the quad's Philox normals, site_update4, and the result back to the image.
// With two images (they fit up to 20,000-odd sites) a step reads one and
// writes the other, one barrier per step; with one image every wave must have
// finished reading before any writes: two barriers per step.  The periodic
// wraps are selects on per-quad flag bits (y == 0, y == Ly-1, ...) computed
// once; the neighbour offsets are recomputed from them every step (kept out
// of registers on purpose: 6 K offsets per lane would not fit beside the field).
//
// Replica r is bit for bit the single context of the same seed: the site
// arithmetic is site_update4 itself (fin = false: the full guard, identical
// results to the fast path), the counter is {linear quad, kStreamField << 24,
// step_lo, step_hi} through tb_noise, keyed by the replica's seed.  A replica
// whose sig is 0 takes the noise-off instance of the update, as a context with
// C = 0 does.  No work-group ever waits for another one.
#define SQ_PHI4_KERNELS_ONLY
#include "sq_phi4.hip"
#include "sq_phi4_ens.h"

namespace sq {

namespace {

extern __shared__ __attribute__((aligned(16))) char ens_smem[];

// Per-quad flag bits (block-invariant, one VGPR per owned quad).
constexpr uint32_t kEnsY0 = 1, kEnsY1 = 2, kEnsZ0 = 4, kEnsZ1 = 8, kEnsX0 = 16, kEnsX1 = 32, kEnsValid = 64;

struct EnsGeo {  // block-uniform
    int Lx, Q;              // row length in sites, quads of the lattice
    int qrow, qplane;       // quads per row, per plane
    int qywrap, qzwrap;     // (Ly - 1) qrow, (Lz - 1) qplane
};

__device__ __forceinline__ EnsGeo ens_geo(const Phi4EnsArgs &E) {
    EnsGeo g;
    g.Lx = E.Lx;
    g.qrow = E.Lx >> 2;
    g.qplane = g.qrow * E.Ly;
    g.Q = g.qplane * E.Lz;
    g.qywrap = (E.Ly - 1) * g.qrow;
    g.qzwrap = (E.Lz - 1) * g.qplane;
    return g;
}

__device__ __forceinline__ uint32_t ens_flags(const Phi4EnsArgs &E, const EnsGeo &g, int q) {
    if (q >= g.Q) return 0;
    const int x4 = q & (g.qrow - 1);  // Lx is a power of two
    const int yz = q / g.qrow;
    const int y = yz % E.Ly, z = yz / E.Ly;
    return kEnsValid | (y == 0 ? kEnsY0 : 0) | (y == E.Ly - 1 ? kEnsY1 : 0) | (z == 0 ? kEnsZ0 : 0) |
           (z == E.Lz - 1 ? kEnsZ1 : 0) | (x4 == 0 ? kEnsX0 : 0) | (x4 == g.qrow - 1 ? kEnsX1 : 0);
}

// Neighbour offsets of quad q: the four quads in float4 units, the two x-sites in floats.
struct EnsNbr {
    int up, dn, zm, zp, lf, rg;
};
__device__ __forceinline__ EnsNbr ens_nbr(const EnsGeo &g, int q, uint32_t f) {
    EnsNbr n;
    n.up = q + ((f & kEnsY0) ? g.qywrap : -g.qrow);
    n.dn = q + ((f & kEnsY1) ? -g.qywrap : g.qrow);
    n.zm = q + ((f & kEnsZ0) ? g.qzwrap : -g.qplane);
    n.zp = q + ((f & kEnsZ1) ? -g.qzwrap : g.qplane);
    n.lf = 4 * q + ((f & kEnsX0) ? g.Lx - 1 : -1);
    n.rg = 4 * q + ((f & kEnsX1) ? 4 - g.Lx : 4);
    return n;
}

// One step of the lane's K quads: c <- update(c, neighbours in img).
template <int K, bool NZ>
__device__ __forceinline__ void ens_step(const Phi4StepArgs &A, const EnsGeo &g, float4 (&c)[K],
                                         const uint32_t (&fl)[K], const float *img, uint32_t slo, uint32_t shi,
                                         float &am) {
    const float4 *img4 = reinterpret_cast<const float4 *>(img);
    const int T = blockDim.x;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        uint32_t f = fl[j];
        int q = (int)threadIdx.x + j * T;
        // opaque per step: the offsets below are recomputed, not kept (hoisted, both arms of
        // every wrap select stay live: 12 registers per quad)
        asm volatile("" : "+v"(f), "+v"(q));
        if (f & kEnsValid) {
            const EnsNbr n = ens_nbr(g, q, f);
            const float4 up = img4[n.up], dn = img4[n.dn], zm = img4[n.zm], zp = img4[n.zp];
            const float lft = img[n.lf], rgt = img[n.rg];
            const f32x4n xi = tb_noise<NZ>(A, 0u, (uint32_t)q, slo, shi);
            float mp;
            c[j] = site_update4<NZ>(c[j], lft, rgt, up, dn, zm, zp, xi, A, false, f32x2{A.m2, A.m2}, &mp);
            am = fmaxf(am, mp);  // mp: max |phi'| after the full guard, never NaN
        }
    }
}

// The lane's share of S1 = sum phi, S2 = sum phi^2, S4 = sum phi^4, NN = sum
// over sites and the three forward links of phi(x) phi(x + mu), in double
// (every product of two floats is exact there; phi^4 = (phi^2)^2 rounds
// once), and of max |phi|.  img holds the same field as c.
template <int K>
__device__ __forceinline__ void ens_sums(const EnsGeo &g, const float4 (&c)[K], const uint32_t (&fl)[K],
                                         const float *img, double (&s)[4], float &mx) {
    const float4 *img4 = reinterpret_cast<const float4 *>(img);
    const int T = blockDim.x;
    s[0] = s[1] = s[2] = s[3] = 0.0;
    mx = 0.f;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        uint32_t f = fl[j];
        int q = (int)threadIdx.x + j * T;
        asm volatile("" : "+v"(f), "+v"(q));  // as ens_step
        if (f & kEnsValid) {
            const EnsNbr n = ens_nbr(g, q, f);
            const float4 dn = img4[n.dn], zp = img4[n.zp];
            const double x = c[j].x, y = c[j].y, z = c[j].z, w = c[j].w, r = img[n.rg];
            const double x2 = x * x, y2 = y * y, z2 = z * z, w2 = w * w;
            s[0] += (x + y) + (z + w);
            s[1] += (x2 + y2) + (z2 + w2);
            s[2] += (x2 * x2 + y2 * y2) + (z2 * z2 + w2 * w2);
            s[3] += ((x * y + y * z) + (z * w + w * r)) +
                    ((x * (double)dn.x + y * (double)dn.y) + (z * (double)dn.z + w * (double)dn.w)) +
                    ((x * (double)zp.x + y * (double)zp.y) + (z * (double)zp.z + w * (double)zp.w));
            mx = fmaxf(mx, fmaxf(fmaxf(fabsf(c[j].x), fabsf(c[j].y)), fmaxf(fabsf(c[j].z), fabsf(c[j].w))));
        }
    }
}

// Wave total by the DPP inclusive-scan sequence (row_shr 1/2/4/8, row_bcast
// 15/31; a lane without a source adds 0), read from lane 63: no LDS round
// trips, a fixed order.
__device__ __forceinline__ double ens_wave_sum(double v) {
    v += dpp_d<0x111, 0xf, 0xf>(v, 0.0);
    v += dpp_d<0x112, 0xf, 0xf>(v, 0.0);
    v += dpp_d<0x114, 0xf, 0xf>(v, 0.0);
    v += dpp_d<0x118, 0xf, 0xf>(v, 0.0);
    v += dpp_d<0x142, 0xa, 0xf>(v, 0.0);
    v += dpp_d<0x143, 0xc, 0xf>(v, 0.0);
    return readlane_d(v, 63);
}

// Wave totals into the scratch behind the images, one barrier, then lane i < 4
// of wave 0 folds sum i over the waves in wave order into out[i] (and lane 4
// the maximum into out[4] when mxout): the same bits on every call.  The
// scratch is free again after the next block barrier, which every later
// writer sits behind.
__device__ __forceinline__ void ens_fold(double (&s)[4], float mx, double *scr, double *out, bool mxout) {
    float *scm = reinterpret_cast<float *>(scr + 16 * 4);
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = ens_wave_sum(s[i]);
    mx = dpp_all_max_f(mx);  // never NaN: fmaxf of magnitudes drops them
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) scr[4 * w + i] = s[i];
        scm[w] = mx;
    }
    __syncthreads();
    const int i = threadIdx.x;
    if (i < 4) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 16; ++k) t += k < nw ? scr[4 * k + i] : 0.0;
        out[i] = t;
    } else if (i == 4 && mxout) {
        float m = 0.f;
#pragma unroll
        for (int k = 0; k < 16; ++k) m = fmaxf(m, k < nw ? scm[k] : 0.f);
        out[4] = (double)m;
    }
}

template <int K>
__device__ __forceinline__ void ens_load(const Phi4EnsArgs &E, const EnsGeo &g, int r, float4 (&c)[K],
                                         uint32_t (&fl)[K], float *img) {
    const float4 *gf = reinterpret_cast<const float4 *>(E.field + (size_t)r * (size_t)(4 * g.Q));
    float4 *img4 = reinterpret_cast<float4 *>(img);
    const int T = blockDim.x;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        const int q = (int)threadIdx.x + j * T;
        fl[j] = ens_flags(E, g, q);
        c[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (fl[j] & kEnsValid) {
            c[j] = gf[q];
            img4[q] = c[j];
        }
    }
    __syncthreads();
}

// two != 0: two LDS images (the launcher sized the dynamic LDS for them).
template <int K>
__global__ __launch_bounds__(kPhi4EnsMaxLanes) void phi4_ens_step_kernel(const Phi4EnsArgs E, const int two) {
    const int r = blockIdx.x;
    const EnsGeo g = ens_geo(E);
    const Phi4EnsRec rc = E.rec[r];
    Phi4StepArgs A{};
    A.h = rc.h;
    A.m2 = rc.m2;
    A.lam6 = rc.lam6;
    A.sig = rc.sig;
    A.sigq = rc.sigq;
    A.clampv = E.clampv;
    A.k0 = rc.k0;
    A.k1 = rc.k1;
    const bool nz = rc.sig != 0.0f;  // phi4_step_launch's choice of instance
    float *img0 = reinterpret_cast<float *>(ens_smem);
    float *img1 = two ? img0 + 4 * g.Q : img0;
    double *scr = reinterpret_cast<double *>(ens_smem + (size_t)(two ? 2 : 1) * 16 * (size_t)g.Q);
    float4 c[K];
    uint32_t fl[K];
    ens_load<K>(E, g, r, c, fl, img0);
    const int T = blockDim.x;
    float am = 0.f;
    const unsigned long long s0 = rc.step + E.adv;
    float *cur = img0, *oth = img1;
    int left = E.every;  // steps until the next measurement
    int rec = 0;
    for (int t = 0; t < E.nsteps; ++t) {
        const unsigned long long s = s0 + (unsigned long long)t;
        const uint32_t slo = (uint32_t)s, shi = (uint32_t)(s >> 32);
        if (nz) ens_step<K, true>(A, g, c, fl, cur, slo, shi, am);
        else ens_step<K, false>(A, g, c, fl, cur, slo, shi, am);
        if (!two) __syncthreads();  // one image: every wave has read it
        {
            float *x = cur;
            cur = oth;
            oth = x;
        }
        float4 *cur4 = reinterpret_cast<float4 *>(cur);
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (fl[j] & kEnsValid) cur4[(int)threadIdx.x + j * T] = c[j];
        __syncthreads();
        if (E.series != nullptr && --left == 0) {
            left = E.every;
            double sm[4];
            float mx;
            ens_sums<K>(g, c, fl, cur, sm, mx);
            ens_fold(sm, mx, scr, E.series + 4 * ((size_t)rec * gridDim.x + (size_t)r), false);
            ++rec;
        }
    }
    float4 *gf = reinterpret_cast<float4 *>(E.field + (size_t)r * (size_t)(4 * g.Q));
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (fl[j] & kEnsValid) gf[(int)threadIdx.x + j * T] = c[j];
    // some site was clamped (NaN -> +clamp) iff the running max after the guard reached the clamp
    if (am >= E.clampv) E.flags[r] = 1;
}

template <int K>
__global__ __launch_bounds__(kPhi4EnsMaxLanes) void phi4_ens_moments_kernel(const Phi4EnsArgs E, const int first,
                                                                             double *out) {
    const int r = first + blockIdx.x;
    const EnsGeo g = ens_geo(E);
    float *img = reinterpret_cast<float *>(ens_smem);
    double *scr = reinterpret_cast<double *>(ens_smem + 16 * (size_t)g.Q);
    float4 c[K];
    uint32_t fl[K];
    ens_load<K>(E, g, r, c, fl, img);
    double sm[4];
    float mx;
    ens_sums<K>(g, c, fl, img, sm, mx);
    ens_fold(sm, mx, scr, out + 5 * (size_t)blockIdx.x, true);
}

// phi4_init_kernel's field for every replica (blockIdx.y) from its own key.
__global__ __launch_bounds__(256) void phi4_ens_init_kernel(const Phi4EnsArgs E, const float amp) {
    const int r = blockIdx.y;
    const size_t nq = (size_t)(E.Lx >> 2) * (size_t)E.Ly * (size_t)E.Lz;
    const uint32_t k0 = E.rec[r].k0, k1 = E.rec[r].k1;
    float4 *gf = reinterpret_cast<float4 *>(E.field + (size_t)r * 4 * nq);
    for (size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += (size_t)gridDim.x * blockDim.x) {
        const f32x4n n = normals4(q, kStreamInit, 0u, 0u, k0, k1);
        gf[q] = make_float4(amp * n.a, amp * n.b, amp * n.c, amp * n.d);
    }
}

hipError_t ens_lds_attr(const void *fn, int bytes) {
    // above the default dynamic-LDS ceiling the function needs the attribute (once per instance and device;
    // setting it again is harmless)
    if (bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

bool ens_shape_ok(const Phi4EnsArgs &a) {
    const long long S = (long long)a.Lx * a.Ly * a.Lz;
    return (a.Lx == 8 || a.Lx == 16 || a.Lx == 32 || a.Lx == 64) && a.Ly >= 2 && a.Lz >= 2 &&
           S <= kPhi4EnsMaxSites && a.field != nullptr && a.rec != nullptr;
}

}  // namespace

Phi4EnsShape phi4_ens_shape(int sites) {
    Phi4EnsShape s;
    const int Q = sites / 4;
    s.K = Q <= kPhi4EnsMaxLanes ? 1 : (Q <= 2 * kPhi4EnsMaxLanes ? 2 : (Q <= 4 * kPhi4EnsMaxLanes ? 4 : 8));
    s.T = (((Q + s.K - 1) / s.K) + 63) / 64 * 64;
    s.two = 2 * 4 * sites + kPhi4EnsScratchBytes <= kPhi4EnsLdsBytes;
    s.lds_bytes = (s.two ? 2 : 1) * 4 * sites + kPhi4EnsScratchBytes;
    return s;
}

hipError_t phi4_ens_step_launch(const Phi4EnsArgs &a, int nrep, hipStream_t s) {
    if (!ens_shape_ok(a) || a.flags == nullptr || nrep < 1 || a.nsteps < 0 || a.every < 0 ||
        (a.series != nullptr && a.every < 1))
        return hipErrorInvalidValue;
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz);
    Phi4EnsArgs q = a;
    int two = sh.two ? 1 : 0;
    void *args[] = {&q, &two};
    const void *fn = sh.K == 1   ? (const void *)&phi4_ens_step_kernel<1>
                     : sh.K == 2 ? (const void *)&phi4_ens_step_kernel<2>
                     : sh.K == 4 ? (const void *)&phi4_ens_step_kernel<4>
                                 : (const void *)&phi4_ens_step_kernel<8>;
    hipError_t e = ens_lds_attr(fn, sh.lds_bytes);
    if (e != hipSuccess) return e;
    return hipLaunchKernel(fn, dim3((unsigned)nrep), dim3((unsigned)sh.T), args, (size_t)sh.lds_bytes, s);
}

hipError_t phi4_ens_moments_launch(const Phi4EnsArgs &a, int first, int count, double *out, hipStream_t s) {
    if (!ens_shape_ok(a) || first < 0 || count < 1 || out == nullptr) return hipErrorInvalidValue;
    const int sites = a.Lx * a.Ly * a.Lz;
    const Phi4EnsShape sh = phi4_ens_shape(sites);
    const int bytes = 4 * sites + kPhi4EnsScratchBytes;
    Phi4EnsArgs q = a;
    void *args[] = {&q, &first, &out};
    const void *fn = sh.K == 1   ? (const void *)&phi4_ens_moments_kernel<1>
                     : sh.K == 2 ? (const void *)&phi4_ens_moments_kernel<2>
                     : sh.K == 4 ? (const void *)&phi4_ens_moments_kernel<4>
                                 : (const void *)&phi4_ens_moments_kernel<8>;
    hipError_t e = ens_lds_attr(fn, bytes);
    if (e != hipSuccess) return e;
    return hipLaunchKernel(fn, dim3((unsigned)count), dim3((unsigned)sh.T), args, (size_t)bytes, s);
}

hipError_t phi4_ens_init_launch(const Phi4EnsArgs &a, int nrep, float amp, hipStream_t s) {
    if (!ens_shape_ok(a) || nrep < 1) return hipErrorInvalidValue;
    const int nq = a.Lx * a.Ly * a.Lz / 4;
    Phi4EnsArgs q = a;
    void *args[] = {&q, &amp};
    // grid.y <= 65535: larger ensembles go in slices of replicas
    for (int r0 = 0; r0 < nrep; r0 += 32768) {
        const int n = nrep - r0 < 32768 ? nrep - r0 : 32768;
        q.field = a.field + (size_t)r0 * (size_t)(4 * nq);
        q.rec = a.rec + r0;
        hipError_t e = hipLaunchKernel((const void *)&phi4_ens_init_kernel, dim3((unsigned)((nq + 255) / 256), (unsigned)n),
                                       dim3(256), args, 0, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace sq
