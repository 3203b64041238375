// sq_phi4_ens_dev.h -- the device functions every kernel of the phi^4 lattice
// ensemble shares (the sq_phi4_ens*.hip translation units).
// Device code only: the kernels and their launchers are the units' own.
//
// Work-group r owns replica r: each lane a fixed set of K float4 quads (quad
// q = lane + j T of the lattice's linear order, j < K) in registers, and one
// or two LDS images (ens_smem) that serve the neighbour reads.
//
// Per step and quad: four ds_read_b128 (y-1, y+1, z-1, z+1 quads) and two
// ds_read_b32 (x-1 of the quad's first site, x+1 of its last) from the image,
// the quad's Philox normals, site_update4, and the result back to the image.
// The periodic wraps are selects on per-quad flag bits (y == 0, y == Ly-1, ...)
// computed once; the neighbour offsets are recomputed from them every step
// (kept out of registers on purpose: 6 K offsets per lane would not fit beside
// the field).
//
// Replica r is bit for bit the single context of the same seed: the site
// arithmetic is site_update4 itself (fin = false: the full guard, identical
// results to the fast path), the counter is {linear quad, kStreamField << 24,
// step_lo, step_hi} through tb_noise, keyed by the replica's seed.
//
// The device functions of sq_phi4.hip come in by its SQ_PHI4_KERNELS_ONLY
// include, which stands here once for all the units.
#pragma once
#define SQ_PHI4_KERNELS_ONLY
#include <type_traits>

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
// writer sits behind.  tid: the lane's threadIdx.x; a caller with no register
// to spare passes an opaque copy, so that nothing formed from it here is
// hoisted out of the caller's loops and kept (ens_corr, ens_pcorr_measure alike).
__device__ __forceinline__ void ens_fold(double (&s)[4], float mx, double *scr, double *out, bool mxout,
                                         unsigned tid = threadIdx.x) {
    float *scm = reinterpret_cast<float *>(scr + 16 * 4);
    const int w = tid >> 6, nw = blockDim.x >> 6;
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = ens_wave_sum(s[i]);
    mx = dpp_all_max_f(mx);  // never NaN: fmaxf of magnitudes drops them
    if ((tid & 63) == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) scr[4 * w + i] = s[i];
        scm[w] = mx;
    }
    __syncthreads();
    const int i = tid;
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

// One time-slice correlator measurement of the field in img.
// Slice sums: wave w takes slices w, w + nw, ...; its lanes stride the slice's
// quads in ascending order, each quad (x + y) + (z + w) in double, the wave by
// ens_wave_sum, S(z) to Sl[z]: the bits depend on the slice's shape and sites
// only.  One barrier, then lane t (and t + T) forms g(t) = sum_z S(z) S((z + t)
// mod Lz), z ascending, every product and sum rounded once, and lane T - 1
// s1 = sum_z S(z).  ACC: G[t] = G[t] + g(t), S1 += s1, nmeas += 1 in place (the
// same lane owns an entry for the whole call); else G[t] = g(t) and, Sout
// given, the slice sums to it.  Every lane of the block calls it; Sl is free
// again after the next block barrier.
template <bool ACC>
__device__ __forceinline__ void ens_corr(const EnsGeo &g, int Lz, const float *img, double *Sl, double *G, double *S1,
                                         long long *nm, double *Sout, unsigned tid = threadIdx.x) {
#pragma clang fp contract(off)
    const float4 *img4 = reinterpret_cast<const float4 *>(img);
    const int T = blockDim.x, lane = tid & 63, nw = T >> 6;
    const int w = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
    for (int z = w; z < Lz; z += nw) {  // wave-uniform: every lane reaches the scan
        const float4 *sl = img4 + z * g.qplane;
        double a = 0.0;
        for (int i = lane; i < g.qplane; i += 64) {
            const float4 v = sl[i];
            a += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
        }
        a = ens_wave_sum(a);
        if (lane == 63) Sl[z] = a;
    }
    __syncthreads();
    const int nt = Lz / 2 + 1;
    for (int t = tid; t < nt; t += T) {
        double old = 0.0;
        if (ACC) old = G[t];
        double acc = 0.0;
        int zt = t;
        for (int z = 0; z < Lz; ++z) {
            acc = __dadd_rn(acc, __dmul_rn(Sl[z], Sl[zt]));
            zt = zt + 1 == Lz ? 0 : zt + 1;
        }
        G[t] = ACC ? __dadd_rn(old, acc) : acc;
    }
    if (ACC) {
        if ((int)tid == T - 1) {
            double s = 0.0;
            for (int z = 0; z < Lz; ++z) s = __dadd_rn(s, Sl[z]);
            *S1 = __dadd_rn(*S1, s);
            *nm += 1;
        }
    } else if (Sout != nullptr) {
        for (int z = tid; z < Lz; z += T) Sout[z] = Sl[z];
    }
}

// One momentum measurement of the field in img, momentum by
// momentum through the 2 Lz doubles at Pl (A at Pl[z], B at Pl[Lz + z]; the
// zero-momentum Sl of an ens_corr call just before lies in the same region).
// Projections: as ens_corr's slice sums, wave w slices w, w + nw, ..., the
// lanes striding the slice's quads; 64 is a multiple of the row's quads, so
// every quad of a lane has the same x0 = 4 (lane mod qrow) and its eight
// x-twiddles are loaded once per momentum; the row y = i / qrow changes per
// quad.  Per quad re = (p0 cx0 + p1 cx1) + (p2 cx2 + p3 cx3), im the same with
// sx, a += re cy - im sy, b += re sy + im cy, every product and sum rounded
// once; the wave by ens_wave_sum.  Then, behind a barrier, lane t (and t + T)
// forms g_m(t) = sum_z [A(z) A(zt) + B(z) B(zt)] as (acc + A A) + B B, z
// ascending.  ACC: Gp[m][t] = Gp[m][t] + g_m(t) and nmeas_p += 1 in place (the
// same lane owns an entry for the whole call); else Gp[m][t] = g_m(t) and, ABout
// given, the projections to ABout[m][z][2].  A barrier stands between a
// region's last reader and its next writer: at the top of every momentum (the
// reader before the first one is ens_corr's or the previous measurement's).
// Every lane of the block calls it; Pl is free again after the next block barrier.
template <bool ACC>
__device__ __forceinline__ void ens_pcorr(const EnsGeo &g, int Ly, int Lz, const float *img, double *Pl,
                                          const Phi4EnsPCorrArgs &P, double *Gp, long long *nm, double *ABout) {
#pragma clang fp contract(off)
    const float4 *img4 = reinterpret_cast<const float4 *>(img);
    // opaque per measurement: nothing that depends on the lane is hoisted out of the caller's loops and kept
    // in registers across its steps (the K = 8 frames instance has none to spare)
    int tid = (int)threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int T = blockDim.x, lane = tid & 63, nw = T >> 6;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nt = Lz / 2 + 1;
    const int qsh = 31 - __builtin_clz((unsigned)g.qrow);  // qrow is a power of two
    const int x0 = 4 * (lane & (g.qrow - 1));
    double *Al = Pl, *Bl = Pl + Lz;
    for (int m = 0; m < P.M; ++m) {
        const double *cx = P.cx + m * g.Lx + x0, *sx = P.sx + m * g.Lx + x0;
        const double *cy = P.cy + m * Ly, *sy = P.sy + m * Ly;
        const double c0 = cx[0], c1 = cx[1], c2 = cx[2], c3 = cx[3];
        const double s0 = sx[0], s1 = sx[1], s2 = sx[2], s3 = sx[3];
        __syncthreads();
        for (int z = w; z < Lz; z += nw) {  // wave-uniform: every lane reaches the scans
            const float4 *sl = img4 + z * g.qplane;
            double a = 0.0, b = 0.0;
            for (int i = lane; i < g.qplane; i += 64) {
                const float4 v = sl[i];
                const int y = i >> qsh;
                const double p0 = v.x, p1 = v.y, p2 = v.z, p3 = v.w, yc = cy[y], ys = sy[y];
                const double re = __dadd_rn(__dadd_rn(__dmul_rn(p0, c0), __dmul_rn(p1, c1)),
                                            __dadd_rn(__dmul_rn(p2, c2), __dmul_rn(p3, c3)));
                const double im = __dadd_rn(__dadd_rn(__dmul_rn(p0, s0), __dmul_rn(p1, s1)),
                                            __dadd_rn(__dmul_rn(p2, s2), __dmul_rn(p3, s3)));
                a = __dadd_rn(a, __dsub_rn(__dmul_rn(re, yc), __dmul_rn(im, ys)));
                b = __dadd_rn(b, __dadd_rn(__dmul_rn(re, ys), __dmul_rn(im, yc)));
            }
            a = ens_wave_sum(a);
            b = ens_wave_sum(b);
            if (lane == 63) {
                Al[z] = a;
                Bl[z] = b;
            }
        }
        __syncthreads();
        double *G = Gp + m * nt;
        for (int t = tid; t < nt; t += T) {
            double old = 0.0;
            if (ACC) old = G[t];
            double acc = 0.0;
            int zt = t;
            for (int z = 0; z < Lz; ++z) {
                acc = __dadd_rn(__dadd_rn(acc, __dmul_rn(Al[z], Al[zt])), __dmul_rn(Bl[z], Bl[zt]));
                zt = zt + 1 == Lz ? 0 : zt + 1;
            }
            G[t] = ACC ? __dadd_rn(old, acc) : acc;
        }
        if (!ACC && ABout != nullptr) {
            double *o = ABout + (size_t)m * (size_t)(2 * Lz);
            for (int z = tid; z < Lz; z += T) {
                o[2 * z] = Al[z];
                o[2 * z + 1] = Bl[z];
            }
        }
    }
    if (ACC && tid == T - 1) *nm += 1;
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

// A kernel's step coefficients from its replica's record (the frames kernels
// rewrite h, sig and sigq after every frame's verdict).
__device__ __forceinline__ Phi4StepArgs ens_step_args(const Phi4EnsRec &rc, float clampv) {
    Phi4StepArgs A{};
    A.h = rc.h;
    A.m2 = rc.m2;
    A.lam6 = rc.lam6;
    A.sig = rc.sig;
    A.sigq = rc.sigq;
    A.clampv = clampv;
    A.k0 = rc.k0;
    A.k1 = rc.k1;
    return A;
}

// The correlator instances of the step and frames kernels are the same kernel
// templates with one trailing Phi4EnsCorrArgs argument (CA = {Phi4EnsCorrArgs});
// the plain instances (CA empty) keep their argument list and, every
// correlator statement being behind `if constexpr`, their code.
template <typename... CA>
__device__ __forceinline__ Phi4EnsCorrArgs ens_corr_args(const CA &...c) {
    static_assert(sizeof...(CA) <= 1, "at most one Phi4EnsCorrArgs");
    const Phi4EnsCorrArgs a[] = {c..., Phi4EnsCorrArgs{}};
    return a[0];
}

// The momentum instances are the third kind: CA = {Phi4EnsPCorrArgs}.
template <typename... CA>
constexpr bool kEnsPCorr = (std::is_same<CA, Phi4EnsPCorrArgs>::value || ...);
template <typename... CA>
__device__ __forceinline__ Phi4EnsPCorrArgs ens_pcorr_args(const CA &...c) {
    static_assert(sizeof...(CA) <= 1, "at most one Phi4EnsPCorrArgs");
    const Phi4EnsPCorrArgs a[] = {c..., Phi4EnsPCorrArgs{}};
    return a[0];
}

// The replica's momentum measurement where its zero-momentum one sits: that one
// first when P.corr is given, both through the region at Pl.
__device__ __forceinline__ void ens_pcorr_measure(const EnsGeo &g, const Phi4EnsArgs &E, int r, const float *img,
                                                  double *Pl, const Phi4EnsPCorrArgs &P,
                                                  unsigned tid = threadIdx.x) {
    const int nt = E.Lz / 2 + 1;
    if (P.corr.G != nullptr)  // block-uniform
        ens_corr<true>(g, E.Lz, img, Pl, P.corr.G + (size_t)r * (size_t)nt, P.corr.S1 + r, P.corr.nmeas + r, nullptr,
                       tid);
    ens_pcorr<true>(g, E.Ly, E.Lz, img, Pl, P, P.Gp + (size_t)r * (size_t)(P.M * nt), P.nmeas_p + r, nullptr);
}

// The guard of site_update on a value formed outside it: NaN -> +clamp, else clipped to [-clamp, clamp].
__device__ __forceinline__ float ens_guard(float v, float cl) { return fmaxf(fminf(v, cl), -cl); }

// The K flag words of a lane, four to a register (each has seven bits): the Heun kernel's K = 8 instances
// have no register to spare, and a shift and a mask per quad and loop buy six.
template <int K>
struct EnsFlagsPk {
    uint32_t w[(K + 3) / 4];
    __device__ __forceinline__ void pack(const uint32_t (&fl)[K]) {
#pragma unroll
        for (int i = 0; i < (K + 3) / 4; ++i) w[i] = 0u;
#pragma unroll
        for (int j = 0; j < K; ++j) w[j >> 2] |= fl[j] << (8 * (j & 3));
    }
    __device__ __forceinline__ uint32_t get(int j) const {
        uint32_t v = w[j >> 2];
        asm volatile("" : "+v"(v));  // opaque per use: the unpacked words are not hoisted and kept
        return (v >> (8 * (j & 3))) & 0xffu;
    }
};

// A wave's record of one Heun step.  Where FrameAcc carries the running (m, d)
// in every lane, this one carries the wave's maximum key in scalars: the K = 8
// instances of phi4_ens_heun_frames_kernel have no two registers for them.
struct EnsHeunAcc {
    float am;                // per lane: max |p|, |e|, |phi'| after their guards
    unsigned long long key;  // wave-uniform: max over the wave's sites so far of ord(phi') << 32 | bits(d); 0: none
    float mw;                // wave-uniform: the phi' of key, -inf before the first site
};

// ens_frame_sites (below) for a Heun step: the record of the lane's float4 o =
// phi' against the step's input c = phi, both in registers, and the step's
// normals xi: d = |fma(-sigq, xi, phi' - phi)|, the Heun step's drift increment
// h/2 (F(phi) + F(p)) where the Euler record has h F(phi).  mo: max |phi'| of o
// after the guard, 0 in a lane without the quad, whose o is -inf.  A float4
// below the wave's running maximum can neither set nor tie the step's; where
// some lane's reaches it, the lanes take their four sites by stab_site from
// (-inf, 0) and the wave's largest key joins f.key: every site that reaches the
// final maximum was at or above the running one when its quad came, so the key
// is exact.  Every lane of the wave calls it.
template <bool NZ>
__device__ __forceinline__ void ens_heun_sites(const Phi4StepArgs &A, EnsHeunAcc &f, uint32_t fl, const float4 &o,
                                               const float4 &c, const f32x4n &xi, float mo) {
    f.am = vmax(f.am, mo);
    if (__ballot(mo >= f.mw) == 0ull) return;  // max |o| >= max o
    const float o4 = vmax(vmax3(o.x, o.y, o.z), o.w);  // the guard's output: never NaN
    if (__ballot(o4 >= f.mw) == 0ull) return;
    FrameAcc t = frame_acc();
    asm volatile("" : "+v"(fl));
    if (fl & kEnsValid) {
        const float s = NZ ? A.sigq : 0.f;
        stab_site(t, o.x, c.x, xi.a, s);
        stab_site(t, o.y, c.y, xi.b, s);
        stab_site(t, o.z, c.z, xi.c, s);
        stab_site(t, o.w, c.w, xi.d, s);
    }
    const unsigned long long k = dpp_all_max_u64(((unsigned long long)ord_f32(t.m) << 32) | __float_as_uint(t.d));
    if (k > f.key) {  // wave-uniform
        f.key = k;
        f.mw = unord_f32_dev((uint32_t)(k >> 32));
    }
}

// One stochastic Heun step of the lane's K quads: with E the
// update of ens_step at counter s, c <- guard(0.5 (c + E(E(c)))), both
// applications with the normals of s.  The lane keeps phi in c throughout;
// p = E(phi) lives in an image only, and stage 2 reads the lane's own p quad
// back beside its six neighbour reads.  On return cur holds phi' behind a
// block barrier, as after a step of phi4_ens_step_kernel.
//
// TWO (two images): stage 1 reads cur (phi) and writes p to oth, barrier,
// stage 2 reads oth and writes phi' to cur, barrier.  cur is read by stage 1
// and written by stage 2 only, oth the other way round, and a barrier stands
// between every stage and the next: two barriers per step.
// One image: stage 1 forms p into c from the image, barrier (every phi
// neighbour read is done), the lane exchanges its own quads -- phi back from
// the image into c, p into the image: no lane touches another lane's quad --
// barrier, stage 2 forms phi' into c from the image of p, barrier (every p
// read is done), phi' to the image, barrier: four barriers per step.
//
// KEEP: the normals of stage 1 stay in registers for stage 2 (4 K VGPRs);
// otherwise stage 2 evaluates tb_noise again: the same counter and key, so
// the same bits.  am takes max |p|, max |e| and max |phi'|, each after its guard.
//
// FR (phi4_ens_heun_frames_kernel): stage 2 also takes the step's stability
// record into *fa (ens_heun_sites), where phi (the lane's registers), the
// normals and phi' are at hand together; am is fa->am; the quads of lanes
// without one hold -inf, as for ens_step_fr; and the step's last barrier is the
// caller's, which posts the wave's record before it.
template <int K, bool NZ, bool TWO, bool FR = false>
__device__ __forceinline__ void ens_heun(const Phi4StepArgs &A, const EnsGeo &g, float4 (&c)[K],
                                         const EnsFlagsPk<K> &fl, float *cur, float *oth, uint32_t slo, uint32_t shi,
                                         float &am, EnsHeunAcc *fa = nullptr) {
    constexpr bool KEEP = NZ && K <= 4;
    const int T = blockDim.x;
    f32x4n xk[KEEP ? K : 1] = {};
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
                const f32x4n xi = tb_noise<NZ>(A, 0u, (uint32_t)q, slo, shi);
                if constexpr (KEEP) xk[j] = xi;
                float mp;
                const float4 p = site_update4<NZ>(c[j], lft, rgt, up, dn, zm, zp, xi, A, false, f32x2{A.m2, A.m2}, &mp);
                am = fmaxf(am, mp);
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
        float4 *cur4 = reinterpret_cast<float4 *>(cur);
        const float cl = A.clampv;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            uint32_t f = fl.get(j);
            int q = (int)threadIdx.x + j * T;
            asm volatile("" : "+v"(f), "+v"(q));
            if constexpr (FR) {
                const float4 phi = c[j];  // -inf in a lane without this quad: so is its phi' below
                f32x4n xi{};
                float mo = 0.f;
                if (f & kEnsValid) {
                    const EnsNbr n = ens_nbr(g, q, f);
                    const float4 p = img4[q];
                    const float4 up = img4[n.up], dn = img4[n.dn], zm = img4[n.zm], zp = img4[n.zp];
                    const float lft = img[n.lf], rgt = img[n.rg];
                    if constexpr (KEEP) xi = xk[j];
                    else xi = tb_noise<NZ>(A, 0u, (uint32_t)q, slo, shi);
                    float mp;
                    const float4 e =
                        site_update4<NZ>(p, lft, rgt, up, dn, zm, zp, xi, A, false, f32x2{A.m2, A.m2}, &mp);
                    float4 o;
                    o.x = ens_guard(__fmul_rn(0.5f, __fadd_rn(phi.x, e.x)), cl);
                    o.y = ens_guard(__fmul_rn(0.5f, __fadd_rn(phi.y, e.y)), cl);
                    o.z = ens_guard(__fmul_rn(0.5f, __fadd_rn(phi.z, e.z)), cl);
                    o.w = ens_guard(__fmul_rn(0.5f, __fadd_rn(phi.w, e.w)), cl);
                    c[j] = o;
                    mo = fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fmaxf(fabsf(o.z), fabsf(o.w)));  // never NaN
                    am = fmaxf(am, mp);
                    if constexpr (TWO) cur4[q] = o;
                }
                ens_heun_sites<NZ>(A, *fa, f, c[j], phi, xi, mo);
            } else if (f & kEnsValid) {
                const EnsNbr n = ens_nbr(g, q, f);
                const float4 p = img4[q];
                const float4 up = img4[n.up], dn = img4[n.dn], zm = img4[n.zm], zp = img4[n.zp];
                const float lft = img[n.lf], rgt = img[n.rg];
                f32x4n xi;
                if constexpr (KEEP) xi = xk[j];
                else xi = tb_noise<NZ>(A, 0u, (uint32_t)q, slo, shi);
                float mp;
                const float4 e = site_update4<NZ>(p, lft, rgt, up, dn, zm, zp, xi, A, false, f32x2{A.m2, A.m2}, &mp);
                float4 o;
                o.x = ens_guard(__fmul_rn(0.5f, __fadd_rn(c[j].x, e.x)), cl);
                o.y = ens_guard(__fmul_rn(0.5f, __fadd_rn(c[j].y, e.y)), cl);
                o.z = ens_guard(__fmul_rn(0.5f, __fadd_rn(c[j].z, e.z)), cl);
                o.w = ens_guard(__fmul_rn(0.5f, __fadd_rn(c[j].w, e.w)), cl);
                c[j] = o;
                // after the guard: never NaN
                am = fmaxf(am, fmaxf(mp, fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fmaxf(fabsf(o.z), fabsf(o.w)))));
                if constexpr (TWO) cur4[q] = o;
            }
        }
        if constexpr (!TWO) {
            __syncthreads();  // every wave has read p
#pragma unroll
            for (int j = 0; j < K; ++j)
                if (fl.get(j) & kEnsValid) cur4[(int)threadIdx.x + j * T] = c[j];
        }
    }
    if constexpr (!FR) __syncthreads();  // phi' is in cur
}

// frame_sites (sq_phi4.hip) for a lane that may own no quad here: the step's
// stability record of the lane's float4 o into f.  am takes
// every site (mp: site_update4's max |phi'| after the guard); the per-site
// (m, d) update runs only in waves where some float4 reaches the wave's
// running maximum mw, which keeps the wave's maximum key exact.  The inputs of
// o are read back from the image, which holds them until the step's store:
// the lane keeps no second copy of its quad.  Every lane of the wave calls it
// (the wave scan needs them all); a lane without a quad comes with o = -inf
// and mp = 0, below every site, and is tested for only on the per-site path
// (fl made opaque there: no exec mask per quad kept across the step).
template <bool NZ>
__device__ __forceinline__ void ens_frame_sites(const Phi4StepArgs &A, FrameAcc &f, uint32_t fl, const float4 &o,
                                                const float4 *old, const f32x4n &xi, float mp) {
    f.am = vmax(f.am, mp);
    if (__ballot(mp >= f.mw) == 0ull) return;  // max |o| >= max o
    const float o4 = vmax(vmax3(o.x, o.y, o.z), o.w);  // the guard's output: never NaN
    if (__ballot(o4 >= f.mw) == 0ull) return;
    asm volatile("" : "+v"(fl));
    if (fl & kEnsValid) {
        const float4 c = *old;
        const float s = NZ ? A.sigq : 0.f;
        stab_site(f, o.x, c.x, xi.a, s);
        stab_site(f, o.y, c.y, xi.b, s);
        stab_site(f, o.z, c.z, xi.c, s);
        stab_site(f, o.w, c.w, xi.d, s);
    }
    f.mw = dpp_all_max_f(f.m);
}

// ens_step for a frame: the same update, and the step's record in fa.  The
// quads of lanes without one hold -inf (phi4_ens_frames_kernel sets them).
template <int K, bool NZ>
__device__ __forceinline__ void ens_step_fr(const Phi4StepArgs &A, const EnsGeo &g, float4 (&c)[K],
                                            const uint32_t (&fl)[K], const float *img, uint32_t slo, uint32_t shi,
                                            FrameAcc &fa) {
    const float4 *img4 = reinterpret_cast<const float4 *>(img);
    const int T = blockDim.x;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        uint32_t f = fl[j];
        int q = (int)threadIdx.x + j * T;
        asm volatile("" : "+v"(f), "+v"(q));  // as ens_step
        f32x4n xi{};
        float mp = 0.f;
        if (f & kEnsValid) {
            const EnsNbr n = ens_nbr(g, q, f);
            const float4 up = img4[n.up], dn = img4[n.dn], zm = img4[n.zm], zp = img4[n.zp];
            const float lft = img[n.lf], rgt = img[n.rg];
            xi = tb_noise<NZ>(A, 0u, (uint32_t)q, slo, shi);
            c[j] = site_update4<NZ>(c[j], lft, rgt, up, dn, zm, zp, xi, A, false, f32x2{A.m2, A.m2}, &mp);
        }
        ens_frame_sites<NZ>(A, fa, f, c[j], img4 + q, xi, mp);
    }
}

}  // namespace

}  // namespace sq
