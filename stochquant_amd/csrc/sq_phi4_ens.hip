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
//
// phi4_ens_frames_kernel runs whole frames the same way: per
// step the block's stability record behind the step's own barrier, the rule,
// an early exit once it has fired; per frame the verdict, the Δτ controller
// and the store to / reload from the replica's HBM field, its snapshot.
//
// The correlator instances of both kernels add ens_corr, the zero-momentum
// time-slice correlator over z of the field in the image, accumulated per
// replica in device memory; phi4_ens_slices_kernel is the same routine on the
// stored field.  The momentum instances add ens_pcorr, the same correlator
// projected on spatial momenta (p_x, p_y); phi4_ens_pslices_kernel is that
// routine on the stored field.
//
// phi4_ens_heun_kernel is the step kernel with the second-order stochastic
// Heun step in place of the Euler one: phi' = guard(0.5 (phi + E(E(phi)))), E
// the update above applied twice with the normals of one counter (ens_heun).
// phi4_ens_heun_frames_kernel runs whole frames of such steps: the frames
// kernel's rule, exit, verdict, controller and snapshot around ens_heun, the
// step's record taken of phi' against the Heun step's input.
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

// two != 0: two LDS images (the launcher sized the dynamic LDS for them).
// With the correlator: one ens_corr measurement after each every-th step into
// the replica's rows, the slice sums behind the scratch; the series as without
// it when E.series is given.  With momenta: ens_pcorr_measure in its place.
template <int K, typename... CA>
__global__ __launch_bounds__(kPhi4EnsMaxLanes) void phi4_ens_step_kernel(const Phi4EnsArgs E, const int two,
                                                                          const CA... ca) {
    constexpr bool PC = kEnsPCorr<CA...>;
    constexpr bool CORR = sizeof...(CA) != 0;  // either kind of measurement
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
        if ((CORR || E.series != nullptr) && --left == 0) {
            left = E.every;
            if (!CORR || E.series != nullptr) {
                double sm[4];
                float mx;
                ens_sums<K>(g, c, fl, cur, sm, mx);
                ens_fold(sm, mx, scr, E.series + 4 * ((size_t)rec * gridDim.x + (size_t)r), false);
                ++rec;
            }
            if constexpr (PC) {
                ens_pcorr_measure(g, E, r, cur, scr + kPhi4EnsScratchBytes / 8, ens_pcorr_args(ca...));
            } else if constexpr (CORR) {
                const Phi4EnsCorrArgs C = ens_corr_args(ca...);
                ens_corr<true>(g, E.Lz, cur, scr + kPhi4EnsScratchBytes / 8, C.G + (size_t)r * (size_t)(E.Lz / 2 + 1),
                               C.S1 + r, C.nmeas + r, nullptr);
            }
        }
    }
    float4 *gf = reinterpret_cast<float4 *>(E.field + (size_t)r * (size_t)(4 * g.Q));
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (fl[j] & kEnsValid) gf[(int)threadIdx.x + j * T] = c[j];
    // some site was clamped (NaN -> +clamp) iff the running max after the guard reached the clamp
    if (am >= E.clampv) E.flags[r] = 1;
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

// phi4_ens_step_kernel with ens_heun as its step (sq_phi4_ens_step_heun): the
// same arguments, LDS layout and work-group shape, the counter advancing by one
// per Heun step; cur is img0 for the whole call.  The measurement code behind
// the step is that kernel's, `left` / `every` counting Heun steps.
template <int K, typename... CA>
__global__ __launch_bounds__(kPhi4EnsMaxLanes) void phi4_ens_heun_kernel(const Phi4EnsArgs E, const int two,
                                                                          const CA... ca) {
    constexpr bool PC = kEnsPCorr<CA...>;
    constexpr bool CORR = sizeof...(CA) != 0;  // either kind of measurement
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
    float am = 0.f;
    const unsigned long long s0 = rc.step + E.adv;
    int left = E.every;  // steps until the next measurement
    int rec = 0;
    for (int t = 0; t < E.nsteps; ++t) {
        const unsigned long long s = s0 + (unsigned long long)t;
        const uint32_t slo = (uint32_t)s, shi = (uint32_t)(s >> 32);
        if (two) {
            if (nz) ens_heun<K, true, true>(A, g, c, fl, cur, oth, slo, shi, am);
            else ens_heun<K, false, true>(A, g, c, fl, cur, oth, slo, shi, am);
        } else {
            if (nz) ens_heun<K, true, false>(A, g, c, fl, cur, oth, slo, shi, am);
            else ens_heun<K, false, false>(A, g, c, fl, cur, oth, slo, shi, am);
        }
        if ((CORR || E.series != nullptr) && --left == 0) {
            left = E.every;
            if (!CORR || E.series != nullptr) {
                double sm[4];
                float mx;
                uint32_t f[K];
#pragma unroll
                for (int j = 0; j < K; ++j) f[j] = fl.get(j);
                ens_sums<K>(g, c, f, cur, sm, mx);
                ens_fold(sm, mx, scr, E.series + 4 * ((size_t)rec * gridDim.x + (size_t)r), false);
                ++rec;
            }
            if constexpr (PC) {
                ens_pcorr_measure(g, E, r, cur, scr + kPhi4EnsScratchBytes / 8, ens_pcorr_args(ca...));
            } else if constexpr (CORR) {
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
    // a stage's guarded maximum or the final guard reached the clamp
    if (am >= E.clampv) E.flags[r] = 1;
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

// n frames of replica blockIdx.x, all decided here: per step the block's
// record (M, D, A) through LDS atomic maxima behind the step's own barrier,
// the stability rule on the carried T and V, an early exit once it has fired;
// per frame the verdict, the Δτ controller and the new coefficients
// (frame_decide / phi4_base_args, operation for operation), then the store
// of the adopted field to HBM -- the next frame's snapshot -- or the reload
// of registers and image from it.  The noise counter advances by loops per
// frame either way.
//
// The step records rotate through three LDS slots: step s posts to slot s % 3
// before its barrier, every lane reads it after, and lane 0 then clears slot
// (s + 2) % 3 -- last read before this barrier, next posted after the next one.
//
// CORR: one ens_corr measurement of the adopted field after every stable frame
// (after the verdict: cur holds that field and every wave is past the last
// step's barrier); a rolled-back frame measures nothing.  With momenta:
// ens_pcorr_measure in its place.
template <int K, typename... CA>
__global__ __launch_bounds__(kPhi4EnsMaxLanes) void phi4_ens_frames_kernel(const Phi4EnsArgs E,
                                                                            const Phi4EnsFrameArgs F, const int two,
                                                                            const CA... ca) {
    constexpr bool PC = kEnsPCorr<CA...>;
    constexpr bool CORR = sizeof...(CA) != 0;  // either kind of measurement
    const int r = blockIdx.x;
    const EnsGeo g = ens_geo(E);
    const Phi4EnsRec rc = E.rec[r];
    const Phi4EnsFrameState st = F.st[r];
    Phi4StepArgs A{};
    A.h = rc.h;
    A.m2 = rc.m2;
    A.lam6 = rc.lam6;
    A.sig = rc.sig;
    A.sigq = rc.sigq;
    A.clampv = E.clampv;
    A.k0 = rc.k0;
    A.k1 = rc.k1;
    const bool nz = rc.sig != 0.0f;
    float *img0 = reinterpret_cast<float *>(ens_smem);
    float *img1 = two ? img0 + 4 * g.Q : img0;
    char *sb = ens_smem + (size_t)(two ? 2 : 1) * 16 * (size_t)g.Q;
    double *scr = reinterpret_cast<double *>(sb);
    unsigned long long *fk = reinterpret_cast<unsigned long long *>(sb + kPhi4EnsScratchBytes);  // [3]
    uint32_t *fw = reinterpret_cast<uint32_t *>(fk + 3);  // [0..2] max |phi'| of a step, [3], [4] the start field's
    if (threadIdx.x < 3) fk[threadIdx.x] = 0ull;
    if (threadIdx.x < 5) fw[threadIdx.x] = 0u;
    float4 c[K];
    uint32_t fl[K];
    ens_load<K>(E, g, r, c, fl, img0);  // ends in a barrier
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (!(fl[j] & kEnsValid)) c[j].x = c[j].y = c[j].z = c[j].w = -__builtin_inff();  // ens_step_fr
    const int T = blockDim.x;
    const bool lane0 = (threadIdx.x & 63) == 0;
    float sT = st.T, sV = st.V;
    if (!st.init) {  // the replica's first frame ever: max phi and max |phi| of its start field
        float mp = -__builtin_inff(), ma = 0.f;
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (fl[j] & kEnsValid) {
                mp = fmaxf(mp, fmaxf(fmaxf(c[j].x, c[j].y), fmaxf(c[j].z, c[j].w)));
                ma = fmaxf(ma, fmaxf(fmaxf(fabsf(c[j].x), fabsf(c[j].y)), fmaxf(fabsf(c[j].z), fabsf(c[j].w))));
            }
        mp = dpp_all_max_f(mp);
        ma = dpp_all_max_f(ma);
        if (lane0) {
            atomicMax(&fw[3], ord_f32(mp));
            atomicMax(&fw[4], __float_as_uint(ma));
        }
        __syncthreads();
        sT = unord_f32_dev(fw[3]);
        sV = __uint_as_float(fw[4]);
    }
    sT = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(sT)));
    sV = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(sV)));
    double dtau = st.dtau;
    int cnt = st.cnt, fired = -1, gflag = 0, exec = 0, sticky = 0;
    int slot = 0;
    const int L = F.loops;
    const unsigned long long s0 = rc.step + E.adv;
    float *cur = img0, *oth = img1;
    float4 *gf = reinterpret_cast<float4 *>(E.field + (size_t)r * (size_t)(4 * g.Q));
    float *recM = F.recs + (size_t)r * 3 * (size_t)L, *recD = recM + L, *recA = recD + L;
    for (int f = 0; f < F.nframes; ++f) {
        fired = -1;
        gflag = 0;
        const unsigned long long sf = s0 + (unsigned long long)f * (unsigned long long)L;
        for (int t = 0; t < L; ++t) {
            const unsigned long long s = sf + (unsigned long long)t;
            const uint32_t slo = (uint32_t)s, shi = (uint32_t)(s >> 32);
            FrameAcc fa = frame_acc();
            if (nz) ens_step_fr<K, true>(A, g, c, fl, cur, slo, shi, fa);
            else ens_step_fr<K, false>(A, g, c, fl, cur, slo, shi, fa);
            // the wave's key from the lanes that hold its maximum (frame_flush2), its max |phi'| by a scan
            if (fa.m >= fa.mw && fa.mw > -__builtin_inff())
                atomicMax(&fk[slot], ((unsigned long long)ord_f32(fa.m) << 32) | __float_as_uint(fa.d));
            const uint32_t wa = (uint32_t)dpp_all_max_i((int)__float_as_uint(fminf(fa.am, A.clampv)));
            if (lane0) atomicMax(&fw[slot], wa);
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
            const unsigned long long key = fk[slot];
            const uint32_t kM = __builtin_amdgcn_readfirstlane((uint32_t)(key >> 32));
            const float M = unord_f32_dev(kM);
            const float D = __uint_as_float(__builtin_amdgcn_readfirstlane((uint32_t)key));
            const float Am = __uint_as_float(__builtin_amdgcn_readfirstlane(fw[slot]));
            const int clr = slot == 0 ? 2 : slot - 1;
            slot = slot == 2 ? 0 : slot + 1;
            if (threadIdx.x == 0) {
                fk[clr] = 0ull;
                fw[clr] = 0u;
                recM[t] = M;
                recD[t] = D;
                recA[t] = Am;
            }
            ++exec;
            if (Am >= E.clampv) gflag = 1;  // some site was clamped (NaN -> +clamp)
            const bool fire = M > sT && D > sV;  // stab_rule (sq_phi4_frames.cpp)
            sT = M;
            sV = sV < Am ? Am : sV;
            if (fire) {
                fired = t;
                break;  // the verdict is settled, T and V frozen: the rest of the frame is skipped
            }
        }
        sticky |= gflag;
        const int stable = (gflag == 0 && fired < 0) ? 1 : 0;
        if (F.adapt) {  // frame_decide
            if (stable) {
                if (cnt > 10) {
                    cnt = 0;
                    dtau /= 0.950;
                }
                cnt += 1;
            } else {
                dtau *= 0.950;
                cnt = 0;
            }
        }
        const float hf = (float)dtau;  // phi4_base_args
        A.h = hf;
        A.sig = (float)(__builtin_sqrt(2.0 * (double)hf) * st.C);
        A.sigq = (float)(__builtin_sqrt(2.0 * (double)hf) * st.C * kSqrt2Ln2);
        // q opaque per frame: hoisted out of the frame loop, the K 64-bit addresses of the lane's quads
        // take 2 K registers for the whole call
        if (stable) {
#pragma unroll
            for (int j = 0; j < K; ++j) {
                int q = (int)threadIdx.x + j * T;
                asm volatile("" : "+v"(q));
                if (fl[j] & kEnsValid) gf[q] = c[j];
            }
        } else {
            // every wave is past the last step's barrier and reads no image before the next one
            float4 *cur4 = reinterpret_cast<float4 *>(cur);
#pragma unroll
            for (int j = 0; j < K; ++j) {
                int q = (int)threadIdx.x + j * T;
                asm volatile("" : "+v"(q));
                if (fl[j] & kEnsValid) {
                    c[j] = gf[q];
                    cur4[q] = c[j];
                }
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            F.stable[(size_t)f * gridDim.x + (size_t)r] = stable;
            F.dtau[(size_t)f * gridDim.x + (size_t)r] = dtau;
        }
        if (E.series != nullptr) {
            double sm[4];
            float mx;
            ens_sums<K>(g, c, fl, cur, sm, mx);
            ens_fold(sm, mx, scr, E.series + 4 * ((size_t)f * gridDim.x + (size_t)r), false);
        }
        if constexpr (PC) {
            if (stable)  // block-uniform, as below
                ens_pcorr_measure(g, E, r, cur, reinterpret_cast<double *>(sb + kPhi4EnsFrameScratchBytes),
                                  ens_pcorr_args(ca...));
        } else if constexpr (CORR) {
            if (stable) {  // block-uniform: every lane decided the frame from the same records
                const Phi4EnsCorrArgs C = ens_corr_args(ca...);
                ens_corr<true>(g, E.Lz, cur, reinterpret_cast<double *>(sb + kPhi4EnsFrameScratchBytes),
                               C.G + (size_t)r * (size_t)(E.Lz / 2 + 1), C.S1 + r, C.nmeas + r, nullptr);
            }
        }
    }
    if (threadIdx.x == 0) {
        Phi4EnsFrameState o = st;
        o.dtau = dtau;
        o.T = sT;
        o.V = sV;
        o.init = 1;
        o.cnt = cnt;
        o.fired = fired;
        o.flag = gflag;
        o.exec = exec;
        F.st[r] = o;
        if (sticky) E.flags[r] = 1;
    }
}

// phi4_ens_frames_kernel with ens_heun as its step (sq_phi4_ens_run_frames_heun,
// DESIGN.md §4.3): the same frame state, rule, controller, snapshot, records,
// series and measurements, the counter advancing by one per Heun step and by
// loops per frame.  The step's record comes from ens_heun's stage 2; the wave's
// key and maximum go to the rotating slot before the step's last barrier, which
// stands here, and are read behind it: no barrier beyond ens_heun's two (TWO)
// or four.  TWO is a template parameter: cur is img0 for the whole call, and the
// one-image K = 8 instances have no register for a run-time choice.
//
// LDS hazards.  Within a step they are ens_heun's: TWO, stage 1 reads cur and
// writes oth, barrier, stage 2 reads oth and writes cur, barrier; one image,
// stage 1 reads it, barrier, the lanes exchange their own quads, barrier, stage 2
// reads it, barrier, phi' to it, barrier.  Behind a step's last barrier no wave
// reads an image before stage 1 of the next step (the record slots, the scratch
// and the measurement regions lie behind the images), and stage 1 never writes
// cur.  So the snapshot reload, which follows the frame's last executed step,
// writes the lane's own quads of cur with no wave reading them, and its own
// barrier puts them in front of every later reader: ens_sums, the measurement
// and the next frame's stage 1.
template <int K, bool TWO, typename... CA>
__global__ __launch_bounds__(kPhi4EnsMaxLanes) void phi4_ens_heun_frames_kernel(const Phi4EnsArgs E,
                                                                                 const Phi4EnsFrameArgs F,
                                                                                 const CA... ca) {
    constexpr bool PC = kEnsPCorr<CA...>;
    constexpr bool CORR = sizeof...(CA) != 0;  // either kind of measurement
    const int r = blockIdx.x;
    const EnsGeo g = ens_geo(E);
    const Phi4EnsRec rc = E.rec[r];
    const Phi4EnsFrameState st = F.st[r];
    Phi4StepArgs A{};
    A.h = rc.h;
    A.m2 = rc.m2;
    A.lam6 = rc.lam6;
    A.sig = rc.sig;
    A.sigq = rc.sigq;
    A.clampv = E.clampv;
    A.k0 = rc.k0;
    A.k1 = rc.k1;
    const bool nz = rc.sig != 0.0f;
    float *cur = reinterpret_cast<float *>(ens_smem);
    float *oth = TWO ? cur + 4 * g.Q : cur;
    char *sb = ens_smem + (size_t)(TWO ? 2 : 1) * 16 * (size_t)g.Q;
    unsigned long long *fk = reinterpret_cast<unsigned long long *>(sb + kPhi4EnsScratchBytes);  // [3]
    uint32_t *fw = reinterpret_cast<uint32_t *>(fk + 3);  // [0..2] a step's maximum, [3], [4] the start field's
    if (threadIdx.x < 3) fk[threadIdx.x] = 0ull;
    if (threadIdx.x < 5) fw[threadIdx.x] = 0u;
    float4 c[K];
    EnsFlagsPk<K> fl;
    float sT = st.T, sV = st.V;
    {
        uint32_t f[K];
        ens_load<K>(E, g, r, c, f, cur);  // ends in a barrier
        fl.pack(f);
        float mp = -__builtin_inff(), ma = 0.f;  // max phi and max |phi| of the start field (the first frame ever)
#pragma unroll
        for (int j = 0; j < K; ++j) {
            if (f[j] & kEnsValid) {
                mp = fmaxf(mp, fmaxf(fmaxf(c[j].x, c[j].y), fmaxf(c[j].z, c[j].w)));
                ma = fmaxf(ma, fmaxf(fmaxf(fabsf(c[j].x), fabsf(c[j].y)), fmaxf(fabsf(c[j].z), fabsf(c[j].w))));
            } else {
                c[j].x = c[j].y = c[j].z = c[j].w = -__builtin_inff();  // ens_heun<FR>
            }
        }
        if (!st.init) {
            mp = dpp_all_max_f(mp);
            ma = dpp_all_max_f(ma);
            if ((threadIdx.x & 63) == 0) {
                atomicMax(&fw[3], ord_f32(mp));
                atomicMax(&fw[4], __float_as_uint(ma));
            }
            __syncthreads();
            sT = unord_f32_dev(fw[3]);
            sV = __uint_as_float(fw[4]);
        }
    }
    sT = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(sT)));
    sV = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(sV)));
    double dtau = st.dtau;
    int cnt = st.cnt, fired = -1, gflag = 0, exec = 0, sticky = 0;
    int slot = 0;
    const unsigned long long s0 = rc.step + E.adv;
    for (int f = 0; f < F.nframes; ++f) {
        fired = -1;
        gflag = 0;
        const unsigned long long sf = s0 + (unsigned long long)f * (unsigned long long)F.loops;
        for (int t = 0; t < F.loops; ++t) {
            const unsigned long long s = sf + (unsigned long long)t;
            const uint32_t slo = (uint32_t)s, shi = (uint32_t)(s >> 32);
            EnsHeunAcc fa{0.f, 0ull, -__builtin_inff()};
            if (nz) ens_heun<K, true, TWO, true>(A, g, c, fl, cur, oth, slo, shi, fa.am, &fa);
            else ens_heun<K, false, TWO, true>(A, g, c, fl, cur, oth, slo, shi, fa.am, &fa);
            // the wave's key (a wave without a quad has none) and its largest magnitude, by a scan
            const uint32_t wa = (uint32_t)dpp_all_max_i((int)__float_as_uint(fminf(fa.am, A.clampv)));
            unsigned tid = threadIdx.x;
            asm volatile("" : "+v"(tid));  // opaque per step: no lane mask is hoisted and kept in scalars
            if ((tid & 63) == 0) {
                if (fa.mw > -__builtin_inff()) atomicMax(&fk[slot], fa.key);
                atomicMax(&fw[slot], wa);
            }
            __syncthreads();  // the step's last barrier: phi' is in cur, the records are posted
            const unsigned long long key = fk[slot];
            const uint32_t kM = __builtin_amdgcn_readfirstlane((uint32_t)(key >> 32));
            const float M = unord_f32_dev(kM);
            const float D = __uint_as_float(__builtin_amdgcn_readfirstlane((uint32_t)key));
            const float Am = __uint_as_float(__builtin_amdgcn_readfirstlane(fw[slot]));
            const int clr = slot == 0 ? 2 : slot - 1;
            slot = slot == 2 ? 0 : slot + 1;
            if (tid == 0) {
                fk[clr] = 0ull;
                fw[clr] = 0u;
                float *rec = F.recs + (size_t)r * 3 * (size_t)F.loops + t;  // M | D | A rows of loops entries
                rec[0] = M;
                rec[F.loops] = D;
                rec[2 * F.loops] = Am;
            }
            ++exec;
            if (Am >= E.clampv) gflag = 1;  // a stage's guarded maximum or the final guard reached the clamp
            const bool fire = M > sT && D > sV;  // stab_rule (sq_phi4_frames.cpp)
            sT = M;
            sV = sV < Am ? Am : sV;
            if (fire) {
                fired = t;
                break;  // the verdict is settled, T and V frozen: the rest of the frame is skipped
            }
        }
        sticky |= gflag;
        const int stable = (gflag == 0 && fired < 0) ? 1 : 0;
        if (F.adapt) {  // frame_decide
            if (stable) {
                if (cnt > 10) {
                    cnt = 0;
                    dtau /= 0.950;
                }
                cnt += 1;
            } else {
                dtau *= 0.950;
                cnt = 0;
            }
        }
        const float hf = (float)dtau;  // phi4_base_args
        A.h = hf;
        A.sig = (float)(__builtin_sqrt(2.0 * (double)hf) * st.C);
        A.sigq = (float)(__builtin_sqrt(2.0 * (double)hf) * st.C * kSqrt2Ln2);
        unsigned tid = threadIdx.x;
        asm volatile("" : "+v"(tid));  // opaque per frame: what the code below forms from it is not hoisted and kept
        {
            // the lane's addresses are formed per frame (q opaque): hoisted, they take 2 K registers for the call
            float4 *gf = reinterpret_cast<float4 *>(E.field + (size_t)r * (size_t)(4 * g.Q));
            float4 *cur4 = reinterpret_cast<float4 *>(cur);
            const int T = blockDim.x;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                int q = (int)tid + j * T;
                asm volatile("" : "+v"(q));
                if (fl.get(j) & kEnsValid) {
                    if (stable) {
                        gf[q] = c[j];  // the next frame's snapshot
                    } else {
                        c[j] = gf[q];
                        cur4[q] = c[j];  // no wave reads cur here (see above)
                    }
                }
            }
            if (!stable) __syncthreads();  // block-uniform: every lane decided the frame from the same records
        }
        if (tid == 0) {
            F.stable[(size_t)f * gridDim.x + (size_t)r] = stable;
            F.dtau[(size_t)f * gridDim.x + (size_t)r] = dtau;
        }
        if (E.series != nullptr) {
            double sm[4];
            float mx;
            uint32_t fu[K];
#pragma unroll
            for (int j = 0; j < K; ++j) fu[j] = fl.get(j);
            ens_sums<K>(g, c, fu, cur, sm, mx);
            ens_fold(sm, mx, reinterpret_cast<double *>(sb), E.series + 4 * ((size_t)f * gridDim.x + (size_t)r), false,
                     tid);
        }
        if constexpr (PC) {
            if (stable)  // block-uniform
                ens_pcorr_measure(g, E, r, cur, reinterpret_cast<double *>(sb + kPhi4EnsFrameScratchBytes),
                                  ens_pcorr_args(ca...), tid);
        } else if constexpr (CORR) {
            if (stable) {
                const Phi4EnsCorrArgs C = ens_corr_args(ca...);
                ens_corr<true>(g, E.Lz, cur, reinterpret_cast<double *>(sb + kPhi4EnsFrameScratchBytes),
                               C.G + (size_t)r * (size_t)(E.Lz / 2 + 1), C.S1 + r, C.nmeas + r, nullptr, tid);
            }
        }
    }
    if (threadIdx.x == 0) {
        Phi4EnsFrameState o = st;
        o.dtau = dtau;
        o.T = sT;
        o.V = sV;
        o.init = 1;
        o.cnt = cnt;
        o.fired = fired;
        o.flag = gflag;
        o.exec = exec;
        F.st[r] = o;
        if (sticky) E.flags[r] = 1;
    }
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

// ens_corr on the stored field of replica first + blockIdx.x, accumulating
// nothing: S[blockIdx.x][Lz], g[blockIdx.x][nt].
template <int K>
__global__ __launch_bounds__(kPhi4EnsMaxLanes) void phi4_ens_slices_kernel(const Phi4EnsArgs E, const int first,
                                                                            double *S, double *gout) {
    const int r = first + blockIdx.x;
    const EnsGeo g = ens_geo(E);
    float *img = reinterpret_cast<float *>(ens_smem);
    double *Sl = reinterpret_cast<double *>(ens_smem + 16 * (size_t)g.Q + kPhi4EnsScratchBytes);
    float4 c[K];
    uint32_t fl[K];
    ens_load<K>(E, g, r, c, fl, img);  // ends in a barrier
    ens_corr<false>(g, E.Lz, img, Sl, gout + (size_t)blockIdx.x * (size_t)(E.Lz / 2 + 1), nullptr, nullptr,
                    S + (size_t)blockIdx.x * (size_t)E.Lz);
}

// ens_pcorr on the stored field of replica first + blockIdx.x, accumulating
// nothing: AB[blockIdx.x][M][Lz][2], g[blockIdx.x][M][nt].
template <int K>
__global__ __launch_bounds__(kPhi4EnsMaxLanes) void phi4_ens_pslices_kernel(const Phi4EnsArgs E,
                                                                             const Phi4EnsPCorrArgs P, const int first,
                                                                             double *AB, double *gout) {
    const int r = first + blockIdx.x;
    const EnsGeo g = ens_geo(E);
    float *img = reinterpret_cast<float *>(ens_smem);
    double *Pl = reinterpret_cast<double *>(ens_smem + 16 * (size_t)g.Q + kPhi4EnsScratchBytes);
    float4 c[K];
    uint32_t fl[K];
    ens_load<K>(E, g, r, c, fl, img);  // ends in a barrier
    ens_pcorr<false>(g, E.Ly, E.Lz, img, Pl, P, gout + (size_t)blockIdx.x * (size_t)(P.M * (E.Lz / 2 + 1)), nullptr,
                     AB + (size_t)blockIdx.x * (size_t)(P.M * 2 * E.Lz));
}

#ifndef SQ_PHI4_ENS_KERNELS_ONLY  // sq_phi4_ens_flow.hip includes the device functions and templates, not what follows
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

#endif  // SQ_PHI4_ENS_KERNELS_ONLY

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

#ifndef SQ_PHI4_ENS_KERNELS_ONLY  // the launchers below belong to this translation unit alone
Phi4EnsShape phi4_ens_shape(int sites, int Lz) {
    Phi4EnsShape s;
    const int Q = sites / 4;
    s.K = Q <= kPhi4EnsMaxLanes ? 1 : (Q <= 2 * kPhi4EnsMaxLanes ? 2 : (Q <= 4 * kPhi4EnsMaxLanes ? 4 : 8));
    s.T = (((Q + s.K - 1) / s.K) + 63) / 64 * 64;
    s.two = 2 * 4 * sites + kPhi4EnsScratchBytes <= kPhi4EnsLdsBytes;
    s.lds_bytes = (s.two ? 2 : 1) * 4 * sites + kPhi4EnsScratchBytes;
    // the frames launch: the same layout, with the frame records' words behind the scratch
    s.fr_two = 2 * 4 * sites + kPhi4EnsFrameScratchBytes <= kPhi4EnsLdsBytes;
    s.fr_lds_bytes = (s.fr_two ? 2 : 1) * 4 * sites + kPhi4EnsFrameScratchBytes;
    s.mom_lds_bytes = 4 * sites + kPhi4EnsScratchBytes;
    // the correlator launches: Lz doubles behind the scratch, sized by their own rule
    const int sl = 8 * Lz;
    s.co_two = 2 * 4 * sites + kPhi4EnsScratchBytes + sl <= kPhi4EnsLdsBytes;
    s.co_lds_bytes = (s.co_two ? 2 : 1) * 4 * sites + kPhi4EnsScratchBytes + sl;
    s.co_fr_two = 2 * 4 * sites + kPhi4EnsFrameScratchBytes + sl <= kPhi4EnsLdsBytes;
    s.co_fr_lds_bytes = (s.co_fr_two ? 2 : 1) * 4 * sites + kPhi4EnsFrameScratchBytes + sl;
    s.sl_lds_bytes = 4 * sites + kPhi4EnsScratchBytes + sl;
    // the momentum launches: 2 Lz doubles there; legal when one image fits in each of the three
    const int pl = 16 * Lz;
    s.pc_two = 2 * 4 * sites + kPhi4EnsScratchBytes + pl <= kPhi4EnsLdsBytes;
    s.pc_lds_bytes = (s.pc_two ? 2 : 1) * 4 * sites + kPhi4EnsScratchBytes + pl;
    s.pc_fr_two = 2 * 4 * sites + kPhi4EnsFrameScratchBytes + pl <= kPhi4EnsLdsBytes;
    s.pc_fr_lds_bytes = (s.pc_fr_two ? 2 : 1) * 4 * sites + kPhi4EnsFrameScratchBytes + pl;
    s.pc_sl_lds_bytes = 4 * sites + kPhi4EnsScratchBytes + pl;
    s.pc_ok = Lz > 0 && s.pc_lds_bytes <= kPhi4EnsLdsBytes && s.pc_fr_lds_bytes <= kPhi4EnsLdsBytes &&
              s.pc_sl_lds_bytes <= kPhi4EnsLdsBytes;
    return s;
}

namespace {
bool ens_pcorr_ok(const Phi4EnsPCorrArgs &p, bool acc) {
    return p.cx != nullptr && p.sx != nullptr && p.cy != nullptr && p.sy != nullptr && p.M >= 1 &&
           p.M <= kPhi4EnsMaxMomenta && (!acc || (p.Gp != nullptr && p.nmeas_p != nullptr)) &&
           (p.corr.G == nullptr || (p.corr.S1 != nullptr && p.corr.nmeas != nullptr));
}
}  // namespace

hipError_t phi4_ens_step_pcorr_launch(const Phi4EnsArgs &a, const Phi4EnsPCorrArgs &p, int nrep, hipStream_t s) {
    if (!ens_shape_ok(a) || a.flags == nullptr || nrep < 1 || a.nsteps < 0 || a.every < 1 || !ens_pcorr_ok(p, true))
        return hipErrorInvalidValue;
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz, a.Lz);
    if (!sh.pc_ok) return hipErrorInvalidValue;
    Phi4EnsArgs q = a;
    Phi4EnsPCorrArgs pq = p;
    int two = sh.pc_two ? 1 : 0;
    void *args[] = {&q, &two, &pq};
    const void *fn = sh.K == 1   ? (const void *)&phi4_ens_step_kernel<1, Phi4EnsPCorrArgs>
                     : sh.K == 2 ? (const void *)&phi4_ens_step_kernel<2, Phi4EnsPCorrArgs>
                     : sh.K == 4 ? (const void *)&phi4_ens_step_kernel<4, Phi4EnsPCorrArgs>
                                 : (const void *)&phi4_ens_step_kernel<8, Phi4EnsPCorrArgs>;
    hipError_t e = ens_lds_attr(fn, sh.pc_lds_bytes);
    if (e != hipSuccess) return e;
    return hipLaunchKernel(fn, dim3((unsigned)nrep), dim3((unsigned)sh.T), args, (size_t)sh.pc_lds_bytes, s);
}

hipError_t phi4_ens_frames_pcorr_launch(const Phi4EnsArgs &a, const Phi4EnsFrameArgs &f, const Phi4EnsPCorrArgs &p,
                                        int nrep, hipStream_t s) {
    if (!ens_shape_ok(a) || a.flags == nullptr || nrep < 1 || f.nframes < 1 || f.loops < 1 || f.st == nullptr ||
        f.stable == nullptr || f.dtau == nullptr || f.recs == nullptr || !ens_pcorr_ok(p, true))
        return hipErrorInvalidValue;
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz, a.Lz);
    if (!sh.pc_ok) return hipErrorInvalidValue;
    int two = sh.pc_fr_two ? 1 : 0;
    const int bytes = sh.pc_fr_lds_bytes;
    Phi4EnsArgs q = a;
    Phi4EnsFrameArgs fq = f;
    Phi4EnsPCorrArgs pq = p;
    void *args[] = {&q, &fq, &two, &pq};
    const void *fn = sh.K == 1   ? (const void *)&phi4_ens_frames_kernel<1, Phi4EnsPCorrArgs>
                     : sh.K == 2 ? (const void *)&phi4_ens_frames_kernel<2, Phi4EnsPCorrArgs>
                     : sh.K == 4 ? (const void *)&phi4_ens_frames_kernel<4, Phi4EnsPCorrArgs>
                                 : (const void *)&phi4_ens_frames_kernel<8, Phi4EnsPCorrArgs>;
    hipError_t e = ens_lds_attr(fn, bytes);
    if (e != hipSuccess) return e;
    return hipLaunchKernel(fn, dim3((unsigned)nrep), dim3((unsigned)sh.T), args, (size_t)bytes, s);
}

hipError_t phi4_ens_pslices_launch(const Phi4EnsArgs &a, const Phi4EnsPCorrArgs &p, int first, int count, double *AB,
                                   double *g, hipStream_t s) {
    if (!ens_shape_ok(a) || first < 0 || count < 1 || AB == nullptr || g == nullptr || !ens_pcorr_ok(p, false))
        return hipErrorInvalidValue;
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz, a.Lz);
    if (!sh.pc_ok) return hipErrorInvalidValue;
    const int bytes = sh.pc_sl_lds_bytes;
    Phi4EnsArgs q = a;
    Phi4EnsPCorrArgs pq = p;
    void *args[] = {&q, &pq, &first, &AB, &g};
    const void *fn = sh.K == 1   ? (const void *)&phi4_ens_pslices_kernel<1>
                     : sh.K == 2 ? (const void *)&phi4_ens_pslices_kernel<2>
                     : sh.K == 4 ? (const void *)&phi4_ens_pslices_kernel<4>
                                 : (const void *)&phi4_ens_pslices_kernel<8>;
    hipError_t e = ens_lds_attr(fn, bytes);
    if (e != hipSuccess) return e;
    return hipLaunchKernel(fn, dim3((unsigned)count), dim3((unsigned)sh.T), args, (size_t)bytes, s);
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

hipError_t phi4_ens_step_corr_launch(const Phi4EnsArgs &a, const Phi4EnsCorrArgs &c, int nrep, hipStream_t s) {
    if (!ens_shape_ok(a) || a.flags == nullptr || nrep < 1 || a.nsteps < 0 || a.every < 1 || c.G == nullptr ||
        c.S1 == nullptr || c.nmeas == nullptr)
        return hipErrorInvalidValue;
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz, a.Lz);
    Phi4EnsArgs q = a;
    Phi4EnsCorrArgs cq = c;
    int two = sh.co_two ? 1 : 0;
    void *args[] = {&q, &two, &cq};
    const void *fn = sh.K == 1   ? (const void *)&phi4_ens_step_kernel<1, Phi4EnsCorrArgs>
                     : sh.K == 2 ? (const void *)&phi4_ens_step_kernel<2, Phi4EnsCorrArgs>
                     : sh.K == 4 ? (const void *)&phi4_ens_step_kernel<4, Phi4EnsCorrArgs>
                                 : (const void *)&phi4_ens_step_kernel<8, Phi4EnsCorrArgs>;
    hipError_t e = ens_lds_attr(fn, sh.co_lds_bytes);
    if (e != hipSuccess) return e;
    return hipLaunchKernel(fn, dim3((unsigned)nrep), dim3((unsigned)sh.T), args, (size_t)sh.co_lds_bytes, s);
}

namespace {
template <typename... CA>
const void *ens_heun_fn(int K) {
    return K == 1   ? (const void *)&phi4_ens_heun_kernel<1, CA...>
           : K == 2 ? (const void *)&phi4_ens_heun_kernel<2, CA...>
           : K == 4 ? (const void *)&phi4_ens_heun_kernel<4, CA...>
                    : (const void *)&phi4_ens_heun_kernel<8, CA...>;
}
}  // namespace

hipError_t phi4_ens_heun_launch(const Phi4EnsArgs &a, const Phi4EnsCorrArgs *c, const Phi4EnsPCorrArgs *p, int nrep,
                                hipStream_t s) {
    const bool meas = c != nullptr || p != nullptr;
    if (!ens_shape_ok(a) || a.flags == nullptr || nrep < 1 || a.nsteps < 0 || a.every < (meas ? 1 : 0) ||
        (a.series != nullptr && a.every < 1) || (c != nullptr && p != nullptr))
        return hipErrorInvalidValue;
    if (c != nullptr && (c->G == nullptr || c->S1 == nullptr || c->nmeas == nullptr)) return hipErrorInvalidValue;
    if (p != nullptr && !ens_pcorr_ok(*p, true)) return hipErrorInvalidValue;
    // the step launches' layouts, each by its own rule
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz, meas ? a.Lz : 0);
    if (p != nullptr && !sh.pc_ok) return hipErrorInvalidValue;
    int two = (p ? sh.pc_two : c ? sh.co_two : sh.two) ? 1 : 0;
    const int bytes = p ? sh.pc_lds_bytes : c ? sh.co_lds_bytes : sh.lds_bytes;
    Phi4EnsArgs q = a;
    Phi4EnsCorrArgs cq = c ? *c : Phi4EnsCorrArgs{};
    Phi4EnsPCorrArgs pq = p ? *p : Phi4EnsPCorrArgs{};
    void *args[] = {&q, &two, p ? (void *)&pq : (void *)&cq};  // the plain instances take the first two
    const void *fn = p   ? ens_heun_fn<Phi4EnsPCorrArgs>(sh.K)
                     : c ? ens_heun_fn<Phi4EnsCorrArgs>(sh.K)
                         : ens_heun_fn<>(sh.K);
    hipError_t e = ens_lds_attr(fn, bytes);
    if (e != hipSuccess) return e;
    return hipLaunchKernel(fn, dim3((unsigned)nrep), dim3((unsigned)sh.T), args, (size_t)bytes, s);
}

namespace {
template <bool TWO, typename... CA>
const void *ens_heun_frames_fn(int K) {
    return K == 1   ? (const void *)&phi4_ens_heun_frames_kernel<1, TWO, CA...>
           : K == 2 ? (const void *)&phi4_ens_heun_frames_kernel<2, TWO, CA...>
           : K == 4 ? (const void *)&phi4_ens_heun_frames_kernel<4, TWO, CA...>
                    : (const void *)&phi4_ens_heun_frames_kernel<8, TWO, CA...>;
}
}  // namespace

hipError_t phi4_ens_heun_frames_launch(const Phi4EnsArgs &a, const Phi4EnsFrameArgs &f, const Phi4EnsCorrArgs *c,
                                       const Phi4EnsPCorrArgs *p, int nrep, hipStream_t s) {
    if (!ens_shape_ok(a) || a.flags == nullptr || nrep < 1 || f.nframes < 1 || f.loops < 1 || f.st == nullptr ||
        f.stable == nullptr || f.dtau == nullptr || f.recs == nullptr || (c != nullptr && p != nullptr))
        return hipErrorInvalidValue;
    if (c != nullptr && (c->G == nullptr || c->S1 == nullptr || c->nmeas == nullptr)) return hipErrorInvalidValue;
    if (p != nullptr && !ens_pcorr_ok(*p, true)) return hipErrorInvalidValue;
    // the frames launches' layouts, each by its own rule
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz, (c || p) ? a.Lz : 0);
    if (p != nullptr && !sh.pc_ok) return hipErrorInvalidValue;
    const bool two = p ? sh.pc_fr_two : c ? sh.co_fr_two : sh.fr_two;
    const int bytes = p ? sh.pc_fr_lds_bytes : c ? sh.co_fr_lds_bytes : sh.fr_lds_bytes;
    Phi4EnsArgs q = a;
    Phi4EnsFrameArgs fq = f;
    Phi4EnsCorrArgs cq = c ? *c : Phi4EnsCorrArgs{};
    Phi4EnsPCorrArgs pq = p ? *p : Phi4EnsPCorrArgs{};
    void *args[] = {&q, &fq, p ? (void *)&pq : (void *)&cq};  // the plain instances take the first two
    const void *fn = p   ? (two ? ens_heun_frames_fn<true, Phi4EnsPCorrArgs>(sh.K)
                                : ens_heun_frames_fn<false, Phi4EnsPCorrArgs>(sh.K))
                     : c ? (two ? ens_heun_frames_fn<true, Phi4EnsCorrArgs>(sh.K)
                                : ens_heun_frames_fn<false, Phi4EnsCorrArgs>(sh.K))
                         : (two ? ens_heun_frames_fn<true>(sh.K) : ens_heun_frames_fn<false>(sh.K));
    hipError_t e = ens_lds_attr(fn, bytes);
    if (e != hipSuccess) return e;
    return hipLaunchKernel(fn, dim3((unsigned)nrep), dim3((unsigned)sh.T), args, (size_t)bytes, s);
}

hipError_t phi4_ens_frames_launch(const Phi4EnsArgs &a, const Phi4EnsFrameArgs &f, int nrep, hipStream_t s) {
    if (!ens_shape_ok(a) || a.flags == nullptr || nrep < 1 || f.nframes < 1 || f.loops < 1 || f.st == nullptr ||
        f.stable == nullptr || f.dtau == nullptr || f.recs == nullptr)
        return hipErrorInvalidValue;
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz);
    int two = sh.fr_two ? 1 : 0;
    const int bytes = sh.fr_lds_bytes;
    Phi4EnsArgs q = a;
    Phi4EnsFrameArgs fq = f;
    void *args[] = {&q, &fq, &two};
    const void *fn = sh.K == 1   ? (const void *)&phi4_ens_frames_kernel<1>
                     : sh.K == 2 ? (const void *)&phi4_ens_frames_kernel<2>
                     : sh.K == 4 ? (const void *)&phi4_ens_frames_kernel<4>
                                 : (const void *)&phi4_ens_frames_kernel<8>;
    hipError_t e = ens_lds_attr(fn, bytes);
    if (e != hipSuccess) return e;
    return hipLaunchKernel(fn, dim3((unsigned)nrep), dim3((unsigned)sh.T), args, (size_t)bytes, s);
}

hipError_t phi4_ens_frames_corr_launch(const Phi4EnsArgs &a, const Phi4EnsFrameArgs &f, const Phi4EnsCorrArgs &c,
                                       int nrep, hipStream_t s) {
    if (!ens_shape_ok(a) || a.flags == nullptr || nrep < 1 || f.nframes < 1 || f.loops < 1 || f.st == nullptr ||
        f.stable == nullptr || f.dtau == nullptr || f.recs == nullptr || c.G == nullptr || c.S1 == nullptr ||
        c.nmeas == nullptr)
        return hipErrorInvalidValue;
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz, a.Lz);
    int two = sh.co_fr_two ? 1 : 0;
    const int bytes = sh.co_fr_lds_bytes;
    Phi4EnsArgs q = a;
    Phi4EnsFrameArgs fq = f;
    Phi4EnsCorrArgs cq = c;
    void *args[] = {&q, &fq, &two, &cq};
    const void *fn = sh.K == 1   ? (const void *)&phi4_ens_frames_kernel<1, Phi4EnsCorrArgs>
                     : sh.K == 2 ? (const void *)&phi4_ens_frames_kernel<2, Phi4EnsCorrArgs>
                     : sh.K == 4 ? (const void *)&phi4_ens_frames_kernel<4, Phi4EnsCorrArgs>
                                 : (const void *)&phi4_ens_frames_kernel<8, Phi4EnsCorrArgs>;
    hipError_t e = ens_lds_attr(fn, bytes);
    if (e != hipSuccess) return e;
    return hipLaunchKernel(fn, dim3((unsigned)nrep), dim3((unsigned)sh.T), args, (size_t)bytes, s);
}

hipError_t phi4_ens_slices_launch(const Phi4EnsArgs &a, int first, int count, double *S, double *g, hipStream_t s) {
    if (!ens_shape_ok(a) || first < 0 || count < 1 || S == nullptr || g == nullptr) return hipErrorInvalidValue;
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz, a.Lz);
    const int bytes = sh.sl_lds_bytes;
    Phi4EnsArgs q = a;
    void *args[] = {&q, &first, &S, &g};
    const void *fn = sh.K == 1   ? (const void *)&phi4_ens_slices_kernel<1>
                     : sh.K == 2 ? (const void *)&phi4_ens_slices_kernel<2>
                     : sh.K == 4 ? (const void *)&phi4_ens_slices_kernel<4>
                                 : (const void *)&phi4_ens_slices_kernel<8>;
    hipError_t e = ens_lds_attr(fn, bytes);
    if (e != hipSuccess) return e;
    return hipLaunchKernel(fn, dim3((unsigned)count), dim3((unsigned)sh.T), args, (size_t)bytes, s);
}

hipError_t phi4_ens_moments_launch(const Phi4EnsArgs &a, int first, int count, double *out, hipStream_t s) {
    if (!ens_shape_ok(a) || first < 0 || count < 1 || out == nullptr) return hipErrorInvalidValue;
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz);
    const int bytes = sh.mom_lds_bytes;
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
#endif  // SQ_PHI4_ENS_KERNELS_ONLY

}  // namespace sq
