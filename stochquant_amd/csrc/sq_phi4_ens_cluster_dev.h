// sq_phi4_ens_cluster_dev.h -- the kernel of the Swendsen-Wang cluster sweeps
// of the embedded Ising signs of the phi^4 lattice ensemble (Brower, Tamayo;
// DESIGN.md §4.3).  Device code only; its two kinds of instance are launched
// from sq_phi4_ens_cluster.hip (the plain sweep) and
// sq_phi4_ens_cluster_improved.hip (the sweep with the cluster sums).
//
// One work-group owns one replica for one sweep.  include/stochquant.h has the
// definition:
//   beta = 2 h / (sig sig) in double from the float record;
//   site i = (z Ly + y) Lx + x draws the Philox block o_i at counter
//   {i, kPhi4EnsStreamCluster << 24, c lo, c hi} under the replica's key;
//   the forward bond mu of site i to j = i + mu^ is on iff t = phi_i phi_j > 0
//   and (word mu of o_i + 0.5) 2^-32 >= exp(-(2 beta) t);
//   a cluster is a connected component of the on-bonds, its label the smallest
//   site index in it; it flips (sign bit toggled) iff word 3 of o_label is odd.
//
// Course of a work-group (the moments launch's shape: K quads per lane, T
// lanes, one LDS image and the scratch behind it):
//   ens_load phi -> registers c, image                       | barrier (ens_load's)
//   every site's three forward bond bits from the image     | barrier (the floats are read)
//   the bits to the image, one word per site                | barrier
//   every site's three backward bond bits from its x-, y-,
//   z-predecessor's word: 6 bits per site, 24 per quad in bb | barrier (the words are read)
//   label[i] = i to the image, the pass flags cleared       | barrier
//   passes, one barrier each (below)
//   flips from the root's Philox word, computed again from the label; the
//   quads that hold a flipped site stored; the counts folded (ens_fold).
//
// A pass.  Every site takes the minimum m of its own label and the labels of
// its bonded neighbours, then min(m, label[m]) (pointer jumping); if m is
// below its label L it lowers label[L], its parent's word, and its own word
// to m, both by an atomic minimum in LDS (ds_min_u32): a whole subtree is
// hooked under the smaller label at once (lowering only the site's own word
// took 7.6 times as long at the critical point of 32^3).
// Words are read by other lanes with no barrier in between.  That is safe: a word
// only falls (every write is an atomic minimum), every value a word ever
// holds is the index of a site of the same component (it starts as i, and m
// is read from a word of the component of i, whose label L is another site
// of it), and a 32-bit LDS word is read and written whole, so a reader gets
// an older or a newer label, never a foreign one.  A pass in which no lane
// found m < L wrote nothing and saw the same words throughout: every site's
// label is then <= its bonded neighbours' both ways, hence equal over the
// component, and the component's smallest site m holds label[m] <= m from
// its own component, so label[m] = m: the fixed point is the definition's
// labelling, whatever the order of the waves.
//
// The end of the passes.  A lane that lowered a word sets flag[p % 3]; behind the
// pass's barrier every wave reads that word.  Lane 0 clears flag[(p + 1) % 3]
// during pass p: its last readers sat between the barriers of passes p - 2
// and p - 1, its next writers come behind the barrier of pass p.  The loop
// has a bound written here, sites + 1 passes, what plain minimum propagation
// needs in the worst case (after p passes a site holds the minimum over its
// p-neighbourhood); a work-group that reaches it writes no field word, counts
// one unconverged sweep and ends.  It cannot spin.
//
// No global atomics: every device word has one writer (the lane that owns the
// quad; lanes 0 .. 2 the replica's five counters).
//
// The cluster sums (the instances with a trailing Phi4EnsClusterSumArgs, built
// by sq_phi4_ens_cluster_improved.hip; the plain instances keep their argument
// list and, every statement of the sums being behind `if constexpr`, their
// code).  Behind the flips the labels are final
// and the image is free, if a lane keeps the labels of its 4 K sites: in
// registers for K <= 4; for K = 8, which has no 32 registers to spare, in the
// replica's row of a device scratch (Phi4EnsClusterSumArgs::park), together
// with the roots' partial sums, and the magnitudes are read again from the
// field's row.  The image then serves as one 32-bit
// accumulator per possible root.  A site's weight (include/stochquant.h: q,
// a_mu, b_mu, 48-bit signed integers) goes in as three 16-bit limbs, the top
// one signed, one limb per pass:
//   every site adds its limb to acc[label] (ds_add_u32; runs of one label
//   inside a quad are added up first)                          | barrier
//   every root reads its word, keeps the low 16 bits and leaves
//   the upper half, the carry, in the word for the next limb
//   (0 behind the third)                                       | barrier
// 32,768 x 65,535 + 32,767 < 2^31, so no word overflows, and integer addition
// makes the sums independent of the order of the waves.  Behind the third limb
// the root has the sum as int64 and adds its square to the lane's share, which
// ens_fold totals per weight into four doubles behind the scratch (the launch
// asks for 32 bytes more than the plain one): lanes 0 and 1 write the record.
// 7 weights, 21 passes, 42 barriers and 7 folds.  Only roots ever hold a
// non-zero word, so the image is all zero behind the last pass: its base takes
// three integer accumulators (ds_add_u64, ds_max_u64, ds_add_u32) for Mtot,
// Mmax and nsat.
#pragma once
#include "sq_phi4_ens_dev.h"

namespace sq {

namespace {

// The forward bond bit of one link: t = a b in double (exact), w the site's Philox word of the direction.
__device__ __forceinline__ uint32_t clu_bond(float a, float b, uint32_t w, double nb2) {
#pragma clang fp contract(off)
    const double t = (double)a * (double)b;
    if (!(t > 0.0)) return 0u;  // a NaN t, t = 0 and t < 0: off
    const double u = ((double)w + 0.5) * 0x1p-32;
    return u >= exp(nb2 * t) ? 1u : 0u;
}

__device__ __forceinline__ uint32_t clu_min(uint32_t a, uint32_t b) { return a < b ? a : b; }

// One site's weight: q = floor(a 2^32) (t = 1, fl) or rint((a t) 2^32), 0 for a saturated site.
__device__ __forceinline__ bool clu_saturated(float v) { return !(fabs((double)v) < 32768.0); }
__device__ __forceinline__ long long clu_weight(float v, double t, bool fl) {
#pragma clang fp contract(off)
    if (clu_saturated(v)) return 0;
    const double x = (fabs((double)v) * t) * 0x1p32;  // |x| < 2^47
    // x + 1.5 2^52 rounds x to an integer, ties to even, and holds it in the low bits of its significand
    return __double_as_longlong((fl ? floor(x) : x) + 0x1.8p52) - __double_as_longlong(0x1.8p52);
}

template <typename... XA>
__device__ __forceinline__ Phi4EnsClusterSumArgs clu_sum_args(const XA &...x) {
    static_assert(sizeof...(XA) <= 1, "at most one Phi4EnsClusterSumArgs");
    const Phi4EnsClusterSumArgs a[] = {x..., Phi4EnsClusterSumArgs{}};
    return a[0];
}

// XA empty: the plain sweep.  XA = {Phi4EnsClusterSumArgs}: the sweep with the cluster sums.
template <int K, typename... XA>
__global__ __launch_bounds__(kPhi4EnsMaxLanes) void phi4_ens_cluster_kernel(const Phi4EnsArgs E,
                                                                             const Phi4EnsClusterArgs W,
                                                                             const XA... xa) {
#pragma clang fp contract(off)
    constexpr bool IMP = sizeof...(XA) != 0;
    constexpr bool PARK = K == 8;  // phi4_ens_cluster_sum_shape's rule
    const Phi4EnsClusterSumArgs X = clu_sum_args(xa...);
    const int r = blockIdx.x;
    const EnsGeo g = ens_geo(E);
    const int T = blockDim.x;
    float *img = reinterpret_cast<float *>(ens_smem);
    uint32_t *lab = reinterpret_cast<uint32_t *>(ens_smem);
    uint4 *lab4 = reinterpret_cast<uint4 *>(ens_smem);
    double *scr = reinterpret_cast<double *>(ens_smem + 16 * (size_t)g.Q);
    uint32_t *flag = reinterpret_cast<uint32_t *>(scr + 16 * 4);  // three words of the scratch's float part
    float4 c[K];
    uint32_t fl[K], bb[K];
    ens_load<K>(E, g, r, c, fl, img);
    const Phi4EnsRec rc = E.rec[r];
    const double beta = 2.0 * (double)rc.h / ((double)rc.sig * (double)rc.sig);
    const double nb2 = -(2.0 * beta);
    const uint32_t clo = (uint32_t)W.c, chi = (uint32_t)(W.c >> 32);
    constexpr uint32_t kStr = kPhi4EnsStreamCluster << 24;

    // forward bonds: bits 3 s + mu of bb[j], s the site of the quad
    {
        const float4 *img4 = reinterpret_cast<const float4 *>(img);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            bb[j] = 0u;
            if (fl[j] & kEnsValid) {
                const int q = (int)threadIdx.x + j * T;
                const EnsNbr n = ens_nbr(g, q, fl[j]);
                const float4 dn = img4[n.dn], zp = img4[n.zp];
                const float rg = img[n.rg];
                const float own[5] = {c[j].x, c[j].y, c[j].z, c[j].w, rg};
                const float yn[4] = {dn.x, dn.y, dn.z, dn.w}, zn[4] = {zp.x, zp.y, zp.z, zp.w};
                uint32_t b = 0u;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const u32x4 o = philox4x32_10(u32x4{(uint32_t)(4 * q + s), kStr, clo, chi}, rc.k0, rc.k1);
                    b |= clu_bond(own[s], own[s + 1], o.x, nb2) << (3 * s);
                    b |= clu_bond(own[s], yn[s], o.y, nb2) << (3 * s + 1);
                    b |= clu_bond(own[s], zn[s], o.z, nb2) << (3 * s + 2);
                }
                bb[j] = b;
            }
        }
    }
    __syncthreads();  // every float of the image is read
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (fl[j] & kEnsValid) {
            const int q = (int)threadIdx.x + j * T;
            const uint32_t b = bb[j];
            lab4[q] = make_uint4(b & 7u, (b >> 3) & 7u, (b >> 6) & 7u, (b >> 9) & 7u);
            if (W.bonds != nullptr)
                reinterpret_cast<uint32_t *>(W.bonds + (size_t)r * (size_t)(4 * g.Q))[q] =
                    (b & 7u) | (((b >> 3) & 7u) << 8) | (((b >> 6) & 7u) << 16) | (((b >> 9) & 7u) << 24);
        }
    __syncthreads();
    // backward bonds: bb[j] becomes 6 bits per site, bits 6 s + (0 .. 2) forward x, y, z, + (3 .. 5) backward
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (fl[j] & kEnsValid) {
            const int q = (int)threadIdx.x + j * T;
            const EnsNbr n = ens_nbr(g, q, fl[j]);
            const uint4 up = lab4[n.up], zm = lab4[n.zm];
            const uint32_t lf = lab[n.lf];
            const uint32_t f = bb[j];
            const uint32_t yb[4] = {up.x, up.y, up.z, up.w}, zb[4] = {zm.x, zm.y, zm.z, zm.w};
            uint32_t b = 0u;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const uint32_t xb = s == 0 ? (lf & 1u) : ((f >> (3 * (s - 1))) & 1u);
                const uint32_t six = ((f >> (3 * s)) & 7u) | (xb << 3) | (((yb[s] >> 1) & 1u) << 4) |
                                     (((zb[s] >> 2) & 1u) << 5);
                b |= six << (6 * s);
            }
            bb[j] = b;
        }
    __syncthreads();  // every bond word of the image is read
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (fl[j] & kEnsValid) {
            const int q = (int)threadIdx.x + j * T;
            lab4[q] = make_uint4(4u * q, 4u * q + 1u, 4u * q + 2u, 4u * q + 3u);
        }
    if (threadIdx.x < 3) flag[threadIdx.x] = 0u;
    __syncthreads();

    // the passes
    const int bound = 4 * g.Q + 1;
    bool conv = false;
    for (int p = 0; p < bound; ++p) {
        const int fp = p % 3;
        if (threadIdx.x == 0) flag[fp == 2 ? 0 : fp + 1] = 0u;
        bool stored = false;
#pragma unroll
        for (int j = 0; j < K; ++j) {
            uint32_t f = fl[j];
            int q = (int)threadIdx.x + j * T;
            asm volatile("" : "+v"(f), "+v"(q));  // the offsets are recomputed per pass, not kept (ens_step)
            if (f & kEnsValid) {
                const uint32_t b = bb[j];
                const EnsNbr n = ens_nbr(g, q, f);
                const uint4 o = lab4[q];
                uint32_t m[4] = {o.x, o.y, o.z, o.w};
                const uint32_t own[4] = {o.x, o.y, o.z, o.w};
                if (b & 0x00082082u) {  // a forward y-bond in the quad (bits 6 s + 1)
                    const uint4 v = lab4[n.dn];
                    const uint32_t a[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        if ((b >> (6 * s + 1)) & 1u) m[s] = clu_min(m[s], a[s]);
                }
                if (b & 0x00410410u) {  // a backward y-bond
                    const uint4 v = lab4[n.up];
                    const uint32_t a[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        if ((b >> (6 * s + 4)) & 1u) m[s] = clu_min(m[s], a[s]);
                }
                if (b & 0x00104104u) {  // a forward z-bond
                    const uint4 v = lab4[n.zp];
                    const uint32_t a[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        if ((b >> (6 * s + 2)) & 1u) m[s] = clu_min(m[s], a[s]);
                }
                if (b & 0x00820820u) {  // a backward z-bond
                    const uint4 v = lab4[n.zm];
                    const uint32_t a[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        if ((b >> (6 * s + 5)) & 1u) m[s] = clu_min(m[s], a[s]);
                }
                if ((b >> 3) & 1u) m[0] = clu_min(m[0], lab[n.lf]);   // site 0's backward x-bond
                if ((b >> 18) & 1u) m[3] = clu_min(m[3], lab[n.rg]);  // site 3's forward x-bond
#pragma unroll
                for (int s = 0; s < 3; ++s)
                    if ((b >> (6 * s)) & 1u) {  // the x-bonds inside the quad, both ways
                        m[s] = clu_min(m[s], own[s + 1]);
                        m[s + 1] = clu_min(m[s + 1], own[s]);
                    }
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    m[s] = clu_min(m[s], lab[m[s]]);  // m[s] < 4 Q: an index of the image
                    if (m[s] < own[s]) {
                        // the site's parent takes the label as well (own[s] == i for a root: one operation)
                        atomicMin(&lab[own[s]], m[s]);
                        if (own[s] != (uint32_t)(4 * q + s)) atomicMin(&lab[4 * q + s], m[s]);
                        stored = true;
                    }
                }
            }
        }
        if (stored) flag[fp] = 1u;
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane((int)flag[fp]) == 0) {
            conv = true;
            break;
        }
    }

    long long *st = W.stat + 5 * (size_t)r;
    if (!conv) {  // block-uniform: no field word is written
        if (threadIdx.x == 0) {
            st[0] += 1;
            st[4] += 1;
            if constexpr (IMP) {
                double *o = X.series + 8 * (size_t)r;
#pragma unroll
                for (int i = 0; i < 7; ++i) o[i] = 0.0;
                o[7] = -1.0;
            }
        }
        return;
    }
    // flips, records, counts
    double sm[4] = {0.0, 0.0, 0.0, 0.0};  // clusters, flipped clusters, flipped sites
    float4 *gf = reinterpret_cast<float4 *>(E.field + (size_t)r * (size_t)(4 * g.Q));
    // the sums' copy of the labels: L in registers, or parked in the replica's row of X.park, where a root's word
    // (its own index, which the root bit says as well) later holds its partial sum; bit 8 + s of fl[j]: site s of
    // the quad is a root
    uint4 L[IMP && !PARK ? K : 1];
    int4 *pk = nullptr;
    if constexpr (IMP && PARK) pk = reinterpret_cast<int4 *>(X.park + (size_t)r * (size_t)(4 * g.Q));
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (fl[j] & kEnsValid) {
            const int q = (int)threadIdx.x + j * T;
            const uint4 o = lab4[q];
            const uint32_t l[4] = {o.x, o.y, o.z, o.w};
            if (W.labels != nullptr)
                reinterpret_cast<int4 *>(W.labels + (size_t)r * (size_t)(4 * g.Q))[q] =
                    make_int4((int)o.x, (int)o.y, (int)o.z, (int)o.w);
            if constexpr (IMP) {
                if constexpr (PARK) {
                    pk[q] = make_int4((int)o.x, (int)o.y, (int)o.z, (int)o.w);
                } else {
                    L[j] = o;
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) fl[j] |= (l[s] == (uint32_t)(4 * q + s) ? 1u : 0u) << (8 + s);
            }
            uint32_t fb = 0u, prev = 0u;
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                uint32_t odd;
                if (s > 0 && l[s] == l[s - 1]) odd = prev;
                else odd = philox4x32_10(u32x4{l[s], kStr, clo, chi}, rc.k0, rc.k1).w & 1u;
                prev = odd;
                fb |= odd << s;
                const bool root = l[s] == (uint32_t)(4 * q + s);
                sm[0] += root ? 1.0 : 0.0;
                sm[1] += (root && odd) ? 1.0 : 0.0;
                sm[2] += odd ? 1.0 : 0.0;
            }
            if (fb) {
                float4 v = c[j];
                v.x = __uint_as_float(__float_as_uint(v.x) ^ ((fb & 1u) << 31));
                v.y = __uint_as_float(__float_as_uint(v.y) ^ (((fb >> 1) & 1u) << 31));
                v.z = __uint_as_float(__float_as_uint(v.z) ^ (((fb >> 2) & 1u) << 31));
                v.w = __uint_as_float(__float_as_uint(v.w) ^ (((fb >> 3) & 1u) << 31));
                gf[q] = v;
            }
        }
    // the totals to the image's base, which no lane reads any more behind ens_fold's barrier (>= 32 sites)
    double *tot = reinterpret_cast<double *>(ens_smem);
    ens_fold(sm, 0.f, scr, tot, false);
    if (threadIdx.x < 3) st[1 + threadIdx.x] += (long long)tot[threadIdx.x];
    if (threadIdx.x == 0) st[0] += 1;

    if constexpr (IMP) {
        // the cluster sums
        double *ctot = reinterpret_cast<double *>(ens_smem + 16 * (size_t)g.Q + kPhi4EnsScratchBytes);  // 4 doubles
        double *o = X.series + 8 * (size_t)r;
        long long *wrow = X.weights != nullptr ? X.weights + (size_t)r * (size_t)(4 * g.Q) * 7 : nullptr;
        double mmax = 0.0, fa = 0.0;
        long long mtot = 0;
        uint32_t nsat = 0u;
        uint32_t lo[PARK ? 1 : K][4];  // a root's low 32 bits of the sum while the limbs come in (parked: in pk)
        __syncthreads();    // every label and total of the image is read
#pragma unroll
        for (int j = 0; j < K; ++j)
            if (fl[j] & kEnsValid) lab4[(int)threadIdx.x + j * T] = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
#pragma unroll 1
        for (int wi = 0; wi < 7; ++wi) {
            const int ax = wi == 0 ? 0 : (wi - 1) >> 1;  // the weight's axis; wi odd: the cosine, even: the sine
            const int La = ax == 0 ? E.Lx : (ax == 1 ? E.Ly : E.Lz);
            const double *tp = X.tab + (ax == 0 ? 0 : (ax == 1 ? 2 * E.Lx : 2 * (E.Lx + E.Ly))) + ((wi & 1) ? 0 : La);
            double fs[4] = {0.0, 0.0, 0.0, 0.0};  // the lane's share of the sum of squares, of fourth powers
#pragma unroll 1
            for (int lb = 0; lb < 3; ++lb) {
                // every site's limb lb of weight wi to its root's word
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    uint32_t f = fl[j];
                    int q = (int)threadIdx.x + j * T;
                    asm volatile("" : "+v"(f), "+v"(q));  // nothing formed from them is kept over the passes
                    if (f & kEnsValid) {
                        uint4 lq;
                        if constexpr (PARK) {
                            const int4 p = pk[q];
                            lq = make_uint4((uint32_t)p.x, (uint32_t)p.y, (uint32_t)p.z, (uint32_t)p.w);
                        } else {
                            lq = L[j];
                        }
                        uint32_t l[4] = {lq.x, lq.y, lq.z, lq.w};
                        if constexpr (PARK) {
#pragma unroll
                            for (int s = 0; s < 4; ++s)
                                if ((f >> (8 + s)) & 1u) l[s] = (uint32_t)(4 * q + s);  // the word holds its sum
                        }
                        // the magnitudes: the lane's registers, or (parked: no register to spare) the row of the
                        // field, where the flips changed sign bits only and this lane alone writes the quad
                        const float4 cv = PARK ? gf[q] : c[j];
                        float v[4] = {cv.x, cv.y, cv.z, cv.w};
                        asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));  // the weights neither
                        double t[4] = {1.0, 1.0, 1.0, 1.0};
                        if (wi != 0) {
                            if (ax == 0) {
                                const int x0 = 4 * (q & (g.qrow - 1));
#pragma unroll
                                for (int s = 0; s < 4; ++s) t[s] = tp[x0 + s];
                            } else {
                                const int yz = q / g.qrow;
                                t[0] = t[1] = t[2] = t[3] = tp[ax == 1 ? yz % E.Ly : yz / E.Ly];
                            }
                        }
                        int run = 0;
                        uint32_t rl = l[0];
#pragma unroll
                        for (int s = 0; s < 4; ++s) {
                            const long long w = clu_weight(v[s], t[s], wi == 0);
                            const int limb = lb == 2 ? (int)(w >> 32) : (int)((w >> (16 * lb)) & 0xFFFF);
                            if (wi == 0 && lb == 0) nsat += clu_saturated(v[s]) ? 1u : 0u;
                            if (s > 0 && l[s] != rl) {
                                if (run != 0) atomicAdd(&lab[rl], (uint32_t)run);
                                run = 0;
                                rl = l[s];
                            }
                            run += limb;
                        }
                        if (run != 0) atomicAdd(&lab[rl], (uint32_t)run);  // rl < 4 Q: a label
                    }
                    // one quad at a time: eight quads' loads in flight at once cost the K = 8 instance its registers
                    if constexpr (PARK) __builtin_amdgcn_sched_barrier(0);
                }
                __syncthreads();
                // every root takes its word and leaves the carry; behind the third limb it has the sum
#pragma unroll
                for (int j = 0; j < K; ++j) {
                    uint32_t f = fl[j];
                    int q = (int)threadIdx.x + j * T;
                    asm volatile("" : "+v"(f), "+v"(q));
                    if (f & kEnsValid) {
                        long long sum[4] = {0, 0, 0, 0};
                        if (f & 0xF00u) {
                            const uint4 a = lab4[q];
                            const uint32_t w4[4] = {a.x, a.y, a.z, a.w};
                            uint32_t back[4] = {0u, 0u, 0u, 0u};
                            uint32_t pw[4] = {0u, 0u, 0u, 0u};  // the parked words of the quad
                            if constexpr (PARK) {
                                const int4 p = pk[q];
                                pw[0] = (uint32_t)p.x, pw[1] = (uint32_t)p.y, pw[2] = (uint32_t)p.z, pw[3] = (uint32_t)p.w;
                            }
#pragma unroll
                            for (int s = 0; s < 4; ++s)
                                if ((f >> (8 + s)) & 1u) {
                                    uint32_t &keep = PARK ? pw[s] : lo[PARK ? 0 : j][s];
                                    if (lb == 0) {
                                        keep = w4[s] & 0xFFFFu;
                                        back[s] = w4[s] >> 16;
                                    } else if (lb == 1) {
                                        keep |= (w4[s] & 0xFFFFu) << 16;
                                        back[s] = w4[s] >> 16;
                                    } else {
                                        sum[s] = (long long)(((unsigned long long)w4[s] << 32) |
                                                             (unsigned long long)keep);
                                        const double m = (double)sum[s] * 0x1p-32;
                                        const double m2 = m * m;
                                        fs[0] += m2;
                                        fs[1] += m2 * m2;
                                        if (wi == 0) {
                                            mmax = fmax(mmax, m);
                                            mtot += sum[s];
                                        }
                                    }
                                }
                            lab4[q] = make_uint4(back[0], back[1], back[2], back[3]);
                            if constexpr (PARK) {
                                if (lb != 2) pk[q] = make_int4((int)pw[0], (int)pw[1], (int)pw[2], (int)pw[3]);
                            }
                        }
                        if (lb == 2 && wrow != nullptr) {
#pragma unroll
                            for (int s = 0; s < 4; ++s) wrow[(size_t)(4 * q + s) * 7 + (size_t)wi] = sum[s];
                        }
                    }
                }
                __syncthreads();
            }
            // the weight's totals: I2 and I4 of M; F_mu = sum A_mu^2 + sum B_mu^2, each in the fold's order
            ens_fold(fs, 0.f, scr, ctot, false);
            if (threadIdx.x == 0) {
                const double v = ctot[0];
                if (wi == 0) o[0] = v;
                else if (wi & 1) fa = v;
                else o[2 + ax] = fa + v;
            } else if (threadIdx.x == 1 && wi == 0) {
                o[1] = ctot[1];
            }
        }
        // the image is all zero (only roots ever held a word, and their last carry is 0): its first words take
        // Mtot, Mmax (a non-negative double orders as its bits) and nsat
        unsigned long long *a64 = reinterpret_cast<unsigned long long *>(lab);
        if (mtot != 0) atomicAdd(a64, (unsigned long long)mtot);
        if (mmax != 0.0) atomicMax(a64 + 1, (unsigned long long)__double_as_longlong(mmax));
        if (nsat != 0u) atomicAdd(lab + 4, nsat);
        __syncthreads();
        if (threadIdx.x == 0) {
            o[5] = __longlong_as_double((long long)a64[1]);
            o[6] = (double)(long long)a64[0] * 0x1p-32;
            o[7] = (double)lab[4];
        }
    }
}

}  // namespace

}  // namespace sq
