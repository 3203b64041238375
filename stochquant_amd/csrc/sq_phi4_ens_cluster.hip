// sq_phi4_ens_cluster.hip -- Swendsen-Wang cluster sweeps of the embedded Ising
// signs of the phi^4 lattice ensemble (Brower, Tamayo).
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
#define SQ_PHI4_ENS_KERNELS_ONLY
#include "sq_phi4_ens.hip"

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

template <int K>
__global__ __launch_bounds__(kPhi4EnsMaxLanes) void phi4_ens_cluster_kernel(const Phi4EnsArgs E,
                                                                             const Phi4EnsClusterArgs W) {
#pragma clang fp contract(off)
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
        }
        return;
    }
    // flips, records, counts
    double sm[4] = {0.0, 0.0, 0.0, 0.0};  // clusters, flipped clusters, flipped sites
    float4 *gf = reinterpret_cast<float4 *>(E.field + (size_t)r * (size_t)(4 * g.Q));
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (fl[j] & kEnsValid) {
            const int q = (int)threadIdx.x + j * T;
            const uint4 o = lab4[q];
            const uint32_t l[4] = {o.x, o.y, o.z, o.w};
            if (W.labels != nullptr)
                reinterpret_cast<int4 *>(W.labels + (size_t)r * (size_t)(4 * g.Q))[q] =
                    make_int4((int)o.x, (int)o.y, (int)o.z, (int)o.w);
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
}

}  // namespace

hipError_t phi4_ens_cluster_launch(const Phi4EnsArgs &a, const Phi4EnsClusterArgs &w, int nrep, hipStream_t s) {
    if (!ens_shape_ok(a) || nrep < 1 || w.stat == nullptr) return hipErrorInvalidValue;
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz);
    const int bytes = sh.mom_lds_bytes;
    Phi4EnsArgs q = a;
    Phi4EnsClusterArgs wq = w;
    void *args[] = {&q, &wq};
    const void *fn = sh.K == 1   ? (const void *)&phi4_ens_cluster_kernel<1>
                     : sh.K == 2 ? (const void *)&phi4_ens_cluster_kernel<2>
                     : sh.K == 4 ? (const void *)&phi4_ens_cluster_kernel<4>
                                 : (const void *)&phi4_ens_cluster_kernel<8>;
    hipError_t e = ens_lds_attr(fn, bytes);
    if (e != hipSuccess) return e;
    return hipLaunchKernel(fn, dim3((unsigned)nrep), dim3((unsigned)sh.T), args, (size_t)bytes, s);
}

}  // namespace sq
