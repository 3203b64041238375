// sq_phi4_ens_exchange.hip -- replica exchange (parallel tempering) between
// neighbouring slots of the phi^4 lattice ensemble.
//
// The R replicas are cut into ladders of nlad consecutive slots.  Round x pairs
// slots (l nlad + o + 2 j, + 1), o = x & 1, inside every ladder l; one
// work-group owns one pair (a, b = a + 1) and is the only reader and the only
// writer of both rows of the field array in the launch.  include/stochquant.h
// has the definition:
//   beta_r = 2 h_r / sig_r^2,  p_r = beta_r (3 + m2_r / 2),  q_r = beta_r lam6_r / 4,
//   Delta = (p_a - p_b)(S2_b - S2_a) - (beta_a - beta_b)(NN_b - NN_a) + (q_a - q_b)(S4_b - S4_a)
// in double from the float records, the sums those of phi4_ens_moments_kernel
// bit for bit; u from Philox at {0, kPhi4EnsStreamExchange << 24, x lo, x hi}
// under slot a's key; verdict 1 when Delta <= 0 or u < exp(-Delta), else 0 (a
// NaN Delta included).  On verdict 1 the two rows and the two walker labels
// change places; on verdict 0 no field word is written.
//
// Course of a work-group (the moments launch's shape: K quads per lane, T
// lanes, one LDS image and the scratch behind it):
//   ens_load phi_a -> registers ca, image              | barrier (ens_load's)
//   ens_sums, ens_fold: lanes 0 .. 3 put the totals at the image's base, which
//   no lane reads any more behind ens_fold's barrier    | barrier
//   every lane takes S2, S4, NN of phi_a into scalars   | barrier (the image is free)
//   the same for phi_b into cb                           | barrier
//   every lane forms Delta, u and the verdict from the same words in the same
//   order: the block branches uniformly, nothing is posted or waited for
//   (phi4_ens_mala_kernel's way); lane 0 writes the counters, the labels and
//   the record; verdict 1: the lanes store cb to row a and ca to row b.
// The loads of both rows are complete before the verdict exists (the sums
// depend on them), so the stores cannot overtake a read of the same row.
// 2 K float4 of field per lane: 64 registers at K = 8.  No atomics: every word
// has one writer.
#include "sq_phi4_ens_dev.h"
#include "sq_phi4_ens_launch.h"

namespace sq {

namespace {

// beta, p, q of one slot's record.
struct XchgCoef {
    double beta, p, q;
};
__device__ __forceinline__ XchgCoef xchg_coef(const Phi4EnsRec &rc) {
#pragma clang fp contract(off)
    const double h = (double)rc.h, sig = (double)rc.sig, m2 = (double)rc.m2, lam6 = (double)rc.lam6;
    XchgCoef c;
    c.beta = 2.0 * h / (sig * sig);
    c.p = c.beta * (3.0 + m2 / 2.0);
    c.q = c.beta * (lam6 / 4.0);
    return c;
}

// Load, sum and fold the field of slot r; on return every lane holds its S2, S4, NN (block-uniform) and the image
// is free: the last statement is a barrier behind every read of it.
template <int K>
__device__ __forceinline__ void xchg_sums(const Phi4EnsArgs &E, const EnsGeo &g, int r, float4 (&c)[K],
                                          uint32_t (&fl)[K], float *img, double *scr, double (&s)[3]) {
    ens_load<K>(E, g, r, c, fl, img);
    double sm[4];
    float mx;
    ens_sums<K>(g, c, fl, img, sm, mx);
    double *tot = reinterpret_cast<double *>(img);  // >= 32 sites: 128 bytes
    ens_fold(sm, mx, scr, tot, false);
    __syncthreads();
    s[0] = readlane_d(tot[1], 0);
    s[1] = readlane_d(tot[2], 0);
    s[2] = readlane_d(tot[3], 0);
    __syncthreads();
}

template <int K>
__global__ __launch_bounds__(kPhi4EnsMaxLanes) void phi4_ens_exchange_kernel(const Phi4EnsArgs E,
                                                                              const Phi4EnsXchgArgs W) {
#pragma clang fp contract(off)
    const int o = (int)(W.x & 1ull);
    const int np = (W.nlad - o) / 2;  // pairs per ladder, >= 1 (the launcher's grid is ladders * np)
    const int l = (int)blockIdx.x / np, j = (int)blockIdx.x % np;
    const int a = l * W.nlad + o + 2 * j, b = a + 1;
    const EnsGeo g = ens_geo(E);
    float *img = reinterpret_cast<float *>(ens_smem);
    double *scr = reinterpret_cast<double *>(ens_smem + 16 * (size_t)g.Q);
    float4 ca[K], cb[K];
    uint32_t fl[K];
    double sa[3], sb[3];  // S2, S4, NN
    xchg_sums<K>(E, g, a, ca, fl, img, scr, sa);
    xchg_sums<K>(E, g, b, cb, fl, img, scr, sb);
    const Phi4EnsRec ra = E.rec[a], rb = E.rec[b];
    const XchgCoef A = xchg_coef(ra), B = xchg_coef(rb);
    const double t2 = (A.p - B.p) * (sb[0] - sa[0]);
    const double tn = (A.beta - B.beta) * (sb[2] - sa[2]);
    const double t4 = (A.q - B.q) * (sb[1] - sa[1]);
    const double D = readlane_d((t2 - tn) + t4, 0);
    const uint32_t xlo = (uint32_t)W.x, xhi = (uint32_t)(W.x >> 32);
    const u32x4 ph = philox4x32_10(u32x4{0u, kPhi4EnsStreamExchange << 24, xlo, xhi}, ra.k0, ra.k1);
    const double u = ((double)ph.x + 0.5) * 0x1p-32;
    int v = 0;
    if (D <= 0.0) v = 1;
    else if (u < exp(-D)) v = 1;  // false for a NaN Delta
    v = __builtin_amdgcn_readfirstlane(v);
    if (threadIdx.x == 0) {
        long long *st = W.stat + 2 * (size_t)a;
        st[0] += 1;
        st[1] += (long long)v;
        int wa = W.walker[a], wb = W.walker[b];
        if (v) {
            const int t = wa;
            wa = wb;
            wb = t;
            W.walker[a] = wa;
            W.walker[b] = wb;
        }
        if (W.rec != nullptr) {
            double *oa = W.rec + 5 * (size_t)a, *ob = oa + 5;
            oa[0] = D;
            oa[1] = u;
            oa[2] = (double)v;
            oa[3] = (double)b;
            oa[4] = (double)wa;
            ob[0] = D;
            ob[1] = u;
            ob[2] = (double)v;
            ob[3] = (double)a;
            ob[4] = (double)wb;
        }
    }
    if (v) {
        const int T = blockDim.x;
        float4 *ga = reinterpret_cast<float4 *>(E.field + (size_t)a * (size_t)(4 * g.Q));
        float4 *gb = reinterpret_cast<float4 *>(E.field + (size_t)b * (size_t)(4 * g.Q));
#pragma unroll
        for (int k = 0; k < K; ++k)
            if (fl[k] & kEnsValid) {
                const int q = (int)threadIdx.x + k * T;
                ga[q] = cb[k];
                gb[q] = ca[k];
            }
    }
}

}  // namespace

hipError_t phi4_ens_exchange_launch(const Phi4EnsArgs &a, const Phi4EnsXchgArgs &w, int nrep, hipStream_t s) {
    if (!ens_shape_ok(a) || nrep < 2 || w.stat == nullptr || w.walker == nullptr || w.nlad < 2 || w.nlad > nrep ||
        nrep % w.nlad != 0)
        return hipErrorInvalidValue;
    const int np = phi4_ens_xchg_pairs(w.nlad, w.x);
    if (np == 0) return hipSuccess;  // nlad = 2, odd round
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz);
    Phi4EnsArgs q = a;
    Phi4EnsXchgArgs wq = w;
    void *args[] = {&q, &wq};
    return ens_launch(SQ_ENS_KERNEL(sh.K, phi4_ens_exchange_kernel), (nrep / w.nlad) * np, sh.T,
                      sh.lds(kPhi4EnsLdsStored).bytes, args, s);
}

}  // namespace sq
