// sq_qm1d_ens.hip -- R independent QM1D chains (Jacobi order, Philox noise,
// fp64) per launch: one work-group per replica, blockIdx.x = replica, the wave
// and site tiling of the single-chain register kernel (qm1d_wave_shape,
// N <= 4096).  Replica r computes, bit for bit, what qm1d_frame_wave and the
// host bookkeeping of sq_qm1d_host.cpp (qm1d_frame; adapt: sq_phi4_frames.cpp) compute for a chain with
// that replica's key and state.  What differs from the single-chain path:
//   * the frame scalars come from the replica's device record (EnsRec), and the
//     kernel derives h, sigma and sigma_w from the record's Δτ with the host's
//     expressions;
//   * the field-independent work -- omega's recurrence, the site normals,
//     potID 3's x_cl and ddPot -- is generated inside the kernel (with every CU
//     busy there is no idle chip to precompute tables on, and tables would
//     grow with R x loops x N): omega and the three wave-uniform tanhf of 64
//     steps at once, one step per lane; the site normals one Philox call per
//     lane per 4 / K steps, the quad's components handed round by DPP
//     quad_perm (a lane owns K of a quad's 4 sites); a one-wave potID 3 chain
//     gets them from an LDS table of a few steps that helper waves of its
//     work-group keep ahead of it (HELP below);
//   * adoption and the Δτ controller run at the end of the kernel: a stable
//     frame stores f, x, xx0, omega and adds loops to runs, an unstable one
//     stores none of them (the field lives in registers for the whole frame, so
//     the rollback is free); either way lrgEl, lrgVl, the tick, the verdict,
//     the stable-frame count and Δτ are updated.
// Replicas never communicate: no flags, no polling, no co-residency.
#include <type_traits>

#include "sq_dpp.h"
#include "sq_ens.h"
#include "sq_qm1d_math.h"
#include "sq_rng.h"

namespace sq {

namespace {

// The site normals of 4 / K consecutive steps for a lane's K sites.  The K
// sites [K t, K t + K) of thread t lie in quad q = K t / 4, which G = 4 / K
// neighbouring lanes share: lane g of the group draws the quad of step j + g,
// and z[s][k] collects, for step j + s, component K g + k from lane s of the
// group.  All lanes of the wave are active here.
template <int K>
struct SiteNoise {
    float z[4 / K][K];
};

template <int CTRL>
__device__ __forceinline__ f32x4n quad_perm4(const f32x4n &n) {
    return f32x4n{dpp_f<CTRL, 0xf, 0xf>(n.a, 0.f), dpp_f<CTRL, 0xf, 0xf>(n.b, 0.f), dpp_f<CTRL, 0xf, 0xf>(n.c, 0.f),
                  dpp_f<CTRL, 0xf, 0xf>(n.d, 0.f)};
}

template <int K>
__device__ __forceinline__ void site_noise(SiteNoise<K> &Z, int tid, unsigned long long step, uint32_t k0, uint32_t k1) {
    constexpr int G = 4 / K;
    const int g = tid & (G - 1);
    const unsigned long long st = step + (unsigned long long)g;
    const f32x4n n = normals4((unsigned long long)((tid * K) >> 2), kStreamField, (uint32_t)st, (uint32_t)(st >> 32), k0, k1);
    if constexpr (K == 4) {
        Z.z[0][0] = n.a;
        Z.z[0][1] = n.b;
        Z.z[0][2] = n.c;
        Z.z[0][3] = n.d;
    } else if constexpr (K == 2) {
        const f32x4n s0 = quad_perm4<0xA0>(n), s1 = quad_perm4<0xF5>(n);  // quad_perm:[0,0,2,2], [1,1,3,3]
        Z.z[0][0] = g ? s0.c : s0.a;
        Z.z[0][1] = g ? s0.d : s0.b;
        Z.z[1][0] = g ? s1.c : s1.a;
        Z.z[1][1] = g ? s1.d : s1.b;
    } else {
        const f32x4n s0 = quad_perm4<0x00>(n), s1 = quad_perm4<0x55>(n), s2 = quad_perm4<0xAA>(n),
                     s3 = quad_perm4<0xFF>(n);  // quad_perm:[s,s,s,s]
        auto comp = [g](const f32x4n &v) { return g == 0 ? v.a : g == 1 ? v.b : g == 2 ? v.c : v.d; };
        Z.z[0][0] = comp(s0);
        Z.z[1][0] = comp(s1);
        Z.z[2][0] = comp(s2);
        Z.z[3][0] = comp(s3);
    }
}

__device__ __forceinline__ float readlane_f(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// omega at the start of the 64 steps from step0, one step per lane (item N's
// recurrence, as qm1d_omega_kernel): lane q gets the value for step0 + q in
// om_l; om is the value at step0 on entry and at step0 + 64 on return.
__device__ __forceinline__ void omega_batch(double &om, double &om_l, unsigned long long step0, int lane,
                                            const EnsArgs &A, double sigw, uint32_t k0, uint32_t k1) {
    const int N = A.N;
    const double a = A.a, top = (double)(N - 1) * a;
    const unsigned long long sl = step0 + (unsigned long long)lane;
    const float w = normals4(0ull, kStreamOmega, (uint32_t)sl, (uint32_t)(sl >> 32), k0, k1).a;
    const double d = A.kconst * (sigw * (double)w);
    for (int q = 0; q < 64; ++q) {
        if (lane == q) om_l = om;
        const double nwo = om + readlane_d(d, q);
        if (nwo > top) om = 2 * (double)(N - 1) * a - nwo;
        else if (nwo < 0) om = -nwo;
        else om = nwo;
    }
}

// HELP (one compute wave, potID 3, N <= 128): the field-independent tables of
// the next kHelpS steps -- site normals, x_cl's tanhf at i = -1..N, ddPot --
// are produced into LDS by kHelpWaves helper waves on the CU's other SIMDs
// while wave 0 runs the chain on the previous kHelpS, one block barrier per
// kHelpS steps; the chain's wave then issues only what qm1d_frame_wave does.
// The tables are bounded by 2 x kHelpS steps whatever loops and R are.
constexpr int kHelpS = 8, kHelpWaves = 3, kHelpMaxN = 128;
struct HelpTab {
    float xi[2][kHelpS][kHelpMaxN];
    float t[2][kHelpS][kHelpMaxN + 2];
    double dd[2][kHelpS][kHelpMaxN];
    double om[kHelpWaves][64];  // a helper wave's own copy of its omega batch
    double om_end;              // omega after the frame's last step
    int stop[2];                // by chunk parity: the chain ended (unstable) in this chunk
};

// Helper wave hw of a HELP block: the tables of chunk c (steps c kHelpS ...).
// om / om_l: the wave's omega walk (omega_batch), advanced when a chunk starts
// a 64-step batch; chunks never straddle one (kHelpS divides 64).
__device__ __forceinline__ void help_produce(HelpTab &T, int c, int hw, int lane, double &om, double &om_l,
                                             const EnsArgs &A, unsigned long long tick, double sigw, uint32_t k0,
                                             uint32_t k1) {
    const int N = A.N, nq = (N + 3) >> 2, j0 = c * kHelpS, ns = min(kHelpS, A.loops - j0), b = c & 1;
    const int hid = hw * 64 + lane, nh = kHelpWaves * 64;
    if ((j0 & 63) == 0) {
        omega_batch(om, om_l, tick + (unsigned long long)j0, lane, A, sigw, k0, k1);
        T.om[hw][lane] = om_l;  // read back below by this wave only
    }
    if (j0 + ns == A.loops && hw == 0 && lane == 0)
        T.om_end = (A.loops & 63) ? T.om[0][A.loops & 63] : om;
    for (int idx = hid; idx < ns * nq; idx += nh) {
        const int s = idx / nq, q = idx % nq;
        const unsigned long long st = tick + (unsigned long long)(j0 + s);
        const f32x4n n = normals4((unsigned long long)q, kStreamField, (uint32_t)st, (uint32_t)(st >> 32), k0, k1);
        float *o = &T.xi[b][s][4 * q];  // 4 q + 3 < kHelpMaxN: N <= kHelpMaxN, a multiple of 4
        o[0] = n.a;
        o[1] = n.b;
        o[2] = n.c;
        o[3] = n.d;
    }
    for (int idx = hid; idx < ns * (N + 2); idx += nh) {
        const int s = idx / (N + 2), i = idx % (N + 2) - 1;  // i = -1 .. N
        const float t = xcl_tanh((double)i * A.a, T.om[hw][(j0 + s) & 63]);
        T.t[b][s][i + 1] = t;
        if (i >= 0 && i < N) T.dd[b][s][i] = ddpot(kEta * (double)t, 3);
    }
}

// The step body is qm1d_frame_wave's (sq_qm1d.hip): site updates from the old
// field, running means, guard, X', drift check, then the scan's prefix maxima;
// one wave needs no barrier, W waves use two per step.
template <int K, bool MW, bool P3, bool HELP>
__global__ __launch_bounds__(MW ? 1024 : HELP ? 64 * (1 + kHelpWaves) : 64) void qm1d_ens_frame(const EnsArgs A) {
    static_assert(!HELP || (!MW && P3 && K <= 2), "helper waves: one compute wave, potID 3");
    constexpr int kW = 16;
    __shared__ double s_first[2][kW], s_last[2][kW], s_mx[2][kW], s_ma[2][kW];
    __shared__ int s_arg[2][kW], s_un[2][kW];
    __shared__ double s_fmid[2], s_xe[2];
    __shared__ std::conditional_t<HELP, HelpTab, int> s_help;  // HELP only

    const int N = A.N, mid = N / 2;
    constexpr bool p3 = P3;
    constexpr bool kFastDiv = K >= 4;  // as qm1d_frame_wave
    constexpr int G = 4 / K;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int W = MW ? (int)(blockDim.x >> 6) : 1;
    const int i0 = (int)threadIdx.x * K;
    const size_t base = (size_t)blockIdx.x * (size_t)N;
    EnsRec *const R = A.rec + blockIdx.x;

    // the replica's record and the frame's coefficients (the host's expressions, qm1d_frame)
    const double dtau = R->dtau;
    const unsigned long long tick = R->tick;
    const long long runs_ll = R->runs;
    const int runs = (int)runs_ll;
    const uint32_t k0 = R->k0, k1 = R->k1;
    const double h = dtau;
    // sqrtf is the correctly rounded root, as the host's; __fsqrt_rn is v_sqrt_f32 alone
    // here, an ulp off for some Δτ (0.00465 for one)
    const double sig = A.C * (double)sqrtf((float)(2. * dtau / A.a));
    const double sigw = A.C * (double)sqrtf((float)(2. * dtau));
    const double a = A.a;
    const UDiv da2 = udiv_prep(A.a2);
    const double ninf = -__builtin_inf();
    [[maybe_unused]] const int nchunk = (A.loops + kHelpS - 1) / kHelpS;

    if constexpr (HELP) {
        if (wv > 0) {  // a helper wave: one chunk ahead of the chain, the same barriers as wave 0 below
            HelpTab &T = s_help;
            double om = R->omega, om_l = om;
            help_produce(T, 0, wv - 1, lane, om, om_l, A, tick, sigw, k0, k1);
            __syncthreads();
            for (int c = 0; c < nchunk; ++c) {
                if (c + 1 < nchunk) help_produce(T, c + 1, wv - 1, lane, om, om_l, A, tick, sigw, k0, k1);
                __syncthreads();
                if (T.stop[c & 1]) break;
            }
            return;
        }
    }

    double f[K], x[K], xx0[K], Xn[K], dchk[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int i = i0 + k;
        f[k] = i < N ? A.f[base + i] : 0.;
        x[k] = i < N ? A.x[base + i] : 0.;
        xx0[k] = i < N ? A.xx0[base + i] : 0.;
    }
    int E = R->lrgEl;
    double V = R->lrgVl;
    double om = R->omega;  // omega at the start of the next 64-step batch
    int stable = 1, steps = 0;

    // neighbours and f[mid] of the frame-start field
    double fL = dpp_from_left(f[K - 1], 0.), fR = dpp_from_right(f[0], 0.), fmid;
    if constexpr (MW) {
        if (lane == 0) s_first[1][wv] = f[0];
        if (lane == 63) s_last[1][wv] = f[K - 1];
        if (mid / K == (int)threadIdx.x) s_fmid[1] = pick(f, mid % K);
        __syncthreads();
        if (lane == 0 && wv > 0) fL = s_last[1][wv - 1];
        if (lane == 63 && wv + 1 < W) fR = s_first[1][wv + 1];
        fmid = s_fmid[1];
    } else {
        fmid = readlane_d(pick(f, mid % K), mid / K);
    }

    // lane q of every wave: omega at the start of step j0 + q of the current
    // batch (item N's recurrence, as qm1d_omega_kernel) and, potID 3, the
    // tanhf of x_cl at -a, N a and mid a for it
    double om_l = om;
    float tl_l = 0.f, tr_l = 0.f, tm_l = 0.f;
    SiteNoise<K> Z;

    if constexpr (HELP) __syncthreads();  // chunk 0's tables
    for (int j = 0; j < A.loops; ++j) {
        const int p = j & 1, jq = j & 63;
        float xi[K], ct[K], ctl = 0.f, ctr = 0.f, ctm = 0.f;
        double cdd[K];
        if constexpr (HELP) {
            const HelpTab &T = s_help;
            const int b = (j / kHelpS) & 1, s = j % kHelpS;
            ctl = T.t[b][s][0];
            ctr = T.t[b][s][N + 1];
            ctm = T.t[b][s][mid + 1];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int i = min(i0 + k, N - 1);
                xi[k] = T.xi[b][s][i];
                ct[k] = T.t[b][s][i + 1];
                cdd[k] = T.dd[b][s][i];
            }
        } else {
            if (jq == 0) {
                omega_batch(om, om_l, tick + (unsigned long long)j, lane, A, sigw, k0, k1);
                if (p3) {
                    tl_l = xcl_tanh(-1. * a, om_l);
                    tr_l = xcl_tanh((double)N * a, om_l);
                    tm_l = xcl_tanh((double)mid * a, om_l);
                }
            }
            if ((j & (G - 1)) == 0) site_noise<K>(Z, (int)threadIdx.x, tick + (unsigned long long)j, k0, k1);
            const int zs = j & (G - 1);
            const double omj = readlane_d(om_l, jq);
            if (p3) {
                ctl = readlane_f(tl_l, jq);
                ctr = readlane_f(tr_l, jq);
                ctm = readlane_f(tm_l, jq);
            }
#pragma unroll
            for (int k = 0; k < K; ++k) {
                xi[k] = Z.z[0][k];
#pragma unroll
                for (int s = 1; s < G; ++s)
                    if (s == zs) xi[k] = Z.z[s][k];
                ct[k] = 0.f;
                cdd[k] = 2.;
                if (p3) {
                    ct[k] = xcl_tanh((double)(i0 + k) * a, omj);
                    cdd[k] = ddpot(kEta * (double)ct[k], 3);
                }
            }
        }
        // ---- 1. site updates ----
        const double Xm = fmid + (p3 ? kEta * (double)ctm : 0.);
        const UDiv dden = udiv_prep((double)(runs + j + 1));
        double nA[K], qA[K];
        double nM2[2 * K], qM2[2 * K];  // the running means': xx0's K numerators, then x's
        bool bad = false;
        {
            double prev_old = fL;  // old f[i-1]
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int i = i0 + k;
                const double fi = f[k];
                const double xc = p3 ? kEta * (double)ct[k] : 0.;  // clas(), :184-189
                const double fr = (k + 1 < K) ? f[k + 1] : fR;
                if (i == 0)
                    nA[k] = kM * h * (fr + (-kEta) - (p3 ? kEta * (double)ctl : 0.) - 2 * fi);
                else if (i == N - 1)
                    nA[k] = kM * h * (prev_old + kEta - (p3 ? kEta * (double)ctr : 0.) - 2 * fi);
                else
                    nA[k] = kM * h * (fr + prev_old - 2 * fi);
                // running means from the OLD field, :144-145
                const double Xi = fi + xc;
                nM2[k] = Xi * Xm - xx0[k];
                nM2[K + k] = Xi - x[k];
                if (i < N) bad = bad || !(udiv_range(nA[k]) && udiv_range(nM2[k]) && udiv_range(nM2[K + k]));
                prev_old = fi;
            }
        }
        udiv_step<K, kFastDiv>(nA, da2, qA, bad);
        udiv_step<2 * K, kFastDiv>(nM2, dden, qM2, bad);
        double lmaxX = ninf, lmaxA = ninf;
        int larg = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int i = i0 + k;
            Xn[k] = ninf;
            dchk[k] = 0.;
            if (i < N) {
                const double fi = f[k];
                const double xc = p3 ? kEta * (double)ct[k] : 0.;  // clas(), :184-189
                const double dp = p3 ? cdd[k] : 2.;                // ddPot(), :190-195
                const double dw = sig * (double)xi[k];
                double v = fi + qA[k] - dp * fi * h + dw;
                if (v > 1000) v = 1000;  // guard, :119-133
                if (v < -1000) v = -1000;
                if (v != v) v = 1000;
                dchk[k] = absol(v - fi - dw);
                const double X = v + xc;
                Xn[k] = X;
                if (X > lmaxX) {
                    lmaxX = X;
                    larg = i;
                }
                lmaxA = dpp_vmax_d(lmaxA, absol(X));
                xx0[k] = xx0[k] + qM2[k];
                x[k] = x[k] + qM2[K + k];
                f[k] = v;
            }
        }
        // ---- 2. scan maxima ----
        const double wmx = dpp_all_max(lmaxX), wma = dpp_all_max(lmaxA);
        const unsigned long long hit = __ballot(lmaxX == wmx);
        const int warg = __builtin_amdgcn_readlane(larg, (int)__builtin_ctzll(hit));
        double XE, pX, pA, gX, totA;
        int garg;
        if constexpr (MW) {
            if (lane == 0) {
                s_mx[p][wv] = wmx;
                s_ma[p][wv] = wma;
                s_arg[p][wv] = warg;
                s_first[p][wv] = f[0];
            }
            if (lane == 63) s_last[p][wv] = f[K - 1];
            if (E / K == (int)threadIdx.x) s_xe[p] = pick(Xn, E % K);
            if (mid / K == (int)threadIdx.x) s_fmid[p] = pick(f, mid % K);
            __syncthreads();
            XE = s_xe[p];
            pX = XE;
            pA = V;
            gX = ninf;
            garg = 0;
            totA = V;
            for (int w = 0; w < W; ++w) {
                const double mx = s_mx[p][w], ma = s_ma[p][w];
                if (w < wv) {
                    pX = dpp_vmax_d(pX, mx);
                    pA = dpp_vmax_d(pA, ma);
                }
                totA = dpp_vmax_d(totA, ma);
                if (mx > gX) {
                    gX = mx;
                    garg = s_arg[p][w];
                }
            }
        } else {
            XE = readlane_d(pick(Xn, E % K), E / K);
            pX = XE;
            pA = V;
            gX = wmx;
            garg = warg;
            totA = dpp_vmax_d(V, wma);
        }
        double runX = dpp_vmax_d(pX, dpp_excl_max(lmaxX)), runA = dpp_vmax_d(pA, dpp_excl_max(lmaxA));
        int unst = 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (Xn[k] > runX) {
                runX = Xn[k];
                if (dchk[k] > runA) unst = 1;
            }
            runA = dpp_vmax_d(runA, absol(Xn[k]));
        }
        int any = __ballot(unst) != 0ull;
        // neighbours of the new field for the next step
        fL = dpp_from_left(f[K - 1], 0.);
        fR = dpp_from_right(f[0], 0.);
        if constexpr (MW) {
            if (lane == 0) s_un[p][wv] = any;
            if (lane == 0 && wv > 0) fL = s_last[p][wv - 1];
            if (lane == 63 && wv + 1 < W) fR = s_first[p][wv + 1];
            fmid = s_fmid[p];
            __syncthreads();
            any = 0;
            for (int w = 0; w < W; ++w) any |= s_un[p][w];
        } else {
            fmid = readlane_d(pick(f, mid % K), mid / K);
        }
        if (gX > XE) E = garg;
        V = totA;
        steps = j + 1;
        if (any) stable = 0;
        if constexpr (HELP) {
            if (!stable || j + 1 == A.loops || (j + 1) % kHelpS == 0) {  // the chain's last step in this chunk
                if (lane == 0) s_help.stop[(j / kHelpS) & 1] = !stable;
                __syncthreads();  // the helpers' next chunk is complete; they see stop
            }
        }
        if (!stable) break;
    }

    // ---- adoption and the Δτ controller (qm1d_frame, adapt: tauhost.c:506-541) ----
    if (stable) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int i = i0 + k;
            if (i < N) {
                A.f[base + i] = f[k];
                A.x[base + i] = x[k];
                A.xx0[base + i] = xx0[k];
            }
        }
    }
    // omega after the last step: the start of step `loops`, in the last batch's
    // lane loops % 64, or the batch's carry when the frame ends on a batch
    double om_end;
    if constexpr (HELP) om_end = s_help.om_end;
    else om_end = (A.loops & 63) ? readlane_d(om_l, A.loops & 63) : om;
    if (threadIdx.x == 0) {
        if (stable) {
            R->omega = om_end;
            R->runs = runs_ll + A.loops;
        }
        R->lrgEl = E;
        R->lrgVl = V;
        R->tick = tick + (unsigned long long)A.loops;
        R->steps_total += steps;
        if (A.verdict != nullptr) A.verdict[blockIdx.x] = stable;
        if (A.adapt) {
            int cnt = R->stab_cnt;
            double nd = dtau;
            if (stable) {
                if (cnt > 10) {
                    cnt = 0;
                    nd = nd / 0.950;
                }
                cnt++;
            } else {
                nd = nd * 0.950;
                cnt = 0;
            }
            R->dtau = nd;
            R->stab_cnt = cnt;
        }
    }
}

// Per site i < n: mean and standard error over the replicas of
// c_r = xx0_r[i] - x_r[i] x_r[mid]; one thread per site walks the replicas in
// order, so the sums are the same in every run.
__global__ __launch_bounds__(64) void qm1d_ens_corr(const double *x, const double *xx0, int N, int nrep, int n,
                                                    double *mean, double *err) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n) return;
    const int mid = N / 2;
    double s = 0.;
    for (int r = 0; r < nrep; ++r) {
        const size_t o = (size_t)r * (size_t)N;
        s += xx0[o + i] - x[o + i] * x[o + mid];
    }
    const double m = s / (double)nrep;
    mean[i] = m;
    if (err == nullptr) return;
    double ss = 0.;
    for (int r = 0; r < nrep; ++r) {
        const size_t o = (size_t)r * (size_t)N;
        const double d = (xx0[o + i] - x[o + i] * x[o + mid]) - m;
        ss += d * d;
    }
    err[i] = nrep > 1 ? sqrt(ss / ((double)nrep * (double)(nrep - 1))) : 0.;
}

template <int K, bool P3>
void launch_ens_p(const EnsArgs &a, int W, int nrep, hipStream_t s) {
    if constexpr (P3 && K <= 2) {
        if (W == 1 && a.N <= kHelpMaxN) {  // one compute wave: helper waves take the potential's tables
            hipLaunchKernelGGL((qm1d_ens_frame<K, false, true, true>), dim3(nrep), dim3(64 * (1 + kHelpWaves)), 0, s, a);
            return;
        }
    }
    if (W == 1) hipLaunchKernelGGL((qm1d_ens_frame<K, false, P3, false>), dim3(nrep), dim3(64), 0, s, a);
    else hipLaunchKernelGGL((qm1d_ens_frame<K, true, P3, false>), dim3(nrep), dim3(64 * W), 0, s, a);
}
template <int K>
void launch_ens(const EnsArgs &a, int W, int nrep, hipStream_t s) {
    if (a.pot == 3) launch_ens_p<K, true>(a, W, nrep, s);
    else launch_ens_p<K, false>(a, W, nrep, s);
}

}  // namespace

hipError_t ens_frame_launch(const EnsArgs &a, int nrep, hipStream_t s) {
    int K = 0, W = 0;
    if (nrep < 1 || a.loops < 1 || !qm1d_wave_shape(a.N, K, W)) return hipErrorInvalidValue;
    switch (K) {
    case 1: launch_ens<1>(a, W, nrep, s); break;
    case 2: launch_ens<2>(a, W, nrep, s); break;
    default: launch_ens<4>(a, W, nrep, s); break;
    }
    return hipGetLastError();
}

hipError_t ens_correlator_launch(const double *x, const double *xx0, int N, int nrep, int n, double *mean, double *err,
                                 hipStream_t s) {
    if (n < 1 || n > N || nrep < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(qm1d_ens_corr, dim3((n + 63) / 64), dim3(64), 0, s, x, xx0, N, nrep, n, mean, err);
    return hipGetLastError();
}

}  // namespace sq
