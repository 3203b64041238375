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
// The step itself (ens_step) and every other device function the ensemble's
// translation units share are sq_phi4_ens_dev.h; this file holds the kernels
// of the plain, correlator, momentum and Heun launches and their launchers
// (sq_phi4_ens_launch.h: the one launch path).  With two images (they fit up
// to 20,000-odd sites) a step reads one and writes the other, one barrier per
// step; with one image every wave must have finished reading before any
// writes: two barriers per step.  A replica whose sig is 0 takes the noise-off
// instance of the update, as a context with C = 0 does.  No work-group ever
// waits for another one.
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
#include "sq_phi4_ens_dev.h"
#include "sq_phi4_ens_launch.h"

namespace sq {

namespace {

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
    const Phi4StepArgs A = ens_step_args(rc, E.clampv);
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
    const Phi4StepArgs A = ens_step_args(rc, E.clampv);
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
    Phi4StepArgs A = ens_step_args(rc, E.clampv);
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
    Phi4StepArgs A = ens_step_args(rc, E.clampv);
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

}  // namespace

Phi4EnsShape phi4_ens_shape(int sites, int Lz) {
    Phi4EnsShape s;
    const int Q = sites / 4;
    s.K = Q <= kPhi4EnsMaxLanes ? 1 : (Q <= 2 * kPhi4EnsMaxLanes ? 2 : (Q <= 4 * kPhi4EnsMaxLanes ? 4 : 8));
    s.T = (((Q + s.K - 1) / s.K) + 63) / 64 * 64;
    s.sites = sites;
    // momenta: legal when one image fits in each of the three launches that take them
    const int pl = phi4_ens_pcorr_bytes(Lz);
    s.pc_ok = Lz > 0 && s.lds(kPhi4EnsLdsStep, pl).bytes <= kPhi4EnsLdsBytes &&
              s.lds(kPhi4EnsLdsFrames, pl).bytes <= kPhi4EnsLdsBytes &&
              s.lds(kPhi4EnsLdsStored, pl).bytes <= kPhi4EnsLdsBytes;
    return s;
}

hipError_t phi4_ens_step_pcorr_launch(const Phi4EnsArgs &a, const Phi4EnsPCorrArgs &p, int nrep, hipStream_t s) {
    if (!ens_step_ok(a, nrep, true) || !ens_pcorr_ok(p, true)) return hipErrorInvalidValue;
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz, a.Lz);
    if (!sh.pc_ok) return hipErrorInvalidValue;
    const Phi4EnsLds l = sh.lds(kPhi4EnsLdsStep, phi4_ens_pcorr_bytes(a.Lz));
    Phi4EnsArgs q = a;
    Phi4EnsPCorrArgs pq = p;
    int two = l.images == 2;
    void *args[] = {&q, &two, &pq};
    return ens_launch(SQ_ENS_KERNEL(sh.K, phi4_ens_step_kernel, Phi4EnsPCorrArgs), nrep, sh.T, l.bytes, args, s);
}

hipError_t phi4_ens_frames_pcorr_launch(const Phi4EnsArgs &a, const Phi4EnsFrameArgs &f, const Phi4EnsPCorrArgs &p,
                                        int nrep, hipStream_t s) {
    if (!ens_frames_ok(a, f, nrep) || !ens_pcorr_ok(p, true)) return hipErrorInvalidValue;
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz, a.Lz);
    if (!sh.pc_ok) return hipErrorInvalidValue;
    const Phi4EnsLds l = sh.lds(kPhi4EnsLdsFrames, phi4_ens_pcorr_bytes(a.Lz));
    int two = l.images == 2;
    Phi4EnsArgs q = a;
    Phi4EnsFrameArgs fq = f;
    Phi4EnsPCorrArgs pq = p;
    void *args[] = {&q, &fq, &two, &pq};
    return ens_launch(SQ_ENS_KERNEL(sh.K, phi4_ens_frames_kernel, Phi4EnsPCorrArgs), nrep, sh.T, l.bytes, args, s);
}

hipError_t phi4_ens_pslices_launch(const Phi4EnsArgs &a, const Phi4EnsPCorrArgs &p, int first, int count, double *AB,
                                   double *g, hipStream_t s) {
    if (!ens_stored_ok(a, first, count) || AB == nullptr || g == nullptr || !ens_pcorr_ok(p, false))
        return hipErrorInvalidValue;
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz, a.Lz);
    if (!sh.pc_ok) return hipErrorInvalidValue;
    const Phi4EnsLds l = sh.lds(kPhi4EnsLdsStored, phi4_ens_pcorr_bytes(a.Lz));
    Phi4EnsArgs q = a;
    Phi4EnsPCorrArgs pq = p;
    void *args[] = {&q, &pq, &first, &AB, &g};
    return ens_launch(SQ_ENS_KERNEL(sh.K, phi4_ens_pslices_kernel), count, sh.T, l.bytes, args, s);
}

hipError_t phi4_ens_step_launch(const Phi4EnsArgs &a, int nrep, hipStream_t s) {
    if (!ens_step_ok(a, nrep, false)) return hipErrorInvalidValue;
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz);
    const Phi4EnsLds l = sh.lds(kPhi4EnsLdsStep);
    Phi4EnsArgs q = a;
    int two = l.images == 2;
    void *args[] = {&q, &two};
    return ens_launch(SQ_ENS_KERNEL(sh.K, phi4_ens_step_kernel), nrep, sh.T, l.bytes, args, s);
}

hipError_t phi4_ens_step_corr_launch(const Phi4EnsArgs &a, const Phi4EnsCorrArgs &c, int nrep, hipStream_t s) {
    if (!ens_step_ok(a, nrep, true) || !ens_corr_ok(c)) return hipErrorInvalidValue;
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz, a.Lz);
    const Phi4EnsLds l = sh.lds(kPhi4EnsLdsStep, phi4_ens_corr_bytes(a.Lz));
    Phi4EnsArgs q = a;
    Phi4EnsCorrArgs cq = c;
    int two = l.images == 2;
    void *args[] = {&q, &two, &cq};
    return ens_launch(SQ_ENS_KERNEL(sh.K, phi4_ens_step_kernel, Phi4EnsCorrArgs), nrep, sh.T, l.bytes, args, s);
}

namespace {
// What a launch with at most one of the two measurements keeps behind its scratch.
int ens_meas_bytes(const Phi4EnsCorrArgs *c, const Phi4EnsPCorrArgs *p, int Lz) {
    return p ? phi4_ens_pcorr_bytes(Lz) : c ? phi4_ens_corr_bytes(Lz) : 0;
}
}  // namespace

hipError_t phi4_ens_heun_launch(const Phi4EnsArgs &a, const Phi4EnsCorrArgs *c, const Phi4EnsPCorrArgs *p, int nrep,
                                hipStream_t s) {
    const bool meas = c != nullptr || p != nullptr;
    if (!ens_step_ok(a, nrep, meas) || (c != nullptr && p != nullptr)) return hipErrorInvalidValue;
    if (c != nullptr && !ens_corr_ok(*c)) return hipErrorInvalidValue;
    if (p != nullptr && !ens_pcorr_ok(*p, true)) return hipErrorInvalidValue;
    // the step launches' layouts, each by its own rule
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz, meas ? a.Lz : 0);
    if (p != nullptr && !sh.pc_ok) return hipErrorInvalidValue;
    const Phi4EnsLds l = sh.lds(kPhi4EnsLdsStep, ens_meas_bytes(c, p, a.Lz));
    int two = l.images == 2;
    Phi4EnsArgs q = a;
    Phi4EnsCorrArgs cq = c ? *c : Phi4EnsCorrArgs{};
    Phi4EnsPCorrArgs pq = p ? *p : Phi4EnsPCorrArgs{};
    void *args[] = {&q, &two, p ? (void *)&pq : (void *)&cq};  // the plain instances take the first two
    const void *fn = p   ? SQ_ENS_KERNEL(sh.K, phi4_ens_heun_kernel, Phi4EnsPCorrArgs)
                     : c ? SQ_ENS_KERNEL(sh.K, phi4_ens_heun_kernel, Phi4EnsCorrArgs)
                         : SQ_ENS_KERNEL(sh.K, phi4_ens_heun_kernel);
    return ens_launch(fn, nrep, sh.T, l.bytes, args, s);
}

hipError_t phi4_ens_heun_frames_launch(const Phi4EnsArgs &a, const Phi4EnsFrameArgs &f, const Phi4EnsCorrArgs *c,
                                       const Phi4EnsPCorrArgs *p, int nrep, hipStream_t s) {
    if (!ens_frames_ok(a, f, nrep) || (c != nullptr && p != nullptr)) return hipErrorInvalidValue;
    if (c != nullptr && !ens_corr_ok(*c)) return hipErrorInvalidValue;
    if (p != nullptr && !ens_pcorr_ok(*p, true)) return hipErrorInvalidValue;
    // the frames launches' layouts, each by its own rule
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz, (c || p) ? a.Lz : 0);
    if (p != nullptr && !sh.pc_ok) return hipErrorInvalidValue;
    const Phi4EnsLds l = sh.lds(kPhi4EnsLdsFrames, ens_meas_bytes(c, p, a.Lz));
    const bool two = l.images == 2;  // selects the instance
    Phi4EnsArgs q = a;
    Phi4EnsFrameArgs fq = f;
    Phi4EnsCorrArgs cq = c ? *c : Phi4EnsCorrArgs{};
    Phi4EnsPCorrArgs pq = p ? *p : Phi4EnsPCorrArgs{};
    void *args[] = {&q, &fq, p ? (void *)&pq : (void *)&cq};  // the plain instances take the first two
    const void *fn = p   ? (two ? SQ_ENS_KERNEL(sh.K, phi4_ens_heun_frames_kernel, true, Phi4EnsPCorrArgs)
                                : SQ_ENS_KERNEL(sh.K, phi4_ens_heun_frames_kernel, false, Phi4EnsPCorrArgs))
                     : c ? (two ? SQ_ENS_KERNEL(sh.K, phi4_ens_heun_frames_kernel, true, Phi4EnsCorrArgs)
                                : SQ_ENS_KERNEL(sh.K, phi4_ens_heun_frames_kernel, false, Phi4EnsCorrArgs))
                         : (two ? SQ_ENS_KERNEL(sh.K, phi4_ens_heun_frames_kernel, true)
                                : SQ_ENS_KERNEL(sh.K, phi4_ens_heun_frames_kernel, false));
    return ens_launch(fn, nrep, sh.T, l.bytes, args, s);
}

hipError_t phi4_ens_frames_launch(const Phi4EnsArgs &a, const Phi4EnsFrameArgs &f, int nrep, hipStream_t s) {
    if (!ens_frames_ok(a, f, nrep)) return hipErrorInvalidValue;
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz);
    const Phi4EnsLds l = sh.lds(kPhi4EnsLdsFrames);
    int two = l.images == 2;
    Phi4EnsArgs q = a;
    Phi4EnsFrameArgs fq = f;
    void *args[] = {&q, &fq, &two};
    return ens_launch(SQ_ENS_KERNEL(sh.K, phi4_ens_frames_kernel), nrep, sh.T, l.bytes, args, s);
}

hipError_t phi4_ens_frames_corr_launch(const Phi4EnsArgs &a, const Phi4EnsFrameArgs &f, const Phi4EnsCorrArgs &c,
                                       int nrep, hipStream_t s) {
    if (!ens_frames_ok(a, f, nrep) || !ens_corr_ok(c)) return hipErrorInvalidValue;
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz, a.Lz);
    const Phi4EnsLds l = sh.lds(kPhi4EnsLdsFrames, phi4_ens_corr_bytes(a.Lz));
    int two = l.images == 2;
    Phi4EnsArgs q = a;
    Phi4EnsFrameArgs fq = f;
    Phi4EnsCorrArgs cq = c;
    void *args[] = {&q, &fq, &two, &cq};
    return ens_launch(SQ_ENS_KERNEL(sh.K, phi4_ens_frames_kernel, Phi4EnsCorrArgs), nrep, sh.T, l.bytes, args, s);
}

hipError_t phi4_ens_slices_launch(const Phi4EnsArgs &a, int first, int count, double *S, double *g, hipStream_t s) {
    if (!ens_stored_ok(a, first, count) || S == nullptr || g == nullptr) return hipErrorInvalidValue;
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz, a.Lz);
    const Phi4EnsLds l = sh.lds(kPhi4EnsLdsStored, phi4_ens_corr_bytes(a.Lz));
    Phi4EnsArgs q = a;
    void *args[] = {&q, &first, &S, &g};
    return ens_launch(SQ_ENS_KERNEL(sh.K, phi4_ens_slices_kernel), count, sh.T, l.bytes, args, s);
}

hipError_t phi4_ens_moments_launch(const Phi4EnsArgs &a, int first, int count, double *out, hipStream_t s) {
    if (!ens_stored_ok(a, first, count) || out == nullptr) return hipErrorInvalidValue;
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz);
    const Phi4EnsLds l = sh.lds(kPhi4EnsLdsStored);
    Phi4EnsArgs q = a;
    void *args[] = {&q, &first, &out};
    return ens_launch(SQ_ENS_KERNEL(sh.K, phi4_ens_moments_kernel), count, sh.T, l.bytes, args, s);
}

hipError_t phi4_ens_init_launch(const Phi4EnsArgs &a, int nrep, float amp, hipStream_t s) {
    if (!ens_shape_ok(a) || nrep < 1) return hipErrorInvalidValue;
    const int nq = a.Lx * a.Ly * a.Lz / 4;
    Phi4EnsArgs q = a;
    void *args[] = {&q, &amp};
    // not ens_launch: a two-dimensional grid, grid.y <= 65535, so larger ensembles go in slices of replicas
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

