// sq_phi4_ens_flow_frames.hip -- gradient-flow measurements of the phi^4
// lattice ensemble inside its frames kernels (Euler and Heun steps) and inside
// the Heun step kernel.
//
// A flow measurement is the one sq_phi4_ens_flow.hip defines, ens_flow_measure
// of sq_phi4_ens_flow_dev.h: the noise-off update with the replica's flow
// record applied to the on-chip field, the levels reached in one pass, at each
// level the four sums and, with the correlator, one ens_corr measurement into
// the flow accumulators.  The three kernels here are phi4_ens_frames_kernel,
// phi4_ens_heun_frames_kernel and phi4_ens_heun_kernel of sq_phi4_ens.hip, loop
// for loop, with that measurement where theirs stand; this translation unit
// takes every device function from sq_phi4_ens_dev.h and restates none.
//
// Where the un-flowed field waits (Phi4EnsFramesFlowShape's stash).  In the
// frames kernels the measurement follows the frame's verdict, where the
// replica's row of E.field holds exactly the field in the lane's registers: a
// stable frame has just stored it, a rolled-back one has just loaded it.  The
// row is the stash for every K: the flow runs on the registers, and the
// restore is the rollback's own reload, a lane reading the quads it owns.  The
// Heun step kernel has no such row at hand and does as phi4_ens_step_flow_kernel:
// the quads to registers for K < 8, to the row (rewritten at the kernel's end)
// at K = 8.
//
// The simulation is not touched: the flow works on c and the images, which the
// restore rewrites; its clamp hits go to a throw-away maximum; the sums use the
// scratch, the correlator the launch's slice region, W's accumulators and
// E.series are the only device memory written.  The frames' record slots (fk,
// fw) lie behind the scratch and are neither read nor written by it.
#include "sq_phi4_ens_flow_dev.h"
#include "sq_phi4_ens_launch.h"

namespace sq {

namespace {

// phi4_ens_frames_kernel with a flow measurement behind the verdict.  E.series
// non-null: every frame is measured (the sums of every level).  CORR: a stable
// frame also adds one ens_corr measurement per level to W's accumulators.
// With E.series null a rolled-back frame runs no flow step (CORR then).
//
// LDS hazards of the flow block.  It starts behind a block barrier behind which
// cur holds the lane's registers: the last step's after a stable frame, the
// reload's after a rollback; no wave reads an image between that barrier and
// the block.  ens_flow_measure's steps carry the step loop's barriers for the
// launch's image count, and its measurement at the last level ends in a block
// barrier behind its last image read (ens_fold's; ens_corr's, which follows it
// when both are taken): that barrier separates the last image read from the
// restore's write of cur.  The restore's own barrier separates it from the next
// frame's first step, whose neighbour reads are the next image reads.  The
// scratch and the slice region are free again after any block barrier.
template <int K, typename... CA>
__global__ __launch_bounds__(kPhi4EnsMaxLanes) void phi4_ens_frames_flow_kernel(const Phi4EnsArgs E,
                                                                                 const Phi4EnsFrameArgs F,
                                                                                 const Phi4EnsFlowArgs W,
                                                                                 const int two, const CA... ca) {
    constexpr bool CORR = sizeof...(CA) != 0;
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
        // the flow block: the replica's row of E.field holds the registers' field (stored or loaded just above)
        const bool docorr = CORR && stable;  // block-uniform: every lane decided the frame from the same records
        if (__builtin_expect(E.series != nullptr || docorr, 0)) {
            double *ser = E.series == nullptr
                              ? nullptr
                              : E.series + 4 * ((size_t)f * (size_t)W.nlev * gridDim.x + (size_t)r);
            ens_flow_measure<K, CORR>(E, W, g, r, c, fl, cur, oth, two, scr,
                                      reinterpret_cast<double *>(sb + kPhi4EnsFrameScratchBytes), ser, docorr);
            // the registers and the image cur back from the row (no wave reads an image here: see above)
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

// phi4_ens_heun_frames_kernel with the same flow block behind the verdict.  cur
// is img0 for the whole call; the flow's ping-pong (TWO) may end in the other
// image after an odd level, so the restore writes img0 explicitly.
//
// LDS hazards of the flow block.  As in phi4_ens_frames_flow_kernel it starts
// behind a block barrier behind which img0 holds the lane's registers and no
// wave reads an image (the step's last barrier, or the reload's).  The flow
// steps are Euler updates: they read one image and write the other (TWO), or
// read, barrier, write the one image, each step ending in a barrier.  The
// measurement at the last level ends in a block barrier behind its last image
// read (ens_fold's or ens_corr's): it separates that read from the restore's
// write of img0.  The restore's own barrier separates it from stage 1 of the
// next step, the next reader of img0; stage 1 writes img1 (TWO), which nobody
// reads before stage 2's barrier, so what the flow left there does not matter.
template <int K, bool TWO, typename... CA>
__global__ __launch_bounds__(kPhi4EnsMaxLanes) void phi4_ens_heun_frames_flow_kernel(const Phi4EnsArgs E,
                                                                                      const Phi4EnsFrameArgs F,
                                                                                      const Phi4EnsFlowArgs W,
                                                                                      const CA... ca) {
    constexpr bool CORR = sizeof...(CA) != 0;
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
                        cur4[q] = c[j];  // no wave reads cur here (see phi4_ens_heun_frames_kernel)
                    }
                }
            }
            if (!stable) __syncthreads();  // block-uniform: every lane decided the frame from the same records
        }
        if (tid == 0) {
            F.stable[(size_t)f * gridDim.x + (size_t)r] = stable;
            F.dtau[(size_t)f * gridDim.x + (size_t)r] = dtau;
        }
        // the flow block: the replica's row of E.field holds the registers' field (stored or loaded just above)
        const bool docorr = CORR && stable;  // block-uniform
        if (__builtin_expect(E.series != nullptr || docorr, 0)) {
            double *ser = E.series == nullptr
                              ? nullptr
                              : E.series + 4 * ((size_t)f * (size_t)W.nlev * gridDim.x + (size_t)r);
            ens_flow_measure<K, CORR>(E, W, g, r, c, fl, cur, oth, TWO ? 1 : 0, reinterpret_cast<double *>(sb),
                                      reinterpret_cast<double *>(sb + kPhi4EnsFrameScratchBytes), ser, docorr, tid);
            // the registers and img0 back from the row (no wave reads an image here: see above)
            float4 *gf = reinterpret_cast<float4 *>(E.field + (size_t)r * (size_t)(4 * g.Q));
            float4 *cur4 = reinterpret_cast<float4 *>(cur);
            const int T = blockDim.x;
#pragma unroll
            for (int j = 0; j < K; ++j) {
                int q = (int)tid + j * T;
                asm volatile("" : "+v"(q));
                if (fl.get(j) & kEnsValid) {
                    c[j] = gf[q];
                    cur4[q] = c[j];
                }
            }
            __syncthreads();
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

// phi4_ens_heun_kernel with a flow measurement after each every-th Heun step,
// the stash as in phi4_ens_step_flow_kernel: registers for K < 8, the replica's
// row of E.field at K = 8 (rewritten at the kernel's end; a lane reloads
// exactly the quads it stored).  CA empty: the plain launch's layout, the sums
// only (E.series non-null).  CA = {Phi4EnsCorrArgs} (its fields unused): the
// correlator launch's layout, one ens_corr measurement per level, the sums when
// E.series is given.
//
// LDS hazards of the flow block.  It starts behind ens_heun's last barrier, cur
// (img0 for the whole call) holding phi', the lane's registers.  The flow steps
// carry their own barriers; the measurement at the last level ends in a block
// barrier behind its last image read (ens_fold's or ens_corr's), which separates
// that read from the restore's write of img0; the restore's own barrier
// separates it from stage 1 of the next Heun step, the next reader of img0.
template <int K, typename... CA>
__global__ __launch_bounds__(kPhi4EnsMaxLanes) void phi4_ens_heun_flow_kernel(const Phi4EnsArgs E,
                                                                               const Phi4EnsFlowArgs W, const int two,
                                                                               const CA... ca) {
    constexpr bool CORR = sizeof...(CA) != 0;
    constexpr bool REG = K < 8;  // where the quads wait: Phi4EnsFramesFlowShape's hs_stash
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
        // unlikely: as in phi4_ens_step_flow_kernel, the hint keeps the flow's loops from costing the step
        if (__builtin_expect(--left == 0, 0)) {
            left = E.every;
            float4 *gf = reinterpret_cast<float4 *>(E.field + (size_t)r * (size_t)(4 * g.Q));
            float4 *cur4 = reinterpret_cast<float4 *>(cur);
            uint32_t fu[K];
#pragma unroll
            for (int j = 0; j < K; ++j) fu[j] = fl.get(j);
            // the quads aside
            float4 keep[REG ? K : 1];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if constexpr (REG) {
                    keep[j] = c[j];
                } else {
                    int q = (int)threadIdx.x + j * T;
                    asm volatile("" : "+v"(q));  // opaque: the address is formed here, not kept for the call
                    if (fu[j] & kEnsValid) gf[q] = c[j];
                }
            }
            double *ser = E.series == nullptr
                              ? nullptr
                              : E.series + 4 * ((size_t)rec * (size_t)W.nlev * gridDim.x + (size_t)r);
            ens_flow_measure<K, CORR>(E, W, g, r, c, fu, cur, oth, two, scr, scr + kPhi4EnsScratchBytes / 8, ser,
                                      true);
            ++rec;
            // the quads and img0 back (no wave reads an image here: see above)
#pragma unroll
            for (int j = 0; j < K; ++j) {
                int q = (int)threadIdx.x + j * T;
                asm volatile("" : "+v"(q));
                if (fu[j] & kEnsValid) {
                    if constexpr (REG) c[j] = keep[j];
                    else c[j] = gf[q];
                    cur4[q] = c[j];
                }
            }
            __syncthreads();
        }
    }
    float4 *gf = reinterpret_cast<float4 *>(E.field + (size_t)r * (size_t)(4 * g.Q));
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (fl.get(j) & kEnsValid) gf[(int)threadIdx.x + j * T] = c[j];
    // a stage's guarded maximum or the final guard reached the clamp
    if (am >= E.clampv) E.flags[r] = 1;
}

}  // namespace

Phi4EnsFramesFlowShape phi4_ens_frames_flow_shape(int sites, int Lz) {
    Phi4EnsFramesFlowShape f{phi4_ens_shape(sites, Lz), 0, 0, 0, 0};
    f.fr_stash = 1;   // the frames kernels: the row, for every K
    f.hfr_stash = 1;
    f.hs_stash = f.K < 8 ? 0 : 1;  // phi4_ens_heun_flow_kernel's REG
    f.mask = 0xf;  // every instance fits its registers (profiles/r07/phi4_ens_flow_frames/resources.txt)
    return f;
}

hipError_t phi4_ens_frames_flow_launch(const Phi4EnsArgs &a, const Phi4EnsFrameArgs &f, const Phi4EnsFlowArgs &w,
                                       bool corr, bool heun, int nrep, hipStream_t s) {
    if (!ens_frames_ok(a, f, nrep) || !ens_flow_ok(a, w, corr)) return hipErrorInvalidValue;
    const Phi4EnsFramesFlowShape sh = phi4_ens_frames_flow_shape(a.Lx * a.Ly * a.Lz, a.Lz);
    if (!(sh.mask >> (2 * (heun ? 1 : 0) + (corr ? 1 : 0)) & 1)) return hipErrorInvalidValue;
    const Phi4EnsLds l = sh.lds(kPhi4EnsLdsFrames, corr ? phi4_ens_corr_bytes(a.Lz) : 0);
    Phi4EnsArgs q = a;
    Phi4EnsFrameArgs fq = f;
    Phi4EnsFlowArgs wq = w;
    Phi4EnsCorrArgs cq{};
    int two = l.images == 2;
    if (heun) {  // the image count selects the instance
        void *args[] = {&q, &fq, &wq, &cq};  // the plain instances take the first three
        const void *fn = corr ? (two ? SQ_ENS_KERNEL(sh.K, phi4_ens_heun_frames_flow_kernel, true, Phi4EnsCorrArgs)
                                     : SQ_ENS_KERNEL(sh.K, phi4_ens_heun_frames_flow_kernel, false, Phi4EnsCorrArgs))
                              : (two ? SQ_ENS_KERNEL(sh.K, phi4_ens_heun_frames_flow_kernel, true)
                                     : SQ_ENS_KERNEL(sh.K, phi4_ens_heun_frames_flow_kernel, false));
        return ens_launch(fn, nrep, sh.T, l.bytes, args, s);
    }
    void *args[] = {&q, &fq, &wq, &two, &cq};  // the plain instances take the first four
    const void *fn = corr ? SQ_ENS_KERNEL(sh.K, phi4_ens_frames_flow_kernel, Phi4EnsCorrArgs)
                          : SQ_ENS_KERNEL(sh.K, phi4_ens_frames_flow_kernel);
    return ens_launch(fn, nrep, sh.T, l.bytes, args, s);
}

hipError_t phi4_ens_heun_flow_launch(const Phi4EnsArgs &a, const Phi4EnsFlowArgs &w, bool corr, int nrep,
                                     hipStream_t s) {
    if (!ens_step_ok(a, nrep, true) || !ens_flow_ok(a, w, corr)) return hipErrorInvalidValue;
    const Phi4EnsFramesFlowShape sh = phi4_ens_frames_flow_shape(a.Lx * a.Ly * a.Lz, a.Lz);
    const Phi4EnsLds l = sh.lds(kPhi4EnsLdsStep, corr ? phi4_ens_corr_bytes(a.Lz) : 0);
    Phi4EnsArgs q = a;
    Phi4EnsFlowArgs wq = w;
    Phi4EnsCorrArgs cq{};
    int two = l.images == 2;
    void *args[] = {&q, &wq, &two, &cq};  // the plain instances take the first three
    const void *fn = corr ? SQ_ENS_KERNEL(sh.K, phi4_ens_heun_flow_kernel, Phi4EnsCorrArgs)
                          : SQ_ENS_KERNEL(sh.K, phi4_ens_heun_flow_kernel);
    return ens_launch(fn, nrep, sh.T, l.bytes, args, s);
}

}  // namespace sq
