// sq_phi4_ens_flow.hip -- gradient-flow measurements of the phi^4 lattice
// ensemble, in the resident kernel.
//
// The flow of a replica is the noise-off step of sq_phi4_ens.hip, ens_step<K,
// false>, applied to a copy of its field with the replica's flow coefficients
// (Phi4EnsFlowRec: the flow step as h, the flow's m² and λ, sig = 0): bit for
// bit what a C = 0 ensemble gives after upload and step.  The measurements at a
// level are the ensemble's too: ens_sums + ens_fold, ens_corr.  This translation
// unit takes those device functions from sq_phi4_ens_dev.h and restates none.
//
// phi4_ens_step_flow_kernel is phi4_ens_step_kernel's loop.  At a measurement
// point -- behind the step's last barrier, cur holding the field the lane's
// registers hold -- it
//   1. puts the lane's K quads aside (registers, or the replica's row of
//      E.field at K = 8: the row is rewritten at the kernel's end, and a lane
//      reloads exactly the quads it stored, no other lane's);
//   2. flows: ens_step<K, false>, a throw-away running maximum, the image
//      ping-pong and the barriers of the step loop for the launch's image count;
//   3. measures at each level on the way, level 0 before the first flow step;
//   4. restores the registers and the image cur, one barrier behind it.
// LDS hazards of the restore.  Every measurement ends in a block barrier behind
// its last image read (ens_fold's, ens_corr's), and a measurement point takes
// at least one at the last level, so no wave reads an image when the restore
// writes cur; the restore's own barrier puts cur in front of the next step's
// neighbour reads.  The scratch and the slice region lie behind the images and
// are free again after any block barrier: every flow step has one, and the
// levels ascend strictly.
//
// phi4_ens_flowed_kernel and phi4_ens_flow_field_kernel load the stored field,
// flow, and measure per level / store to a buffer of their own; they never
// write E.field.
//
// The same measurement inside the frames kernels and the Heun step kernel is
// sq_phi4_ens_flow_frames.hip; what the two files share (ens_flow_args,
// ens_flow_step, ens_flow_measure) is sq_phi4_ens_flow_dev.h.
#include "sq_phi4_ens_flow_dev.h"  // ens_flow_args, ens_flow_step, ens_flow_measure
#include "sq_phi4_ens_launch.h"

namespace sq {

namespace {

// two != 0: two LDS images.  CA empty: the plain launch's layout, the sums only (E.series non-null).  CA =
// {Phi4EnsCorrArgs} (its fields unused: the accumulators are the flow's): the correlator launch's layout, one
// ens_corr measurement per level, the sums when E.series is given.
template <int K, typename... CA>
__global__ __launch_bounds__(kPhi4EnsMaxLanes) void phi4_ens_step_flow_kernel(const Phi4EnsArgs E,
                                                                               const Phi4EnsFlowArgs W, const int two,
                                                                               const CA... ca) {
    constexpr bool CORR = sizeof...(CA) != 0;
    constexpr bool REG = K < 8;  // where the quads wait: phi4_ens_flow_shape's `stash`
    const int r = blockIdx.x;
    const EnsGeo g = ens_geo(E);
    const Phi4EnsRec rc = E.rec[r];
    const Phi4StepArgs A = ens_step_args(rc, E.clampv);
    const bool nz = rc.sig != 0.0f;
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
        // unlikely: the flow's loops nest deeper than the step, and without the hint the register allocator
        // spends its scalar spills on the step (measured: every step of the call 13-18 % slower than
        // phi4_ens_step_kernel's, whatever the number of measurements; with it, the same)
        if (__builtin_expect(--left == 0, 0)) {
            left = E.every;
            float4 *gf = reinterpret_cast<float4 *>(E.field + (size_t)r * (size_t)(4 * g.Q));
            const int nt = E.Lz / 2 + 1;
            // 1. the quads aside
            float4 keep[REG ? K : 1];
#pragma unroll
            for (int j = 0; j < K; ++j) {
                if constexpr (REG) {
                    keep[j] = c[j];
                } else {
                    int q = (int)threadIdx.x + j * T;
                    asm volatile("" : "+v"(q));  // opaque: the address is formed here, not kept for the call
                    if (fl[j] & kEnsValid) gf[q] = c[j];
                }
            }
            // 2., 3. the flow, measuring on the way
            const Phi4StepArgs FA = ens_flow_args(W.rec[r], E.clampv);
            const int nlev = W.nlev;
            float *fc = cur, *fo = oth;
            int done = 0;
            for (int l = 0; l < nlev; ++l) {
                const int n = W.lev[l];
                for (; done < n; ++done) ens_flow_step<K>(FA, g, c, fl, fc, fo, two);
                if (!CORR || E.series != nullptr) {
                    double sm[4];
                    float mx;
                    ens_sums<K>(g, c, fl, fc, sm, mx);
                    ens_fold(sm, mx, scr,
                             E.series + 4 * (((size_t)rec * (size_t)nlev + (size_t)l) * gridDim.x + (size_t)r), false);
                }
                if constexpr (CORR) {
                    const size_t a = (size_t)r * (size_t)nlev + (size_t)l;
                    ens_corr<true>(g, E.Lz, fc, scr + kPhi4EnsScratchBytes / 8, W.G + a * (size_t)nt, W.S1 + a,
                                   W.nmeas + a, nullptr);
                }
            }
            ++rec;
            // 4. the quads and the image back (no wave reads an image here: see the head of the file)
#pragma unroll
            for (int j = 0; j < K; ++j) {
                int q = (int)threadIdx.x + j * T;
                asm volatile("" : "+v"(q));
                if (fl[j] & kEnsValid) {
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
        if (fl[j] & kEnsValid) gf[(int)threadIdx.x + j * T] = c[j];
    // some site was clamped (NaN -> +clamp) iff the running max after the guard reached the clamp
    if (am >= E.clampv) E.flags[r] = 1;
}

// One measurement per level of the stored field of replica first + blockIdx.x, flowed on-chip: the correlator
// launch's layout.  sums[b][l][4], S[b][l][Lz], gout[b][l][nt], b = blockIdx.x.
template <int K>
__global__ __launch_bounds__(kPhi4EnsMaxLanes) void phi4_ens_flowed_kernel(const Phi4EnsArgs E,
                                                                            const Phi4EnsFlowArgs W, const int two,
                                                                            const int first, double *sums, double *S,
                                                                            double *gout) {
    const int r = first + blockIdx.x;
    const EnsGeo g = ens_geo(E);
    float *fc = reinterpret_cast<float *>(ens_smem);
    float *fo = two ? fc + 4 * g.Q : fc;
    double *scr = reinterpret_cast<double *>(ens_smem + (size_t)(two ? 2 : 1) * 16 * (size_t)g.Q);
    float4 c[K];
    uint32_t fl[K];
    ens_load<K>(E, g, r, c, fl, fc);  // ends in a barrier
    const Phi4StepArgs FA = ens_flow_args(W.rec[r], E.clampv);
    const int nt = E.Lz / 2 + 1;
    int done = 0;
    for (int l = 0; l < W.nlev; ++l) {
        const int n = W.lev[l];
        for (; done < n; ++done) ens_flow_step<K>(FA, g, c, fl, fc, fo, two);
        const size_t a = (size_t)blockIdx.x * (size_t)W.nlev + (size_t)l;
        double sm[4];
        float mx;
        ens_sums<K>(g, c, fl, fc, sm, mx);
        ens_fold(sm, mx, scr, sums + 4 * a, false);
        ens_corr<false>(g, E.Lz, fc, scr + kPhi4EnsScratchBytes / 8, gout + a * (size_t)nt, nullptr, nullptr,
                        S + a * (size_t)E.Lz);
    }
}

// The stored field of replica first + blockIdx.x after nsteps flow steps to out[blockIdx.x][sites]: the plain
// launch's layout.
template <int K>
__global__ __launch_bounds__(kPhi4EnsMaxLanes) void phi4_ens_flow_field_kernel(const Phi4EnsArgs E,
                                                                                const Phi4EnsFlowArgs W,
                                                                                const int two, const int first,
                                                                                const int nsteps, float *out) {
    const int r = first + blockIdx.x;
    const EnsGeo g = ens_geo(E);
    float *fc = reinterpret_cast<float *>(ens_smem);
    float *fo = two ? fc + 4 * g.Q : fc;
    float4 c[K];
    uint32_t fl[K];
    ens_load<K>(E, g, r, c, fl, fc);  // ends in a barrier
    const Phi4StepArgs FA = ens_flow_args(W.rec[r], E.clampv);
    for (int t = 0; t < nsteps; ++t) ens_flow_step<K>(FA, g, c, fl, fc, fo, two);
    float4 *of = reinterpret_cast<float4 *>(out + (size_t)blockIdx.x * (size_t)(4 * g.Q));
    const int T = blockDim.x;
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (fl[j] & kEnsValid) of[(int)threadIdx.x + j * T] = c[j];
}

}  // namespace

Phi4EnsFlowShape phi4_ens_flow_shape(int sites, int Lz) {
    Phi4EnsFlowShape f{phi4_ens_shape(sites, Lz), 0};
    f.stash = f.K < 8 ? 0 : 1;  // phi4_ens_step_flow_kernel's REG
    return f;
}

hipError_t phi4_ens_step_flow_launch(const Phi4EnsArgs &a, const Phi4EnsFlowArgs &w, bool corr, int nrep,
                                     hipStream_t s) {
    if (!ens_step_ok(a, nrep, true) || !ens_flow_ok(a, w, corr)) return hipErrorInvalidValue;
    const Phi4EnsFlowShape sh = phi4_ens_flow_shape(a.Lx * a.Ly * a.Lz, a.Lz);
    const Phi4EnsLds l = sh.lds(kPhi4EnsLdsStep, corr ? phi4_ens_corr_bytes(a.Lz) : 0);
    Phi4EnsArgs q = a;
    Phi4EnsFlowArgs wq = w;
    Phi4EnsCorrArgs cq{};
    int two = l.images == 2;
    void *args[] = {&q, &wq, &two, &cq};  // the plain instances take the first three
    const void *fn = corr ? SQ_ENS_KERNEL(sh.K, phi4_ens_step_flow_kernel, Phi4EnsCorrArgs)
                          : SQ_ENS_KERNEL(sh.K, phi4_ens_step_flow_kernel);
    return ens_launch(fn, nrep, sh.T, l.bytes, args, s);
}

hipError_t phi4_ens_flowed_launch(const Phi4EnsArgs &a, const Phi4EnsFlowArgs &w, int first, int count, double *sums,
                                  double *S, double *g, hipStream_t s) {
    if (!ens_stored_ok(a, first, count) || sums == nullptr || S == nullptr || g == nullptr || !ens_flow_levels_ok(w))
        return hipErrorInvalidValue;
    const Phi4EnsFlowShape sh = phi4_ens_flow_shape(a.Lx * a.Ly * a.Lz, a.Lz);
    // the flow steps ping-pong as a step launch's do: its layout with the correlator
    const Phi4EnsLds l = sh.lds(kPhi4EnsLdsStep, phi4_ens_corr_bytes(a.Lz));
    Phi4EnsArgs q = a;
    Phi4EnsFlowArgs wq = w;
    int two = l.images == 2;
    void *args[] = {&q, &wq, &two, &first, &sums, &S, &g};
    return ens_launch(SQ_ENS_KERNEL(sh.K, phi4_ens_flowed_kernel), count, sh.T, l.bytes, args, s);
}

hipError_t phi4_ens_flow_field_launch(const Phi4EnsArgs &a, const Phi4EnsFlowArgs &w, int first, int count,
                                      int nsteps, float *out, hipStream_t s) {
    if (!ens_stored_ok(a, first, count) || out == nullptr || w.rec == nullptr || nsteps < 0 ||
        nsteps > kPhi4EnsMaxFlowSteps)
        return hipErrorInvalidValue;
    const Phi4EnsFlowShape sh = phi4_ens_flow_shape(a.Lx * a.Ly * a.Lz, a.Lz);
    const Phi4EnsLds l = sh.lds(kPhi4EnsLdsStep);  // the plain step launch's layout
    Phi4EnsArgs q = a;
    Phi4EnsFlowArgs wq = w;
    int two = l.images == 2;
    void *args[] = {&q, &wq, &two, &first, &nsteps, &out};
    return ens_launch(SQ_ENS_KERNEL(sh.K, phi4_ens_flow_field_kernel), count, sh.T, l.bytes, args, s);
}

}  // namespace sq
