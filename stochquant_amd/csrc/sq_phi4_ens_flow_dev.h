// sq_phi4_ens_flow_dev.h -- the device functions the gradient-flow kernels
// share (sq_phi4_ens_flow.hip, sq_phi4_ens_flow_frames.hip).
// It calls ens_step, ens_sums, ens_fold and ens_corr of sq_phi4_ens_dev.h and
// restates none of them.
#pragma once
#include "sq_phi4_ens_dev.h"

namespace sq {

namespace {

__device__ __forceinline__ Phi4StepArgs ens_flow_args(const Phi4EnsFlowRec &fr, float clampv) {
    Phi4StepArgs A{};
    A.h = fr.h;
    A.m2 = fr.m2;
    A.lam6 = fr.lam6;
    A.sig = 0.f;
    A.sigq = 0.f;
    A.clampv = clampv;
    return A;
}

// One flow step: c <- update(c, fc) with the noise off, the result to the other image, behind a barrier.
template <int K>
__device__ __forceinline__ void ens_flow_step(const Phi4StepArgs &FA, const EnsGeo &g, float4 (&c)[K],
                                              const uint32_t (&fl)[K], float *&fc, float *&fo, int two) {
    const int T = blockDim.x;
    float fam = 0.f;  // thrown away: a clamp hit during the flow sets no flag
    ens_step<K, false>(FA, g, c, fl, fc, 0u, 0u, fam);
    if (!two) __syncthreads();  // one image: every wave has read it
    {
        float *x = fc;
        fc = fo;
        fo = x;
    }
    float4 *fc4 = reinterpret_cast<float4 *>(fc);
#pragma unroll
    for (int j = 0; j < K; ++j)
        if (fl[j] & kEnsValid) fc4[(int)threadIdx.x + j * T] = c[j];
    __syncthreads();
}

// The lane's K flag words from where the kernel keeps them: an array (the Euler kernels) or EnsFlagsPk (the
// Heun kernels, whose get() is opaque per use: the unpacked words live for one flow step, not for the block).
template <int K>
__device__ __forceinline__ void ens_flow_flags(const uint32_t (&fp)[K], uint32_t (&fl)[K]) {
#pragma unroll
    for (int j = 0; j < K; ++j) fl[j] = fp[j];
}
template <int K>
__device__ __forceinline__ void ens_flow_flags(const EnsFlagsPk<K> &fp, uint32_t (&fl)[K]) {
#pragma unroll
    for (int j = 0; j < K; ++j) fl[j] = fp.get(j);
}

// The flow of one measurement point, measuring on the way: from the field in c and the image fc (the same
// field, behind a block barrier) to each of W's levels in one pass, level 0 before the first flow step.  At
// level l the four sums go to ser + 4 l gridDim.x (ser: the record's row of replica r at level 0; nullable)
// and, CORR and corr (block-uniform), one ens_corr measurement into W's accumulators of (r, l), the slice sums
// through Sl.  The caller asks for at least one of the two.  The flow steps use the two images only (fc, fo;
// the same one when !two), the sums scr, the correlator Sl: nothing behind them is touched.  Every level's
// measurement ends in a block barrier behind its last image read (ens_fold's, ens_corr's), so on return no
// wave reads an image; c and the images hold the field of the last level, in either image.
template <int K, bool CORR, typename FL>
__device__ __forceinline__ void ens_flow_measure(const Phi4EnsArgs &E, const Phi4EnsFlowArgs &W, const EnsGeo &g,
                                                 int r, float4 (&c)[K], const FL &fp, float *fc, float *fo,
                                                 int two, double *scr, double *Sl, double *ser, bool corr,
                                                 unsigned tid = threadIdx.x) {
    const Phi4StepArgs FA = ens_flow_args(W.rec[r], E.clampv);
    const int nlev = W.nlev;
    const int nt = E.Lz / 2 + 1;
    int done = 0;
    for (int l = 0; l < nlev; ++l) {
        const int n = W.lev[l];
        for (; done < n; ++done) {
            uint32_t fl[K];
            ens_flow_flags<K>(fp, fl);
            ens_flow_step<K>(FA, g, c, fl, fc, fo, two);
        }
        if (ser != nullptr) {
            double sm[4];
            float mx;
            uint32_t fl[K];
            ens_flow_flags<K>(fp, fl);
            ens_sums<K>(g, c, fl, fc, sm, mx);
            ens_fold(sm, mx, scr, ser + 4 * (size_t)l * gridDim.x, false, tid);
        }
        if constexpr (CORR) {
            if (corr) {
                const size_t a = (size_t)r * (size_t)nlev + (size_t)l;
                ens_corr<true>(g, E.Lz, fc, Sl, W.G + a * (size_t)nt, W.S1 + a, W.nmeas + a, nullptr, tid);
            }
        }
    }
}

}  // namespace

}  // namespace sq
