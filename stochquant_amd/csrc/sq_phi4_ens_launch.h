// sq_phi4_ens_launch.h -- the one launch path of the phi^4 lattice ensemble's
// kernels: host code, included by the sq_phi4_ens*.hip translation units only.
// A launcher refuses its arguments with the predicates below (every refusal is
// hipErrorInvalidValue), asks Phi4EnsShape::lds for its layout, picks the
// instance of the lattice's K with SQ_ENS_KERNEL and hands it to ens_launch.
#pragma once
#include "sq_phi4_ens.h"

// The instance of a kernel template for K quads per lane (Phi4EnsShape::K: 1, 2, 4 or 8), K the template's
// first parameter and the rest, if any, behind it: SQ_ENS_KERNEL(sh.K, phi4_ens_heun_frames_kernel, TWO, CA...).
// The templates' parameter lists differ (<K>, <K, CA...>, <K, TWO, CA...>), hence a macro.
#define SQ_ENS_KERNEL(K, kernel, ...)                           \
    ((K) == 1   ? (const void *)&kernel<1, ##__VA_ARGS__>       \
     : (K) == 2 ? (const void *)&kernel<2, ##__VA_ARGS__>       \
     : (K) == 4 ? (const void *)&kernel<4, ##__VA_ARGS__>       \
                : (const void *)&kernel<8, ##__VA_ARGS__>)

namespace sq {

namespace {

hipError_t ens_lds_attr(const void *fn, int bytes) {
    // above the default dynamic-LDS ceiling the function needs the attribute (once per instance and device;
    // setting it again is harmless)
    if (bytes <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

// One work-group of T lanes per grid entry, `bytes` of dynamic LDS.
hipError_t ens_launch(const void *fn, int grid, int T, int bytes, void **args, hipStream_t s) {
    const hipError_t e = ens_lds_attr(fn, bytes);
    if (e != hipSuccess) return e;
    return hipLaunchKernel(fn, dim3((unsigned)grid), dim3((unsigned)T), args, (size_t)bytes, s);
}

bool ens_shape_ok(const Phi4EnsArgs &a) {
    const long long S = (long long)a.Lx * a.Ly * a.Lz;
    return (a.Lx == 8 || a.Lx == 16 || a.Lx == 32 || a.Lx == 64) && a.Ly >= 2 && a.Lz >= 2 &&
           S <= kPhi4EnsMaxSites && a.field != nullptr && a.rec != nullptr;
}

// The launches that advance every replica: the field's shape, the guard flags, the grid.
bool ens_run_ok(const Phi4EnsArgs &a, int nrep) { return ens_shape_ok(a) && a.flags != nullptr && nrep >= 1; }

// The step launches of every sampler.  meas: the launch measures after each every-th step whether or not
// a.series is given, so every >= 1; else every may be 0 without a series.
bool ens_step_ok(const Phi4EnsArgs &a, int nrep, bool meas) {
    return ens_run_ok(a, nrep) && a.nsteps >= 0 && a.every >= (meas ? 1 : 0) && (a.series == nullptr || a.every >= 1);
}

// The frames launches.
bool ens_frames_ok(const Phi4EnsArgs &a, const Phi4EnsFrameArgs &f, int nrep) {
    return ens_run_ok(a, nrep) && f.nframes >= 1 && f.loops >= 1 && f.st != nullptr && f.stable != nullptr &&
           f.dtau != nullptr && f.recs != nullptr;
}

// The launches that measure the stored fields of replicas first .. first + count.
bool ens_stored_ok(const Phi4EnsArgs &a, int first, int count) { return ens_shape_ok(a) && first >= 0 && count >= 1; }

bool ens_corr_ok(const Phi4EnsCorrArgs &c) { return c.G != nullptr && c.S1 != nullptr && c.nmeas != nullptr; }

bool ens_pcorr_ok(const Phi4EnsPCorrArgs &p, bool acc) {
    return p.cx != nullptr && p.sx != nullptr && p.cy != nullptr && p.sy != nullptr && p.M >= 1 &&
           p.M <= kPhi4EnsMaxMomenta && (!acc || (p.Gp != nullptr && p.nmeas_p != nullptr)) &&
           (p.corr.G == nullptr || ens_corr_ok(p.corr));
}

bool ens_flow_levels_ok(const Phi4EnsFlowArgs &w) {
    if (w.rec == nullptr || w.nlev < 1 || w.nlev > kPhi4EnsMaxFlowLevels) return false;
    for (int l = 0; l < w.nlev; ++l)
        if (w.lev[l] < (l ? w.lev[l - 1] + 1 : 0) || w.lev[l] > kPhi4EnsMaxFlowSteps) return false;
    return true;
}

// A flow measurement inside a step or frames launch: legal levels, something to measure (the sums to a.series
// or, corr, the correlator into w's accumulators) and, corr, those accumulators.
bool ens_flow_ok(const Phi4EnsArgs &a, const Phi4EnsFlowArgs &w, bool corr) {
    return ens_flow_levels_ok(w) && (a.series != nullptr || corr) &&
           (!corr || (w.G != nullptr && w.S1 != nullptr && w.nmeas != nullptr));
}

}  // namespace

}  // namespace sq
