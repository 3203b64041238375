// sq_phi4_hmc.h -- the launches of the single lattice's HMC trajectory
// (sq_phi4_hmc.hip) as its host code (sq_phi4_hmc.cpp) enqueues them.  Not installed.
#pragma once
#include "sq_internal.h"

namespace sq {

// The trajectory's device words: the statistics of sq_phi4_hmc_stats, the trip
// word the passes raise and the verdict clears, the verdict's accept word for
// the commit, and the guard flag (set by a verdict 2, cleared by sq_phi4_hmc_reset).
struct Phi4HmcState {
    long long stat[4];  // trajectories, accepted, guard trips, leapfrog steps
    int trip, accept, flag, pad;
};

struct Phi4HmcVerdictArgs {
    const double *part_sub, *part_add;  // the two term passes' per-block sums, nblocks each
    int nblocks;
    int L;
    float sig;
    uint32_t k0, k1, s_lo, s_hi;
    Phi4HmcState *st;
    double *rec;  // the trajectory's row {dH, u, verdict, L} in device memory; nullable
};

// All passes take the periodic single-slab decomposition of the Euler step
// (phi4_fill_units over chunks of zc planes) and a.flag = &Phi4HmcState::trip.
int phi4_hmc_blocks(const Phi4StepArgs &a);  // blocks of a pass = doubles of a partials array
// a.in = phi_k, prev = phi_{k-1}, a.out = phi_{k+1} (prev == a.out: in place), a.h = 2h, a.sig = a.sigq = 0
hipError_t phi4_hmc_leap_launch(const Phi4StepArgs &a, const Phi4Geom &g, const float *prev, hipStream_t s);
// partials[block] = the block's sum of -+2 t(f, o): f = a.in with its stencil, o = a.out at the site, a.h = h;
// sub: the minus sign, and max |o| for the trip word
hipError_t phi4_hmc_term_launch(const Phi4StepArgs &a, const Phi4Geom &g, bool sub, double *partials, hipStream_t s);
hipError_t phi4_hmc_verdict_launch(const Phi4HmcVerdictArgs &w, hipStream_t s);
// dst[0 .. n) = src[0 .. n) when st->accept == 1 (n a multiple of 4)
hipError_t phi4_hmc_commit_launch(const float *src, float *dst, size_t n, const Phi4HmcState *st, hipStream_t s);

}  // namespace sq
