// sq_phi4_measure.h -- the launches of the single lattice's in-stream measurement
// (sq_phi4_measure.hip) as its host code (sq_phi4_measure.cpp) enqueues them.  Not installed.
#pragma once
#include "sq_internal.h"

namespace sq {

constexpr int kPhi4MeasMaxMomenta = 8;       // SQ_PHI4_ENS_MAX_MOMENTA
constexpr int kPhi4MeasCorrLds = 64 * 1024;  // the correlator launch keeps its slices in LDS up to here

// The march's outputs.  nq = 1 + 2 M doubles per (plane, unit of the plane): S, then A_m, B_m per momentum.
struct Phi4MeasArgs {
    double *part;      // [nz][nj][nq], nj = nxseg nyg, j = x-span + nxseg row-group
    double *tot;       // [nunits][3]: the unit's chunk totals of phi^2, phi^4, phi (phi_x+1 + phi_y+1 + phi_z+1)
    const double *cx, *sx, *cy, *sy;  // [kPhi4MeasMaxMomenta][Lx] twice, [..][Ly] twice (M > 0)
    int M;
};

struct Phi4MeasFoldArgs {
    const double *part, *tot;
    int nz, nj, nq, nunits;
    double *sl;    // [nq][nz]: S(z), then A_m(z), B_m(z)
    double *sums;  // [3]: the totals of phi^2, phi^4, the forward neighbour sum
};

struct Phi4MeasCorrArgs {
    const double *sl, *sums;  // the fold's outputs
    int nz, nt, M;            // M: momenta whose g_m the launch forms (0: only g)
    int lds;                  // the slices of a block in LDS (16 nz bytes at most)
    double *row;              // {S1, S2, S4, NN}
    double *gout;             // [1 + M][nt] = g, g_m; nullable
    int acc;                  // bit 0: G += g, S1acc += S1, nmeas += 1; bit 1: Gp[m] += g_m, nmeas_p += 1
    double *G, *Gp, *S1acc;   // [nt], [M][nt], one
    long long *nmeas;         // {nmeas, nmeas_p}
};

// a: the periodic single-slab decomposition of the Euler step (phi4_periodic_args); only a.in is read
hipError_t phi4_meas_launch(const Phi4StepArgs &a, const Phi4Geom &g, const Phi4MeasArgs &w, hipStream_t s);
hipError_t phi4_meas_fold_launch(const Phi4MeasFoldArgs &f, hipStream_t s);
hipError_t phi4_meas_corr_launch(const Phi4MeasCorrArgs &k, hipStream_t s);
// LDS bytes of the correlator launch for nz planes (0: the slices are read from device memory)
int phi4_meas_corr_lds(long long nz, int M);
// n doubles at p to 0.0, stream-ordered (the accumulators' reset)
hipError_t phi4_meas_clear_launch(double *p, size_t n, hipStream_t s);

}  // namespace sq
