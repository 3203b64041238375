// sq_ens.h -- the QM1D replica ensemble (sq_qm1d_ens.hip, the sq_ens_* entry
// points of sq_ens.cpp): R independent chains advanced together, one frame
// per launch, one work-group per replica.  Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sq {

// One replica's frame scalars, device-resident: the frame kernel reads them at
// its start and writes them at its end (adoption and the Δτ controller run in
// the kernel), so a sequence of frames is a sequence of launches.
struct EnsRec {
    double omega;            // ω (adopted by stable frames only)
    double lrgVl;            // carried running max |X| (never rolled back)
    double dtau;             // Δτ of the next frame
    unsigned long long tick; // Philox step index of the next frame's first step
    long long runs;          // running-mean count (stable frames add loops)
    long long steps_total;   // steps executed since creation (sq_ens_perf)
    uint32_t k0, k1;         // Philox key
    int lrgEl;               // carried leader index
    int stab_cnt;            // stable frames since the last Δτ change
};

struct EnsArgs {
    double *f, *x, *xx0;  // [R][N], replica r at offset r N
    EnsRec *rec;          // [R]
    int *verdict;         // this frame's R verdict slots (1 stable, 0 unstable); nullable
    int N, pot, loops, adapt;
    double a, a2, C, kconst;
};

// Register-kernel shape of a chain of N <= kQm1dRegMaxN sites (sq_qm1d.hip):
// K sites per lane, W waves.
bool qm1d_wave_shape(int N, int &K, int &W);

// One frame of every replica (grid = nrep work-groups).
hipError_t ens_frame_launch(const EnsArgs &a, int nrep, hipStream_t s);
// mean[i], err[i] (nullable) over the replicas of c_r[i] = xx0_r[i] - x_r[i] x_r[mid], i < n <= N: sums
// in double in replica order; err = sqrt(sum (c_r - mean)^2 / (R (R - 1))), 0 for R = 1.
hipError_t ens_correlator_launch(const double *x, const double *xx0, int N, int nrep, int n, double *mean,
                                 double *err, hipStream_t s);

}  // namespace sq
