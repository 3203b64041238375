// sq_phi4_cluster.h -- the launches of the single lattice's Swendsen-Wang cluster
// sweep (sq_phi4_cluster.hip) as its host code (sq_phi4_cluster.cpp) enqueues
// them, and the choice of the brick both share.  Not installed.
#pragma once
#include "sq_internal.h"

namespace sq {

// The sweeps' device words: the statistics of sq_phi4_cluster_stats and the two
// trip words.  Sweep number n of the context (counted from its first sweep, not
// the Philox counter, which the caller may set) raises and reads trip[n & 1]
// and its last kernel clears trip[(n + 1) & 1] for the sweep behind it: no
// kernel clears a word another block of the same launch may raise.
struct Phi4ClusterState {
    long long stat[5];  // sweeps, clusters, flipped clusters, flipped sites, unconverged sweeps
    int trip[2];
};

constexpr int kPhi4ClusterLanes = 512;         // lanes of a brick's work-group
constexpr int kPhi4ClusterMaxTile = 8192;      // sites of a brick: 16 per lane, 40 KiB of LDS
constexpr int kPhi4ClusterExtraBytes = 4 + 1;  // device bytes per site beside the field: label, bond byte

// The brick of tx x ty x tz sites one work-group labels in LDS, the bricks per
// axis (the last one in y and z may be partial) and the launch's dynamic LDS.
struct Phi4ClusterTile {
    int tx, ty, tz;
    int ntx, nty, ntz;
    int lds;
};

// spec: the text of SQ_CLUSTER_TILE ("tx,ty,tz") or null; a text that names no legal brick of the lattice is ignored.
Phi4ClusterTile phi4_cluster_tile(int Lx, int Ly, long long Lz, const char *spec);

struct Phi4ClusterArgs {
    float *field;      // [Lz][Ly][Lx], local plane 0 of the context's current buffer
    uint32_t *label;   // [sites]
    uint8_t *bonds;    // [sites], bits 0 .. 2 = the site's forward bonds x, y, z
    Phi4ClusterState *st;
    int Lx, Ly, Lz;
    Phi4ClusterTile t;
    int ltx;           // log2 tx
    int par;           // the sweep's trip word
    float h, sig;      // the record beta comes from
    uint32_t k0, k1, clo, chi;
};

// One sweep is these three launches in this order on one stream.
hipError_t phi4_cluster_tile_launch(const Phi4ClusterArgs &a, hipStream_t s);
hipError_t phi4_cluster_seam_launch(const Phi4ClusterArgs &a, hipStream_t s);
hipError_t phi4_cluster_flip_launch(const Phi4ClusterArgs &a, hipStream_t s);
// stat[0 .. 5) = 0, behind the sweeps in flight
hipError_t phi4_cluster_reset_launch(Phi4ClusterState *st, hipStream_t s);

}  // namespace sq
