// sq_phi4_cluster.cpp -- Swendsen-Wang cluster sweeps of the single phi^4 lattice: sq_phi4_cluster,
// sq_phi4_step_hmc_cluster, sq_phi4_cluster_stats, sq_phi4_cluster_reset, the sweep counter and
// sq_phi4_cluster_shape_info (include/stochquant.h; the kernels and the design are sq_phi4_cluster.hip's).
// A sweep is three launches on the slab's step stream; the host reads nothing back inside or between sweeps.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "sq_ctx.h"
#include "sq_phi4_cluster.h"

using namespace sq;

namespace {

Phi4ClusterTile make_tile(int Lx, int Ly, long long Lz, int tx, int ty, int tz) {
    Phi4ClusterTile t{};
    t.tx = tx;
    t.ty = ty;
    t.tz = tz;
    t.ntx = Lx / tx;
    t.nty = (Ly + ty - 1) / ty;
    t.ntz = (int)((Lz + tz - 1) / tz);
    t.lds = 5 * tx * ty * tz + 16;  // labels, bond bytes, the three pass flags
    return t;
}

float cluster_sigma(const sq_ctx *c) { return (float)(sqrt(2.0 * (double)(float)c->dtau) * c->p.C); }  // hmc_sigma's

// The checks every entry point shares: a PHI4 context of one periodic slab.
int cluster_ctx_check(sq_ctx *c) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "cluster sweeps are for PHI4 contexts");
    if (c->p.comm != SQ_COMM_NONE || c->slabs.size() != 1)
        return fail(SQ_E_STATE, "cluster sweeps run on one periodic slab (comm none)");
    return SQ_OK;
}

// Everything that stands against a sweep, before any device work.
int cluster_check(sq_ctx *c) {
    int rc = cluster_ctx_check(c);
    if (rc) return rc;
    if (cluster_sigma(c) == 0.0f)
        return fail(SQ_E_STATE, "a cluster sweep needs noise: beta = 2 dtau / sigma^2 has no value at sigma = 0");
    if ((long long)c->Lx * c->Ly * c->Lz >= (1ll << 31))
        return fail(SQ_E_STATE, "cluster sweeps need fewer than 2^31 sites (32-bit labels)");
    DeviceGuard g(c->dev);
    return gate_check(c, false);  // a pending sticky error: no sweep on a corrupt field
}

int cluster_alloc(sq_ctx *c, size_t rec_sweeps) {
    const size_t sites = (size_t)c->slabs[0].nz * plane_floats(c);
    if (c->clu_st == nullptr) {
        const Phi4ClusterTile t = phi4_cluster_tile(c->Lx, c->Ly, c->Lz, getenv("SQ_CLUSTER_TILE"));
        c->clu_tile[0] = t.tx;
        c->clu_tile[1] = t.ty;
        c->clu_tile[2] = t.tz;
        SQ_HIP(hipMalloc(&c->clu_label, sites * sizeof(uint32_t)));
        SQ_HIP(hipMalloc(&c->clu_bonds, sites));
        SQ_HIP(hipMalloc(&c->clu_st, sizeof(Phi4ClusterState)));
        SQ_HIP(hipMemset(c->clu_st, 0, sizeof(Phi4ClusterState)));
    }
    if (rec_sweeps > c->clu_rec_cap) {
        (void)hipFree(c->clu_rec_bonds);
        (void)hipFree(c->clu_rec_labels);
        c->clu_rec_bonds = nullptr;
        c->clu_rec_labels = nullptr;
        c->clu_rec_cap = 0;
        SQ_HIP(hipMalloc(&c->clu_rec_bonds, rec_sweeps * sites));
        SQ_HIP(hipMalloc(&c->clu_rec_labels, rec_sweeps * sites * sizeof(int)));
        c->clu_rec_cap = rec_sweeps;
    }
    return SQ_OK;
}

// One sweep at the context's counter, enqueued on the step stream; rec >= 0: its bonds and labels to that row of
// the record buffers by stream-ordered device copies.
int cluster_sweep(sq_ctx *c, long long rec) {
    Slab &s = c->slabs[0];
    hipStream_t st = s.sA;
    const size_t sites = (size_t)s.nz * plane_floats(c);
    Phi4ClusterArgs a{};
    a.field = plane0(c, s, c->cur);
    a.label = c->clu_label;
    a.bonds = c->clu_bonds;
    a.st = c->clu_st;
    a.Lx = c->Lx;
    a.Ly = c->Ly;
    a.Lz = (int)c->Lz;
    a.t = make_tile(c->Lx, c->Ly, c->Lz, c->clu_tile[0], c->clu_tile[1], c->clu_tile[2]);
    for (a.ltx = 0; (1 << a.ltx) < a.t.tx; ++a.ltx) {
    }
    a.par = (int)(c->clu_seq & 1);
    a.h = (float)c->dtau;
    a.sig = cluster_sigma(c);
    a.k0 = (uint32_t)c->p.seed;
    a.k1 = (uint32_t)(c->p.seed >> 32);
    a.clo = (uint32_t)c->clu_sweep;
    a.chi = (uint32_t)(c->clu_sweep >> 32);
    SQ_HIP(phi4_cluster_tile_launch(a, st));
    SQ_HIP(phi4_cluster_seam_launch(a, st));
    SQ_HIP(phi4_cluster_flip_launch(a, st));
    if (rec >= 0) {
        SQ_HIP(hipMemcpyAsync(c->clu_rec_bonds + (size_t)rec * sites, c->clu_bonds, sites, hipMemcpyDeviceToDevice, st));
        SQ_HIP(hipMemcpyAsync(c->clu_rec_labels + (size_t)rec * sites, c->clu_label, sites * sizeof(int),
                              hipMemcpyDeviceToDevice, st));
    }
    c->perf.kernel_launches += 3;
    c->clu_sweep += 1;
    c->clu_seq += 1;
    return SQ_OK;
}

// The records of n sweeps to the caller: one read-back, one synchronisation.
int cluster_fetch(sq_ctx *c, int n, unsigned char *bonds, int *labels) {
    hipStream_t st = c->slabs[0].sA;
    const size_t sites = (size_t)c->slabs[0].nz * plane_floats(c);
    if (bonds) SQ_HIP(hipMemcpyAsync(bonds, c->clu_rec_bonds, (size_t)n * sites, hipMemcpyDeviceToHost, st));
    if (labels)
        SQ_HIP(hipMemcpyAsync(labels, c->clu_rec_labels, (size_t)n * sites * sizeof(int), hipMemcpyDeviceToHost, st));
    return SQ_OK;
}

}  // namespace

namespace sq {

Phi4ClusterTile phi4_cluster_tile(int Lx, int Ly, long long Lz, const char *spec) {
    if (spec) {
        int tx = 0, ty = 0, tz = 0;
        char tail = 0;
        if (sscanf(spec, "%d,%d,%d%c", &tx, &ty, &tz, &tail) == 3 && tx >= 8 && tx <= 256 && (tx & (tx - 1)) == 0 &&
            Lx % tx == 0 && ty >= 1 && tz >= 1) {
            ty = std::min(ty, Ly);
            tz = (int)std::min<long long>(tz, Lz);
            if ((long long)tx * ty * tz <= kPhi4ClusterMaxTile) return make_tile(Lx, Ly, Lz, tx, ty, tz);
        }
    }
    // sq_phi4_cluster.hip, "The brick": x cut at 32, y at 16, z what is left of kPhi4ClusterMaxTile sites
    int tx = 8;
    while (tx < 32 && Lx % (2 * tx) == 0) tx *= 2;
    const int ty = std::min(Ly, 16);
    const int tz = (int)std::min<long long>(Lz, std::max(1, kPhi4ClusterMaxTile / (tx * ty)));
    return make_tile(Lx, Ly, Lz, tx, ty, tz);
}

// the sweep in its parts, which sq_phi4_step_hmc_cluster_meas (sq_phi4_measure.cpp) puts a measurement behind
int phi4_cluster_check(sq_ctx *c) { return cluster_check(c); }
int phi4_cluster_reserve(sq_ctx *c, size_t rec_sweeps) { return cluster_alloc(c, rec_sweeps); }
int phi4_cluster_enqueue(sq_ctx *c, long long rec) { return cluster_sweep(c, rec); }
int phi4_cluster_fetch(sq_ctx *c, int n, unsigned char *bonds, int *labels) { return cluster_fetch(c, n, bonds, labels); }

void release_cluster(sq_ctx *c) {
    (void)hipFree(c->clu_label);
    (void)hipFree(c->clu_bonds);
    (void)hipFree(c->clu_st);
    (void)hipFree(c->clu_rec_bonds);
    (void)hipFree(c->clu_rec_labels);
    c->clu_label = nullptr;
    c->clu_bonds = c->clu_rec_bonds = nullptr;
    c->clu_st = nullptr;
    c->clu_rec_labels = nullptr;
    c->clu_rec_cap = 0;
}

}  // namespace sq

extern "C" {

int sq_phi4_cluster(sq_ctx *c, int nsweeps, unsigned char *bonds, int *labels) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (nsweeps < 0) return fail(SQ_E_ARG, "nsweeps must be >= 0");
    int rc = cluster_check(c);
    if (rc || nsweeps == 0) return rc;
    DeviceGuard g(c->dev);
    const bool rec = bonds != nullptr || labels != nullptr;
    rc = cluster_alloc(c, rec ? (size_t)nsweeps : 0);
    for (int i = 0; i < nsweeps && !rc; ++i) rc = cluster_sweep(c, rec ? i : -1);
    if (!rc && rec) rc = cluster_fetch(c, nsweeps, bonds, labels);
    if (rc) return rc;
    if (rec) SQ_HIP(hipStreamSynchronize(c->slabs[0].sA));
    return SQ_OK;
}

int sq_phi4_step_hmc_cluster(sq_ctx *c, int nrounds, int ntraj, int nleap, int randomize, double *rec_hmc,
                             unsigned char *bonds, int *labels) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (nrounds < 0) return fail(SQ_E_ARG, "nrounds must be >= 0");
    int rc = phi4_hmc_check(c, ntraj, nleap);
    if (!rc) rc = cluster_check(c);
    if (rc || nrounds == 0) return rc;
    DeviceGuard g(c->dev);
    const bool rec = bonds != nullptr || labels != nullptr;
    const size_t rows = (size_t)nrounds * (size_t)ntraj;
    if (ntraj > 0) rc = phi4_hmc_reserve(c, rec_hmc ? rows : 0);
    if (!rc) rc = cluster_alloc(c, rec ? (size_t)nrounds : 0);
    for (int r = 0; r < nrounds && !rc; ++r) {
        rc = phi4_hmc_enqueue(c, ntraj, nleap, randomize, (size_t)r * (size_t)ntraj, rec_hmc != nullptr);
        if (!rc) rc = cluster_sweep(c, rec ? r : -1);
    }
    if (!rc && rec_hmc && rows) rc = phi4_hmc_fetch(c, rec_hmc, rows);
    if (!rc && rec) rc = cluster_fetch(c, nrounds, bonds, labels);
    if (rc) return rc;
    if (rec || (rec_hmc && rows)) SQ_HIP(hipStreamSynchronize(c->slabs[0].sA));
    return SQ_OK;
}

int sq_phi4_cluster_stats(sq_ctx *c, long long out[5]) {
    int rc = cluster_ctx_check(c);
    if (rc) return rc;
    if (!out) return fail(SQ_E_ARG, "null argument");
    memset(out, 0, 5 * sizeof(long long));
    if (c->clu_st == nullptr) return SQ_OK;  // no sweep yet
    DeviceGuard g(c->dev);
    hipStream_t st = c->slabs[0].sA;
    SQ_HIP(hipMemcpyAsync(out, c->clu_st->stat, 5 * sizeof(long long), hipMemcpyDeviceToHost, st));
    SQ_HIP(hipStreamSynchronize(st));
    return SQ_OK;
}

int sq_phi4_cluster_reset(sq_ctx *c) {
    int rc = cluster_ctx_check(c);
    if (rc) return rc;
    if (c->clu_st == nullptr) return SQ_OK;
    DeviceGuard g(c->dev);
    SQ_HIP(phi4_cluster_reset_launch(c->clu_st, c->slabs[0].sA));  // behind the sweeps in flight; the trip words stay
    return SQ_OK;
}

int sq_phi4_cluster_sweep(sq_ctx *c, unsigned long long *sweep) {
    if (!c || !sweep) return fail(SQ_E_ARG, "null argument");
    *sweep = c->clu_sweep;
    return SQ_OK;
}

int sq_phi4_set_cluster_sweep(sq_ctx *c, unsigned long long sweep) {
    if (!c) return fail(SQ_E_ARG, "null context");
    c->clu_sweep = sweep;
    return SQ_OK;
}

int sq_phi4_cluster_shape_info(const long long dims[3], int out[8]) {
    if (!dims || !out) return fail(SQ_E_ARG, "null argument");
    Phi4Geom geom{};
    if (dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0 || dims[0] > (1 << 20) || dims[1] > (1 << 20) ||
        dims[2] >= (1ll << 31) || !phi4_geometry((int)dims[0], (int)dims[1], &geom))
        return fail(SQ_E_ARG, "not a shape sq_create accepts for a PHI4 context");
    if (dims[0] * dims[1] * dims[2] >= (1ll << 31))
        return fail(SQ_E_ARG, "cluster sweeps need fewer than 2^31 sites (32-bit labels)");
    const Phi4ClusterTile t = phi4_cluster_tile((int)dims[0], (int)dims[1], dims[2], getenv("SQ_CLUSTER_TILE"));
    const int v[8] = {t.tx, t.ty, t.tz, t.ntx, t.nty, t.ntz, t.lds, kPhi4ClusterExtraBytes};
    memcpy(out, v, sizeof v);
    return SQ_OK;
}

}  // extern "C"
