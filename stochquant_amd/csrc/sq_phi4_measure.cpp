// sq_phi4_measure.cpp -- in-stream measurements of the single phi^4 lattice: sq_phi4_set_momenta,
// sq_phi4_get_momenta, sq_phi4_measure, sq_phi4_step_hmc_meas, sq_phi4_step_heun_meas, sq_phi4_step_heun_fused_meas, sq_phi4_step_hmc_cluster_meas, sq_phi4_corr_sums,
// sq_phi4_corr_reset, sq_phi4_measure_shape_info (include/stochquant.h; the kernels and the order of every sum
// are sq_phi4_measure.hip's).  A measurement is three launches on the slab's step stream; the host reads nothing
// back between them, nor between the trajectories, sweeps and measurements of a call.
#include <cstring>
#include <vector>

#include "sq_ctx.h"
#include "sq_phi4_ens_ckpt_format.h"  // momenta_error: the ensemble setter's argument rules
#include "sq_phi4_measure.h"

using namespace sq;

namespace {

constexpr int kMaxM = SQ_PHI4_ENS_MAX_MOMENTA;
constexpr int kMaxQ = 1 + 2 * kMaxM;

// The checks every entry point shares: a PHI4 context of one periodic slab.
int meas_ctx_check(sq_ctx *c) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "in-stream measurements are for PHI4 contexts");
    if (c->p.comm != SQ_COMM_NONE || c->slabs.size() != 1)
        return fail(SQ_E_STATE, "in-stream measurements run on one periodic slab (comm none)");
    return SQ_OK;
}

// every >= 1, measure within bits 0 and 1, bit 1 only with momenta set
int meas_call_check(sq_ctx *c, int every, int measure) {
    int rc = meas_ctx_check(c);
    if (rc) return rc;
    if (every < 1) return fail(SQ_E_ARG, "every must be >= 1");
    if (measure & ~3) return fail(SQ_E_ARG, "measure has bits 0 (correlator) and 1 (momenta) only");
    if ((measure & 2) && c->mz_M == 0) return fail(SQ_E_STATE, "no momenta set (sq_phi4_set_momenta)");
    return SQ_OK;
}

size_t meas_nz(const sq_ctx *c) { return (size_t)c->slabs[0].nz; }
size_t meas_nt(const sq_ctx *c) { return meas_nz(c) / 2 + 1; }
double *out_sums(const sq_ctx *c) { return c->mz_out + (size_t)kMaxQ * meas_nz(c); }
double *out_row(const sq_ctx *c) { return out_sums(c) + 3; }
double *out_g(const sq_ctx *c) { return out_row(c) + 4; }
double *acc_G(const sq_ctx *c) { return c->mz_acc; }
double *acc_Gp(const sq_ctx *c) { return c->mz_acc + meas_nt(c); }
double *acc_S1(const sq_ctx *c) { return c->mz_acc + (size_t)(1 + kMaxM) * meas_nt(c); }
size_t acc_doubles(const sq_ctx *c) { return (size_t)(1 + kMaxM) * meas_nt(c) + 3; }

int meas_alloc_acc(sq_ctx *c) {
    if (c->mz_acc != nullptr) return SQ_OK;
    SQ_HIP(hipMalloc(&c->mz_acc, acc_doubles(c) * sizeof(double)));
    SQ_HIP(phi4_meas_clear_launch(c->mz_acc, acc_doubles(c), c->slabs[0].sA));
    return SQ_OK;
}

// The buffers of measurements with M momenta and `rows` series rows.
int meas_reserve(sq_ctx *c, int M, size_t rows) {
    const Phi4StepArgs a = phi4_periodic_args(c);
    const size_t nz = meas_nz(c), nt = meas_nt(c);
    const size_t part = nz * (size_t)a.nxseg * (size_t)a.nyg * (size_t)(1 + 2 * M);
    if (part > c->mz_part_cap) {
        (void)hipFree(c->mz_part);
        c->mz_part = nullptr;
        c->mz_part_cap = 0;
        SQ_HIP(hipMalloc(&c->mz_part, part * sizeof(double)));
        c->mz_part_cap = part;
    }
    if (c->mz_nunits != a.nunits) {
        (void)hipFree(c->mz_tot);
        c->mz_tot = nullptr;
        c->mz_nunits = 0;
        SQ_HIP(hipMalloc(&c->mz_tot, 3 * (size_t)a.nunits * sizeof(double)));
        c->mz_nunits = a.nunits;
    }
    if (c->mz_out == nullptr)
        SQ_HIP(hipMalloc(&c->mz_out, ((size_t)kMaxQ * nz + 7 + (size_t)(1 + kMaxM) * nt) * sizeof(double)));
    if (rows > c->mz_series_cap) {
        (void)hipFree(c->mz_series);
        c->mz_series = nullptr;
        c->mz_series_cap = 0;
        SQ_HIP(hipMalloc(&c->mz_series, rows * 4 * sizeof(double)));
        c->mz_series_cap = rows;
    }
    return meas_alloc_acc(c);
}

// One measurement of the current field with M momenta, enqueued on the step stream: the row {S1, S2, S4, NN} to
// `row` (device memory), g and g_m to out_g when `gout`, the accumulators advanced as `acc` says.
int meas_enqueue(sq_ctx *c, int M, double *row, bool gout, int acc) {
    hipStream_t st = c->slabs[0].sA;
    const Phi4StepArgs a = phi4_periodic_args(c);
    const size_t Lx = (size_t)c->Lx, Ly = (size_t)c->Ly;
    Phi4MeasArgs w{};
    w.part = c->mz_part;
    w.tot = c->mz_tot;
    w.M = M;
    if (M > 0) {
        w.cx = c->mz_tab;
        w.sx = c->mz_tab + kMaxM * Lx;
        w.cy = c->mz_tab + 2 * kMaxM * Lx;
        w.sy = c->mz_tab + 2 * kMaxM * Lx + kMaxM * Ly;
    }
    SQ_HIP(phi4_meas_launch(a, c->geom, w, st));
    Phi4MeasFoldArgs f{};
    f.part = c->mz_part;
    f.tot = c->mz_tot;
    f.nz = a.nz;
    f.nj = a.nxseg * a.nyg;
    f.nq = 1 + 2 * M;
    f.nunits = a.nunits;
    f.sl = c->mz_out;
    f.sums = out_sums(c);
    SQ_HIP(phi4_meas_fold_launch(f, st));
    Phi4MeasCorrArgs k{};
    k.sl = c->mz_out;
    k.sums = out_sums(c);
    k.nz = a.nz;
    k.nt = (int)meas_nt(c);
    k.M = M;
    k.lds = phi4_meas_corr_lds(a.nz, M);
    k.row = row;
    k.gout = gout ? out_g(c) : nullptr;
    k.acc = acc;
    k.G = acc_G(c);
    k.Gp = acc_Gp(c);
    k.S1acc = acc_S1(c);
    k.nmeas = reinterpret_cast<long long *>(acc_S1(c) + 1);
    SQ_HIP(phi4_meas_corr_launch(k, st));
    c->perf.kernel_launches += 3;
    return SQ_OK;
}

int series_fetch(sq_ctx *c, double *series, size_t rows) {
    SQ_HIP(hipMemcpyAsync(series, c->mz_series, rows * 4 * sizeof(double), hipMemcpyDeviceToHost, c->slabs[0].sA));
    return SQ_OK;
}

}  // namespace

namespace sq {

void release_measure(sq_ctx *c) {
    (void)hipFree(c->mz_tab);
    (void)hipFree(c->mz_part);
    (void)hipFree(c->mz_tot);
    (void)hipFree(c->mz_out);
    (void)hipFree(c->mz_acc);
    (void)hipFree(c->mz_series);
    c->mz_tab = c->mz_part = c->mz_tot = c->mz_out = c->mz_acc = c->mz_series = nullptr;
    c->mz_part_cap = c->mz_series_cap = 0;
    c->mz_nunits = 0;
    c->mz_M = 0;
}

}  // namespace sq

extern "C" {

int sq_phi4_set_momenta(sq_ctx *c, int M, const int *nxy) {
    int rc = meas_ctx_check(c);
    if (rc) return rc;
    if (const char *why = ckpt::momenta_error(c->Lx, c->Ly, M, nxy)) return fail(SQ_E_ARG, why);
    DeviceGuard g(c->dev);
    const size_t Lx = (size_t)c->Lx, Ly = (size_t)c->Ly, nx = kMaxM * Lx, ny = kMaxM * Ly;
    std::vector<double> tab(2 * (nx + ny), 0.0);
    for (int m = 0; m < M; ++m) {
        rc = sq_phi4_ens_momentum_table(c->Lx, nxy[2 * m], &tab[(size_t)m * Lx], &tab[nx + (size_t)m * Lx]);
        if (rc) return rc;
        if (c->Ly == 1) {  // the table function wants L >= 2; one row has the one twiddle (1, 0)
            tab[2 * nx + (size_t)m] = 1.0;
        } else {
            rc = sq_phi4_ens_momentum_table(c->Ly, nxy[2 * m + 1], &tab[2 * nx + (size_t)m * Ly],
                                            &tab[2 * nx + ny + (size_t)m * Ly]);
            if (rc) return rc;
        }
    }
    hipStream_t st = c->slabs[0].sA;
    SQ_HIP(hipStreamSynchronize(st));  // measurements in flight read the old tables
    if (c->mz_tab == nullptr) SQ_HIP(hipMalloc(&c->mz_tab, tab.size() * sizeof(double)));
    SQ_HIP(hipMemcpy(c->mz_tab, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice));
    rc = meas_alloc_acc(c);
    if (rc) return rc;
    // the momentum accumulators belong to the list: they start over, as the ensemble's do
    SQ_HIP(phi4_meas_clear_launch(acc_Gp(c), (size_t)kMaxM * meas_nt(c), st));
    SQ_HIP(phi4_meas_clear_launch(acc_S1(c) + 2, 1, st));
    c->mz_M = M;
    for (int i = 0; i < 2 * M; ++i) c->mz_n[i] = nxy[i];
    return SQ_OK;
}

int sq_phi4_get_momenta(sq_ctx *c, int *M, int *nxy) {
    int rc = meas_ctx_check(c);
    if (rc) return rc;
    if (!M) return fail(SQ_E_ARG, "null argument");
    *M = c->mz_M;
    if (nxy)
        for (int i = 0; i < 2 * c->mz_M; ++i) nxy[i] = c->mz_n[i];
    return SQ_OK;
}

int sq_phi4_measure(sq_ctx *c, double *sums4, double *S, double *AB, double *g, double *gp) {
    int rc = meas_ctx_check(c);
    if (rc) return rc;
    if ((AB || gp) && c->mz_M == 0) return fail(SQ_E_STATE, "no momenta set (sq_phi4_set_momenta)");
    DeviceGuard dg(c->dev);
    rc = gate_check(c, false);
    if (rc || (!sums4 && !S && !AB && !g && !gp)) return rc;
    const int M = (AB || gp) ? c->mz_M : 0;
    rc = meas_reserve(c, M, 0);
    if (!rc) rc = meas_enqueue(c, M, out_row(c), g != nullptr || gp != nullptr, 0);
    if (rc) return rc;
    hipStream_t st = c->slabs[0].sA;
    const size_t nz = meas_nz(c), nt = meas_nt(c);
    std::vector<double> ab(AB ? 2 * (size_t)M * nz : 0);
    if (sums4) SQ_HIP(hipMemcpyAsync(sums4, out_row(c), 4 * sizeof(double), hipMemcpyDeviceToHost, st));
    if (S) SQ_HIP(hipMemcpyAsync(S, c->mz_out, nz * sizeof(double), hipMemcpyDeviceToHost, st));
    if (AB) SQ_HIP(hipMemcpyAsync(ab.data(), c->mz_out + nz, ab.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    if (g) SQ_HIP(hipMemcpyAsync(g, out_g(c), nt * sizeof(double), hipMemcpyDeviceToHost, st));
    if (gp) SQ_HIP(hipMemcpyAsync(gp, out_g(c) + nt, (size_t)M * nt * sizeof(double), hipMemcpyDeviceToHost, st));
    SQ_HIP(hipStreamSynchronize(st));
    if (AB)  // the device keeps A_m and B_m as rows of nz; the caller's layout is [M][nz][2]
        for (size_t m = 0; m < (size_t)M; ++m)
            for (size_t z = 0; z < nz; ++z) {
                AB[(m * nz + z) * 2] = ab[2 * m * nz + z];
                AB[(m * nz + z) * 2 + 1] = ab[(2 * m + 1) * nz + z];
            }
    return SQ_OK;
}

int sq_phi4_step_hmc_meas(sq_ctx *c, int ntraj, int nleap, int randomize, int every, double *series, int measure,
                          double *rec) {
    int rc = phi4_hmc_check(c, ntraj, nleap);
    if (!rc) rc = meas_call_check(c, every, measure);
    if (rc || ntraj == 0) return rc;
    DeviceGuard g(c->dev);
    const size_t rows = (size_t)(ntraj / every);
    const int M = (measure & 2) ? c->mz_M : 0;
    rc = phi4_hmc_reserve(c, rec ? (size_t)ntraj : 0);
    if (!rc) rc = meas_reserve(c, M, rows);
    for (int t = 0; t < ntraj && !rc; ++t) {
        rc = phi4_hmc_enqueue(c, 1, nleap, randomize, (size_t)t, rec != nullptr);
        if (!rc && (t + 1) % every == 0) rc = meas_enqueue(c, M, c->mz_series + 4 * (size_t)((t + 1) / every - 1), false, measure);
    }
    if (!rc && rec) rc = phi4_hmc_fetch(c, rec, (size_t)ntraj);
    if (!rc && series && rows) rc = series_fetch(c, series, rows);
    if (rc) return rc;
    if (rec || (series && rows)) SQ_HIP(hipStreamSynchronize(c->slabs[0].sA));
    return SQ_OK;
}

// The loop of sq_phi4_step_heun_meas and sq_phi4_step_heun_fused_meas: check / enqueue are the step's parts.
static int heun_meas(sq_ctx *c, int nsteps, int every, double *series, int measure, int (*check)(sq_ctx *, int),
                     int (*enqueue)(sq_ctx *, int)) {
    int rc = check(c, nsteps);
    if (!rc) rc = meas_call_check(c, every, measure);
    if (rc || nsteps == 0) return rc;
    DeviceGuard g(c->dev);
    const size_t rows = (size_t)(nsteps / every);
    const int M = (measure & 2) ? c->mz_M : 0;
    rc = meas_reserve(c, M, rows);
    for (int t = 0; t < nsteps && !rc; ++t) {
        rc = enqueue(c, 1);
        if (!rc && (t + 1) % every == 0) rc = meas_enqueue(c, M, c->mz_series + 4 * (size_t)((t + 1) / every - 1), false, measure);
    }
    if (!rc && series && rows) rc = series_fetch(c, series, rows);
    if (rc) return rc;
    if (series && rows) SQ_HIP(hipStreamSynchronize(c->slabs[0].sA));
    return SQ_OK;
}

int sq_phi4_step_heun_meas(sq_ctx *c, int nsteps, int every, double *series, int measure) {
    return heun_meas(c, nsteps, every, series, measure, phi4_heun_check, phi4_heun_enqueue);
}

int sq_phi4_step_heun_fused_meas(sq_ctx *c, int nsteps, int every, double *series, int measure) {
    return heun_meas(c, nsteps, every, series, measure, phi4_heun_fused_check, phi4_heun_fused_enqueue);
}

int sq_phi4_step_hmc_cluster_meas(sq_ctx *c, int nrounds, int ntraj, int nleap, int randomize, int every, double *series,
                                  int measure, double *rec_hmc, unsigned char *bonds, int *labels) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (nrounds < 0) return fail(SQ_E_ARG, "nrounds must be >= 0");
    int rc = phi4_hmc_check(c, ntraj, nleap);
    if (!rc) rc = phi4_cluster_check(c);
    if (!rc) rc = meas_call_check(c, every, measure);
    if (rc || nrounds == 0) return rc;
    DeviceGuard g(c->dev);
    const bool rec = bonds != nullptr || labels != nullptr;
    const size_t rows = (size_t)nrounds * (size_t)ntraj, srows = (size_t)(nrounds / every);
    const int M = (measure & 2) ? c->mz_M : 0;
    if (ntraj > 0) rc = phi4_hmc_reserve(c, rec_hmc ? rows : 0);
    if (!rc) rc = phi4_cluster_reserve(c, rec ? (size_t)nrounds : 0);
    if (!rc) rc = meas_reserve(c, M, srows);
    for (int r = 0; r < nrounds && !rc; ++r) {
        rc = phi4_hmc_enqueue(c, ntraj, nleap, randomize, (size_t)r * (size_t)ntraj, rec_hmc != nullptr);
        if (!rc) rc = phi4_cluster_enqueue(c, rec ? r : -1);
        if (!rc && (r + 1) % every == 0) rc = meas_enqueue(c, M, c->mz_series + 4 * (size_t)((r + 1) / every - 1), false, measure);
    }
    if (!rc && rec_hmc && rows) rc = phi4_hmc_fetch(c, rec_hmc, rows);
    if (!rc && rec) rc = phi4_cluster_fetch(c, nrounds, bonds, labels);
    if (!rc && series && srows) rc = series_fetch(c, series, srows);
    if (rc) return rc;
    if (rec || (rec_hmc && rows) || (series && srows)) SQ_HIP(hipStreamSynchronize(c->slabs[0].sA));
    return SQ_OK;
}

int sq_phi4_corr_sums(sq_ctx *c, double *G, double *S1, long long *nmeas, double *Gp, long long *nmeas_p) {
    int rc = meas_ctx_check(c);
    if (rc) return rc;
    const size_t nt = meas_nt(c), M = (size_t)c->mz_M;
    std::vector<double> a(acc_doubles(c), 0.0);
    if (c->mz_acc != nullptr) {  // else nothing has been measured: all zero
        DeviceGuard g(c->dev);
        hipStream_t st = c->slabs[0].sA;
        SQ_HIP(hipMemcpyAsync(a.data(), c->mz_acc, a.size() * sizeof(double), hipMemcpyDeviceToHost, st));
        SQ_HIP(hipStreamSynchronize(st));
    }
    const double *tail = a.data() + (1 + kMaxM) * nt;
    if (G) memcpy(G, a.data(), nt * sizeof(double));
    if (Gp && M) memcpy(Gp, a.data() + nt, M * nt * sizeof(double));
    if (S1) *S1 = tail[0];
    if (nmeas) memcpy(nmeas, tail + 1, sizeof(long long));
    if (nmeas_p) memcpy(nmeas_p, tail + 2, sizeof(long long));
    return SQ_OK;
}

int sq_phi4_corr_reset(sq_ctx *c) {
    int rc = meas_ctx_check(c);
    if (rc) return rc;
    if (c->mz_acc == nullptr) return SQ_OK;
    DeviceGuard g(c->dev);
    // behind the measurements in flight; a zero double and a zero 64-bit integer are the same bits
    SQ_HIP(phi4_meas_clear_launch(c->mz_acc, acc_doubles(c), c->slabs[0].sA));
    return SQ_OK;
}

int sq_phi4_measure_shape_info(const long long dims[3], int M, long long out[4]) {
    if (!dims || !out) return fail(SQ_E_ARG, "null argument");
    Phi4Geom geom{};
    if (dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0 || dims[0] > (1 << 20) || dims[1] > (1 << 20) ||
        dims[2] >= (1ll << 31) || !phi4_geometry((int)dims[0], (int)dims[1], &geom) ||
        dims[0] * dims[1] * dims[2] / 4 >= (1ll << 32) || dims[0] * dims[1] * 4 >= (1ll << 31))
        return fail(SQ_E_ARG, "not a shape sq_create accepts for a PHI4 context");
    if (M < 0 || M > kMaxM) return fail(SQ_E_ARG, "0 <= M <= SQ_PHI4_ENS_MAX_MOMENTA momenta");
    const long long nj = (dims[0] / (4 * geom.qx * geom.v)) * ((dims[1] + geom.wy - 1) / geom.wy);
    out[0] = nj;
    out[1] = dims[2] * nj * (1 + 2 * M) * (long long)sizeof(double);
    out[2] = phi4_meas_corr_lds(dims[2], M);
    out[3] = dims[2] / 2 + 1;
    return SQ_OK;
}

}  // extern "C"
