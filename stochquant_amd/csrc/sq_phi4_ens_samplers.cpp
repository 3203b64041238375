// sq_phi4_ens_samplers.cpp -- the phi^4 ensemble's exact samplers: the Metropolis-adjusted Langevin step
// (sq_phi4_ens_mala.hip), hybrid Monte Carlo trajectories (sq_phi4_ens_hmc.hip), replica exchange
// (sq_phi4_ens_exchange.hip), Swendsen-Wang cluster sweeps (sq_phi4_ens_cluster.hip), and the two calls that
// run trajectories and one of the latter round by round without leaving the stream.
#include "sq_phi4_ens_host.h"

#include "sq_phi4_ens_ckpt_format.h"

using namespace sq;

// ---- MALA ----
extern "C" {

int sq_phi4_ens_step_mala(sq_phi4_ens *e, int nsteps, int every, double *series, int measure, double *rec) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nsteps < 0) return fail(SQ_E_ARG, "nsteps must be >= 0");
    if (measure & ~1) return fail(SQ_E_ARG, "measure holds bit 0 (correlator) only: a MALA step measures no momenta");
    if (measure ? every < 1 : every < 0)
        return fail(SQ_E_ARG, measure ? "a correlator measurement needs every >= 1" : "every must be >= 0");
    int rc = ens_needs_noise(e, "a MALA step", "without noise there is no proposal density");
    if (rc || nsteps == 0) return rc;
    const bool corr = (measure & 1) != 0;
    DeviceGuard g(e->dev);
    const size_t nrec = (every > 0 && series) ? (size_t)(nsteps / every) : 0;
    const size_t nd = nrec * (size_t)e->R * 4;
    const size_t nm = rec ? (size_t)nsteps * (size_t)e->R * 3 : 0;
    rc = ens_sync_recs(e);
    if (!rc) rc = ens_zeroed(e->mstat, 3 * (size_t)e->R);
    if (!rc) rc = ens_reserve(e->series, nd);
    if (!rc) rc = ens_reserve(e->mrec, nm);
    if (rc) return rc;
    sq::Phi4EnsArgs a = ens_args(e);
    a.nsteps = nsteps;
    a.every = (nd || corr) ? every : 0;
    a.series = nd ? e->series.data() : nullptr;
    sq::Phi4EnsMalaArgs w{};
    w.stat = e->mstat.data();
    w.rec = nm ? e->mrec.data() : nullptr;
    const sq::Phi4EnsCorrArgs c = ens_corr_args(e);
    SQ_HIP(sq::phi4_ens_mala_launch(a, w, corr ? &c : nullptr, e->R, e->stream));
    e->launches++;
    SQ_HIP(hipStreamSynchronize(e->stream));
    if (nd) memcpy(series, e->series.data(), sizeof(double) * nd);
    if (nm) memcpy(rec, e->mrec.data(), sizeof(double) * nm);
    ens_advance(e, (unsigned long long)nsteps);
    return SQ_OK;
}

int sq_phi4_ens_mala_stats(sq_phi4_ens *e, int first, int count, long long *out) {
    return ens_read_rows(e, &sq_phi4_ens::mstat, 3, first, count, out);  // no MALA step yet: zeros
}

int sq_phi4_ens_mala_reset(sq_phi4_ens *e, int first, int count) {
    return ens_clear_rows(e, &sq_phi4_ens::mstat, 3, first, count);
}

}  // extern "C"

// ---- HMC ----
namespace {

// The arguments of sq_phi4_ens_step_hmc, which the fused calls repeat round by round.
struct EnsHmc {
    int ntraj, nleap, randomize, every, measure;
    double *series, *rec;  // nullable
};

int ens_hmc_check(const EnsHmc &h) {
    if (h.ntraj < 0) return fail(SQ_E_ARG, "ntraj must be >= 0");
    if (h.nleap < 1 || h.nleap > SQ_PHI4_ENS_MAX_LEAP) return fail(SQ_E_ARG, "nleap must lie in [1, 4096]");
    if (h.measure & ~1)
        return fail(SQ_E_ARG, "measure holds bit 0 (correlator) only: a trajectory measures no momenta");
    if (h.measure ? h.every < 1 : h.every < 0)
        return fail(SQ_E_ARG, h.measure ? "a correlator measurement needs every >= 1" : "every must be >= 0");
    return SQ_OK;
}

// The fused calls' rule on top.
int ens_hmc_fused_check(int nrounds, const EnsHmc &h) {
    if (nrounds < 0) return fail(SQ_E_ARG, "nrounds must be >= 0");
    int rc = ens_hmc_check(h);
    if (rc) return rc;
    if (h.every > 0 && h.ntraj % h.every != 0)
        return fail(SQ_E_ARG, "every must divide ntraj: the measurements are those of the separate calls");
    return SQ_OK;
}

// One round's series and per-trajectory records, in doubles.
size_t ens_hmc_series(const sq_phi4_ens *e, const EnsHmc &h) {
    return (h.every > 0 && h.series) ? (size_t)(h.ntraj / h.every) * (size_t)e->R * 4 : 0;
}
size_t ens_hmc_recs(const sq_phi4_ens *e, const EnsHmc &h) {
    return h.rec ? (size_t)h.ntraj * (size_t)e->R * 4 : 0;
}

// Before the first launch of nrounds rounds: the device records, the counters, room for what the kernels write.
int ens_hmc_prepare(sq_phi4_ens *e, int nrounds, const EnsHmc &h) {
    int rc = ens_sync_recs(e);
    if (!rc) rc = ens_zeroed(e->hstat, 4 * (size_t)e->R);
    if (!rc) rc = ens_reserve(e->series, ens_hmc_series(e, h) * (size_t)nrounds);
    if (!rc) rc = ens_reserve(e->hrec, ens_hmc_recs(e, h) * (size_t)nrounds);
    return rc;
}

// nrounds rounds of h.ntraj trajectories with behind(i) enqueued behind round i's, then the synchronisation and
// the series and records to the caller.  A failed enqueue ends the loop; the stream is synchronised all the same.
// The caller advances the counters.
template <class Behind>
int ens_hmc_rounds(sq_phi4_ens *e, int nrounds, const EnsHmc &h, Behind behind) {
    const bool corr = (h.measure & 1) != 0;
    const size_t per = ens_hmc_series(e, h), perh = ens_hmc_recs(e, h);
    const size_t nd = per * (size_t)nrounds, nm = perh * (size_t)nrounds;
    sq::Phi4EnsHmcArgs w{};
    w.stat = e->hstat.data();
    w.nleap = h.nleap;
    w.randomize = h.randomize != 0 ? 1 : 0;
    const sq::Phi4EnsCorrArgs c = ens_corr_args(e);
    int rc = SQ_OK;
    for (int i = 0; i < nrounds && !rc; ++i) {
        if (h.ntraj > 0) {
            sq::Phi4EnsArgs a = ens_args(e);
            a.adv = e->adv + (unsigned long long)i * (unsigned long long)h.ntraj;
            a.nsteps = h.ntraj;
            a.every = (nd || corr) ? h.every : 0;
            a.series = nd ? e->series.data() + per * (size_t)i : nullptr;
            w.rec = nm ? e->hrec.data() + perh * (size_t)i : nullptr;
            const hipError_t he = sq::phi4_ens_hmc_launch(a, w, corr ? &c : nullptr, e->R, e->stream);
            if (he != hipSuccess) {
                rc = fail(SQ_E_HIP, std::string("phi4_ens_hmc_launch: ") + hipGetErrorString(he));
                break;
            }
            e->launches++;
        }
        rc = behind(i);
    }
    const hipError_t he = hipStreamSynchronize(e->stream);
    if (rc) return rc;
    SQ_HIP(he);
    if (nd) memcpy(h.series, e->series.data(), sizeof(double) * nd);
    if (nm) memcpy(h.rec, e->hrec.data(), sizeof(double) * nm);
    return SQ_OK;
}

}  // namespace

extern "C" {

int sq_phi4_ens_step_hmc(sq_phi4_ens *e, int ntraj, int nleap, int randomize, int every, double *series, int measure,
                         double *rec) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    const EnsHmc h{ntraj, nleap, randomize, every, measure, series, rec};
    int rc = ens_hmc_check(h);
    if (!rc) rc = ens_needs_noise(e, "a trajectory", "without noise there is no momentum to draw");
    if (rc || ntraj == 0) return rc;
    DeviceGuard g(e->dev);
    rc = ens_hmc_prepare(e, 1, h);
    if (!rc) rc = ens_hmc_rounds(e, 1, h, [](int) { return SQ_OK; });
    if (rc) return rc;
    ens_advance(e, (unsigned long long)ntraj);  // one count per trajectory
    return SQ_OK;
}

int sq_phi4_ens_hmc_stats(sq_phi4_ens *e, int first, int count, long long *out) {
    return ens_read_rows(e, &sq_phi4_ens::hstat, 4, first, count, out);  // no trajectory yet: zeros
}

int sq_phi4_ens_hmc_reset(sq_phi4_ens *e, int first, int count) {
    return ens_clear_rows(e, &sq_phi4_ens::hstat, 4, first, count);
}

}  // extern "C"

// ---- replica exchange ----
namespace {

// What stands against an exchange round, checked before any device work.
int ens_xchg_state(const sq_phi4_ens *e) {
    if (e->nlad == 0)
        return fail(SQ_E_STATE, "an exchange round needs ladders: call sq_phi4_ens_set_ladder first");
    return ens_needs_noise(e, "an exchange round", "beta = 2 dtau / sig^2 has no value");
}

// Room for nx doubles of records, and with records the labels at the call's start.
int ens_xchg_begin(sq_phi4_ens *e, size_t nx, std::vector<int> &lab) {
    int rc = ens_reserve(e->xrec, nx);
    if (rc || !nx) return rc;
    lab.resize((size_t)e->R);
    SQ_HIP(hipMemcpy(lab.data(), e->walker.data(), sizeof(int) * (size_t)e->R, hipMemcpyDeviceToHost));
    return SQ_OK;
}

// Enqueue round e->xround + i; rec: the call's records are wanted, the round's [R][5] rows of them.
int ens_xchg_enqueue(sq_phi4_ens *e, int i, bool rec) {
    sq::Phi4EnsXchgArgs w{};
    w.stat = e->xstat.data();
    w.walker = e->walker.data();
    w.rec = rec ? e->xrec.data() + 5 * (size_t)i * (size_t)e->R : nullptr;
    w.nlad = e->nlad;
    w.x = e->xround + (unsigned long long)i;
    if (sq::phi4_ens_xchg_pairs(w.nlad, w.x) == 0) return SQ_OK;  // nothing to launch
    SQ_HIP(sq::phi4_ens_exchange_launch(ens_args(e), w, e->R, e->stream));
    e->launches++;
    return SQ_OK;
}

// Behind the synchronisation: the rows of the slots without a partner, round by round (verdict -1, partner -1,
// Delta = u = 0 and the label the slot held before the round; lab: the labels at the call's start), the records
// to the caller, and the round counter.
void ens_xchg_end(sq_phi4_ens *e, int nrounds, double *out, std::vector<int> &lab) {
    if (out) {
        double *rec = e->xrec.data();
        for (int i = 0; i < nrounds; ++i) {
            const unsigned long long x = e->xround + (unsigned long long)i;
            const int o = (int)(x & 1ull), np = sq::phi4_ens_xchg_pairs(e->nlad, x);
            for (int r = 0; r < e->R; ++r) {
                double *row = rec + 5 * ((size_t)i * (size_t)e->R + (size_t)r);
                const int pos = r % e->nlad;
                if (pos >= o && pos - o < 2 * np) {
                    lab[(size_t)r] = (int)row[4];
                } else {
                    row[0] = row[1] = 0.0;
                    row[2] = row[3] = -1.0;
                    row[4] = (double)lab[(size_t)r];
                }
            }
        }
        memcpy(out, rec, sizeof(double) * 5 * (size_t)nrounds * (size_t)e->R);
    }
    e->xround += (unsigned long long)nrounds;
}

}  // namespace

extern "C" {

int sq_phi4_ens_set_ladder(sq_phi4_ens *e, int nlad) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (const char *why = sq::ckpt::ladder_error(nlad, e->R)) return fail(SQ_E_ARG, why);
    e->nlad = nlad;
    return SQ_OK;
}

int sq_phi4_ens_get_ladder(sq_phi4_ens *e, int *nlad) {
    if (!e || !nlad) return fail(SQ_E_ARG, "null argument");
    *nlad = e->nlad;
    return SQ_OK;
}

int sq_phi4_ens_exchange_round(sq_phi4_ens *e, unsigned long long *x) {
    if (!e || !x) return fail(SQ_E_ARG, "null argument");
    *x = e->xround;
    return SQ_OK;
}

int sq_phi4_ens_set_exchange_round(sq_phi4_ens *e, unsigned long long x) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    e->xround = x;
    return SQ_OK;
}

int sq_phi4_ens_exchange(sq_phi4_ens *e, int nrounds, double *rec) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nrounds < 0) return fail(SQ_E_ARG, "nrounds must be >= 0");
    int rc = ens_xchg_state(e);
    if (rc || nrounds == 0) return rc;
    DeviceGuard g(e->dev);
    std::vector<int> lab;
    rc = ens_sync_recs(e);
    if (!rc) rc = ens_xchg_begin(e, rec ? (size_t)nrounds * (size_t)e->R * 5 : 0, lab);
    if (rc) return rc;
    for (int i = 0; i < nrounds && !rc; ++i) rc = ens_xchg_enqueue(e, i, rec != nullptr);
    const hipError_t he = hipStreamSynchronize(e->stream);
    if (rc) return rc;
    SQ_HIP(he);
    ens_xchg_end(e, nrounds, rec, lab);
    return SQ_OK;
}

int sq_phi4_ens_step_hmc_exchange(sq_phi4_ens *e, int nrounds, int ntraj, int nleap, int randomize, int every,
                                  double *series, int measure, double *rec_hmc, double *rec_x) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    const EnsHmc h{ntraj, nleap, randomize, every, measure, series, rec_hmc};
    int rc = ens_hmc_fused_check(nrounds, h);
    if (!rc) rc = ens_xchg_state(e);  // the trajectories' C != 0 as well
    if (rc || nrounds == 0) return rc;
    DeviceGuard g(e->dev);
    std::vector<int> lab;
    rc = ens_hmc_prepare(e, nrounds, h);
    if (!rc) rc = ens_xchg_begin(e, rec_x ? (size_t)nrounds * (size_t)e->R * 5 : 0, lab);
    if (!rc) rc = ens_hmc_rounds(e, nrounds, h, [&](int i) { return ens_xchg_enqueue(e, i, rec_x != nullptr); });
    if (rc) return rc;
    ens_xchg_end(e, nrounds, rec_x, lab);
    ens_advance(e, (unsigned long long)nrounds * (unsigned long long)ntraj);  // one count per trajectory
    return SQ_OK;
}

int sq_phi4_ens_exchange_stats(sq_phi4_ens *e, int first, int count, long long *out) {
    return ens_read_rows(e, &sq_phi4_ens::xstat, 2, first, count, out);
}

int sq_phi4_ens_walkers(sq_phi4_ens *e, int first, int count, int *out) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!out) return fail(SQ_E_ARG, "null argument");
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    SQ_HIP(hipMemcpy(out, e->walker.data() + first, sizeof(int) * (size_t)count, hipMemcpyDeviceToHost));
    return SQ_OK;
}

int sq_phi4_ens_exchange_reset(sq_phi4_ens *e, int first, int count, int walkers) {
    if (!walkers) return ens_clear_rows(e, &sq_phi4_ens::xstat, 2, first, count);
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);  // ens_clear_rows, with the labels in front of its synchronisation
    SQ_HIP(hipMemset(e->xstat.data() + 2 * (size_t)first, 0, sizeof(long long) * 2 * (size_t)count));
    std::vector<int> id((size_t)count);
    for (int r = 0; r < count; ++r) id[(size_t)r] = first + r;
    SQ_HIP(hipMemcpy(e->walker.data() + first, id.data(), sizeof(int) * (size_t)count, hipMemcpyHostToDevice));
    SQ_HIP(hipDeviceSynchronize());
    return SQ_OK;
}

int sq_phi4_ens_exchange_shape_info(const int dims[3], int out[4]) {
    int rc = ens_shape_dims(dims, out);
    if (rc) return rc;
    const sq::Phi4EnsShape s = sq::phi4_ens_shape(dims[0] * dims[1] * dims[2]);
    out[0] = s.K;
    out[1] = s.T;
    out[2] = s.lds(sq::kPhi4EnsLdsStored).bytes;
    out[3] = sq::kPhi4EnsLdsBytes;
    return SQ_OK;
}

}  // extern "C"

// ---- Swendsen-Wang cluster sweeps ----
namespace {

// What stands against a cluster sweep, checked before any device work.
int ens_cluster_state(const sq_phi4_ens *e) {
    return ens_needs_noise(e, "a cluster sweep", "beta = 2 dtau / sig^2 has no value");
}

// What a call with the cluster sums returns beside the plain call's records.
struct EnsSums {
    double *series;      // [n][R][8]
    long long *weights;  // [n][R][sites][7], nullable
};

// The device buffers of a call's records: nsweeps sweeps of [R][sites] each, where the caller wants them; x: the
// call takes the cluster sums, with their series, the tables and, where the shape parks its labels, the scratch.
int ens_cluster_bufs(sq_phi4_ens *e, int nsweeps, bool bonds, bool labels, const EnsSums *x) {
    const size_t n = (size_t)nsweeps * (size_t)e->R * e->sites;
    int rc = ens_reserve(e->cbonds, bonds ? n : 0);
    if (!rc) rc = ens_reserve(e->clabels, labels ? n : 0);
    if (rc || !x) return rc;
    rc = ens_reserve(e->cser, 8 * (size_t)nsweeps * (size_t)e->R);
    if (!rc) rc = ens_reserve(e->cweights, x->weights ? 7 * n : 0);
    if (!rc && sq::phi4_ens_cluster_sum_shape((int)e->sites).park) rc = ens_reserve(e->cpark, (size_t)e->R * e->sites);
    if (rc) return rc;
    // an unconverged sweep leaves its rows of the sums unwritten: zeros
    if (x->weights) SQ_HIP(hipMemsetAsync(e->cweights.data(), 0, sizeof(long long) * 7 * n, e->stream));
    if (e->ctab.data()) return SQ_OK;
    const int L[3] = {e->Lx, e->Ly, e->Lz};
    std::vector<double> tab(2 * (size_t)(L[0] + L[1] + L[2]));
    size_t at = 0;
    for (int mu = 0; mu < 3 && !rc; at += 2 * (size_t)L[mu], ++mu)
        rc = sq_phi4_ens_momentum_table(L[mu], 1, &tab[at], &tab[at + (size_t)L[mu]]);
    if (!rc) rc = ens_reserve(e->ctab, tab.size());
    if (rc) return rc;
    SQ_HIP(hipMemcpy(e->ctab.data(), tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
    return SQ_OK;
}

// Enqueue sweep e->csweep + i; bonds, labels: the call records them; x: with the cluster sums.
int ens_cluster_enqueue(sq_phi4_ens *e, int i, bool bonds, bool labels, const EnsSums *x) {
    const size_t per = (size_t)e->R * e->sites;
    sq::Phi4EnsClusterArgs w{};
    w.stat = e->cstat.data();
    w.bonds = bonds ? e->cbonds.data() + per * (size_t)i : nullptr;
    w.labels = labels ? e->clabels.data() + per * (size_t)i : nullptr;
    w.c = e->csweep + (unsigned long long)i;
    hipError_t he;
    if (x) {
        sq::Phi4EnsClusterSumArgs xs{};
        xs.series = e->cser.data() + 8 * (size_t)i * (size_t)e->R;
        xs.weights = x->weights ? e->cweights.data() + 7 * per * (size_t)i : nullptr;
        xs.tab = e->ctab.data();
        xs.park = e->cpark.data();
        he = sq::phi4_ens_cluster_improved_launch(ens_args(e), w, xs, e->R, e->stream);
    } else {
        he = sq::phi4_ens_cluster_launch(ens_args(e), w, e->R, e->stream);
    }
    if (he != hipSuccess) return fail(SQ_E_HIP, std::string("phi4_ens_cluster_launch: ") + hipGetErrorString(he));
    e->launches++;
    return SQ_OK;
}

// Behind the synchronisation: the records of nsweeps sweeps to the caller, and the sweep counter.
int ens_cluster_end(sq_phi4_ens *e, int nsweeps, unsigned char *bonds, int *labels, const EnsSums *x) {
    const size_t n = (size_t)nsweeps * (size_t)e->R * e->sites;
    if (bonds) SQ_HIP(hipMemcpy(bonds, e->cbonds.data(), n, hipMemcpyDeviceToHost));
    if (labels) SQ_HIP(hipMemcpy(labels, e->clabels.data(), sizeof(int) * n, hipMemcpyDeviceToHost));
    if (x) {
        memcpy(x->series, e->cser.data(), sizeof(double) * 8 * (size_t)nsweeps * (size_t)e->R);
        if (x->weights)
            SQ_HIP(hipMemcpy(x->weights, e->cweights.data(), sizeof(long long) * 7 * n, hipMemcpyDeviceToHost));
    }
    e->csweep += (unsigned long long)nsweeps;
    return SQ_OK;
}

// sq_phi4_ens_cluster and, x non-null, its _improved form.
int ens_cluster(sq_phi4_ens *e, int nsweeps, unsigned char *bonds, int *labels, const EnsSums *x) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nsweeps < 0) return fail(SQ_E_ARG, "nsweeps must be >= 0");
    if (x && nsweeps > 0 && !x->series) return fail(SQ_E_ARG, "null argument: the cluster sums need their series");
    int rc = ens_cluster_state(e);
    if (rc || nsweeps == 0) return rc;
    DeviceGuard g(e->dev);
    rc = ens_sync_recs(e);
    if (!rc) rc = ens_cluster_bufs(e, nsweeps, bonds != nullptr, labels != nullptr, x);
    if (rc) return rc;
    for (int i = 0; i < nsweeps && !rc; ++i) rc = ens_cluster_enqueue(e, i, bonds != nullptr, labels != nullptr, x);
    const hipError_t he = hipStreamSynchronize(e->stream);
    if (rc) return rc;
    SQ_HIP(he);
    return ens_cluster_end(e, nsweeps, bonds, labels, x);
}

// sq_phi4_ens_step_hmc_cluster and, x non-null, its _improved form.
int ens_hmc_cluster(sq_phi4_ens *e, int nrounds, const EnsHmc &h, unsigned char *bonds, int *labels,
                    const EnsSums *x) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    int rc = ens_hmc_fused_check(nrounds, h);
    if (!rc && x && nrounds > 0 && !x->series)
        rc = fail(SQ_E_ARG, "null argument: the cluster sums need their series");
    if (!rc) rc = ens_cluster_state(e);  // the trajectories' C != 0 as well
    if (rc || nrounds == 0) return rc;
    DeviceGuard g(e->dev);
    rc = ens_hmc_prepare(e, nrounds, h);
    if (!rc) rc = ens_cluster_bufs(e, nrounds, bonds != nullptr, labels != nullptr, x);
    if (!rc)
        rc = ens_hmc_rounds(e, nrounds, h,
                            [&](int i) { return ens_cluster_enqueue(e, i, bonds != nullptr, labels != nullptr, x); });
    if (!rc) rc = ens_cluster_end(e, nrounds, bonds, labels, x);
    if (rc) return rc;
    ens_advance(e, (unsigned long long)nrounds * (unsigned long long)h.ntraj);  // one count per trajectory
    return SQ_OK;
}

}  // namespace

extern "C" {

int sq_phi4_ens_cluster_sweep(sq_phi4_ens *e, unsigned long long *c) {
    if (!e || !c) return fail(SQ_E_ARG, "null argument");
    *c = e->csweep;
    return SQ_OK;
}

int sq_phi4_ens_set_cluster_sweep(sq_phi4_ens *e, unsigned long long c) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    e->csweep = c;
    return SQ_OK;
}

int sq_phi4_ens_cluster(sq_phi4_ens *e, int nsweeps, unsigned char *bonds, int *labels) {
    return ens_cluster(e, nsweeps, bonds, labels, nullptr);
}

int sq_phi4_ensemble_cluster_improved(sq_phi4_ens *e, int nsweeps, double *series, unsigned char *bonds, int *labels,
                                 long long *weights) {
    const EnsSums x{series, weights};
    return ens_cluster(e, nsweeps, bonds, labels, &x);
}

int sq_phi4_ens_step_hmc_cluster(sq_phi4_ens *e, int nrounds, int ntraj, int nleap, int randomize, int every,
                                 double *series, int measure, double *rec_hmc, unsigned char *bonds, int *labels) {
    const EnsHmc h{ntraj, nleap, randomize, every, measure, series, rec_hmc};
    return ens_hmc_cluster(e, nrounds, h, bonds, labels, nullptr);
}

int sq_phi4_ensemble_step_hmc_cluster_improved(sq_phi4_ens *e, int nrounds, int ntraj, int nleap, int randomize, int every,
                                          double *series, int measure, double *rec_hmc, unsigned char *bonds,
                                          int *labels, double *cseries, long long *weights) {
    const EnsHmc h{ntraj, nleap, randomize, every, measure, series, rec_hmc};
    const EnsSums x{cseries, weights};
    return ens_hmc_cluster(e, nrounds, h, bonds, labels, &x);
}

int sq_phi4_ens_cluster_stats(sq_phi4_ens *e, int first, int count, long long *out) {
    return ens_read_rows(e, &sq_phi4_ens::cstat, 5, first, count, out);
}

int sq_phi4_ens_cluster_reset(sq_phi4_ens *e, int first, int count) {
    return ens_clear_rows(e, &sq_phi4_ens::cstat, 5, first, count);
}

int sq_phi4_ens_cluster_shape_info(const int dims[3], int out[4]) {
    int rc = ens_shape_dims(dims, out);
    if (rc) return rc;
    const sq::Phi4EnsShape s = sq::phi4_ens_shape(dims[0] * dims[1] * dims[2]);
    out[0] = s.K;
    out[1] = s.T;
    out[2] = s.lds(sq::kPhi4EnsLdsStored).bytes;
    out[3] = sq::kPhi4EnsLdsBytes;
    return SQ_OK;
}

int sq_phi4_ensemble_cluster_improved_shape_info(const int dims[3], int out[5]) {
    int rc = ens_shape_dims(dims, out);
    if (rc) return rc;
    const sq::Phi4EnsClusterSumShape s = sq::phi4_ens_cluster_sum_shape(dims[0] * dims[1] * dims[2]);
    out[0] = s.K;
    out[1] = s.T;
    out[2] = s.lds(sq::kPhi4EnsLdsStored, sq::kPhi4EnsClusterSumBytes).bytes;
    out[3] = sq::kPhi4EnsLdsBytes;
    out[4] = s.park;
    return SQ_OK;
}

}  // extern "C"
