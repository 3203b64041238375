// sq_phi4_ens.cpp -- the phi^4 lattice ensemble behind the sq_phi4_ens_* entry
// points of the C ABI: R lattices per launch (sq_phi4_ens.hip).  The host
// keeps every replica's parameters and step counter; the device records hold
// the coefficients derived from them and are rewritten before the next launch
// whenever a setter changed something.  Frames (sq_phi4_ens_run_frames) are
// decided in the kernel; the host mirrors every replica's frame state between
// calls and uploads it before each one.
#include <cmath>
#include <cstring>
#include <vector>

#include "sq_ctx.h"
#include "sq_phi4_ens.h"

using namespace sq;

struct sq_phi4_ens {
    sq_params p{};
    int dev = 0, Lx = 0, Ly = 0, Lz = 0, R = 0;
    size_t sites = 0;
    struct Rep {
        double dtau, m2, lambda, C;
        unsigned long long seed, step;
    };
    std::vector<Rep> rep;                // [R]
    float *field = nullptr;              // [R][Lz][Ly][Lx]
    sq::Phi4EnsRec *rec = nullptr;       // [R]
    int *flags = nullptr;                // [R]
    double *series = nullptr;            // the last step call's records: pinned host memory the kernel writes
    size_t series_cap = 0;               // ... in doubles
    double *mom = nullptr;               // [R][5]
    bool rec_dirty = true;               // the device records are behind rep[]
    std::vector<sq::Phi4EnsFrameState> fst;  // [R] frame state, current between calls
    sq::Phi4EnsFrameState *fst_dev = nullptr;
    float *frecs = nullptr;              // [R][3][loops] the last frame's records (first frames call on)
    int *fr_stable = nullptr;            // [fr_cap][R] a frames call's verdicts ...
    double *fr_dtau = nullptr;           // ... and Δτ
    size_t fr_cap = 0;                   // ... in frames
    unsigned long long adv = 0;          // steps run since the records were written
    int nt = 0;                          // Lz / 2 + 1 correlator distances
    double *cG = nullptr;                // [R][nt] correlator accumulators: zero at creation, cleared by
    double *cS1 = nullptr;               // [R]     sq_phi4_ens_corr_reset only
    long long *cN = nullptr;             // [R]
    double *ctmp = nullptr;              // sq_phi4_ens_slices' device buffer: [count][Lz] then [count][nt]
    size_t ctmp_cap = 0;                 // ... in replicas
    int pM = 0;                          // momenta set (sq_phi4_ens_set_momenta), 0 .. SQ_PHI4_ENS_MAX_MOMENTA
    int pn[2 * SQ_PHI4_ENS_MAX_MOMENTA] = {};  // their (nx, ny)
    double *ptab = nullptr;              // twiddle tables: cx | sx [8][Lx], cy | sy [8][Ly] (first set_momenta on)
    double *pG = nullptr;                // [R][pM][nt] momentum accumulators: zeroed by set_momenta and
    long long *pN = nullptr;             // [R]         sq_phi4_ens_pcorr_reset only
    size_t pG_cap = 0;                   // ... in momenta
    double *ptmp = nullptr;              // sq_phi4_ens_pslices' device buffer: [count][pM][Lz][2] then [count][pM][nt]
    size_t ptmp_cap = 0;                 // ... in doubles
    int fF = 0;                          // flow levels set (sq_phi4_ens_set_flow), 0: no flow
    int flev[SQ_PHI4_ENS_MAX_FLOW_LEVELS] = {};  // ... strictly ascending flow steps
    double feps = 0.0, fm2 = NAN, flam = NAN;    // flow step; the flow's m², λ (NaN: each replica's own)
    sq::Phi4EnsFlowRec *frec = nullptr;  // [R] flow coefficients (first set_flow on)
    bool frec_dirty = true;              // ... are behind rep[] / the flow parameters
    double *fG = nullptr;                // [R][fF][nt] flow accumulators: zeroed by set_flow and
    double *fS1 = nullptr;               // [R][fF]     sq_phi4_ens_fcorr_reset only
    long long *fN = nullptr;             // [R][fF]
    size_t fG_cap = 0;                   // ... in levels
    double *ftmp = nullptr;              // sq_phi4_ens_flowed's / _flow_field's device buffer
    size_t ftmp_cap = 0;                 // ... in bytes
    long long *mstat = nullptr;          // [R][3] MALA counters: proposed, accepted, guard trips (first MALA call on);
                                         // cleared by sq_phi4_ens_mala_reset only
    double *mrec = nullptr;              // the last MALA call's per-step records: pinned host memory the kernel writes
    size_t mrec_cap = 0;                 // ... in doubles
    long long *hstat = nullptr;          // [R][4] HMC counters: trajectories, accepted, guard trips, leapfrog steps
                                         // (first HMC call on); cleared by sq_phi4_ens_hmc_reset only
    double *hrec = nullptr;              // the last HMC call's per-trajectory records: pinned host memory
    size_t hrec_cap = 0;                 // ... in doubles
    int nlad = 0;                        // slots per exchange ladder (sq_phi4_ens_set_ladder), 0: no ladders
    unsigned long long xround = 0;       // the exchange-round counter
    long long *xstat = nullptr;          // [R][2] attempts, acceptances of the pair (r, r + 1); zero at creation,
                                         // cleared by sq_phi4_ens_exchange_reset only
    int *walker = nullptr;               // [R] the label of the field each slot holds; r at creation
    double *xrec = nullptr;              // the last exchange call's records: pinned host memory the kernel writes
    size_t xrec_cap = 0;                 // ... in doubles
    unsigned long long csweep = 0;       // the cluster-sweep counter
    long long *cstat = nullptr;          // [R][5] sweeps, clusters, flipped clusters, flipped sites, unconverged
                                         // sweeps; zero at creation, cleared by sq_phi4_ens_cluster_reset only
    unsigned char *cbonds = nullptr;     // the last cluster call's bond records: device memory, read back once
    size_t cbonds_cap = 0;               // ... in bytes
    int *clabels = nullptr;              // ... and its label records
    size_t clabels_cap = 0;              // ... in ints
    hipStream_t stream = nullptr;
    long long steps_total = 0, launches = 0;
};

namespace {

int ens_range(const sq_phi4_ens *e, int first, int count) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (first < 0 || count < 0 || first > e->R || count > e->R - first)
        return fail(SQ_E_ARG, "replica range outside [0, nrep)");
    return SQ_OK;
}

// What is wrong with a lattice shape, nullptr for a legal one (sq_phi4_ens_create, sq_phi4_ens_shape_info).
const char *ens_dims_error(long long Lx, long long Ly, long long Lz) {
    if (Lx != 8 && Lx != 16 && Lx != 32 && Lx != 64) return "a phi^4 ensemble needs Lx in {8, 16, 32, 64}";
    if (Ly < 2 || Lz < 2) return "a phi^4 ensemble needs Ly >= 2 and Lz >= 2";
    if (Ly > sq::kPhi4EnsMaxSites || Lz > sq::kPhi4EnsMaxSites || Lx * Ly * Lz > sq::kPhi4EnsMaxSites)
        return "a phi^4 ensemble needs Lx Ly Lz <= 32768 sites (one LDS image per lattice)";
    return nullptr;
}

// create_phi4's parameter bound, per replica (the guard needs every update of a
// field inside [-clamp, clamp] to be finite or an infinity, never NaN)
bool ens_params_ok(double cl, double h, double m2, double lambda, double C) {
    const double drift = 12.0 * cl + std::fabs(m2) * cl + std::fabs(lambda) / 6.0 * cl * cl * cl;
    const float clf = (float)cl;
    return std::isfinite(cl) && cl > 0 && std::isfinite(m2) && std::isfinite(lambda) && std::isfinite(C) &&
           std::isfinite(h) && h > 0 && std::isfinite(clf * clf) &&
           h * drift + cl + 16.0 * sqrt(2.0 * h) * std::fabs(C) < 1e30;
}

// phi4_base_args' coefficients (sq_phi4_steps.cpp)
sq::Phi4EnsRec ens_rec(const sq_phi4_ens::Rep &r) {
    sq::Phi4EnsRec d{};
    const float h = (float)r.dtau;
    d.h = h;
    d.m2 = (float)r.m2;
    d.lam6 = (float)((double)(float)r.lambda / 6.0);
    d.sig = (float)(sqrt(2.0 * (double)h) * r.C);
    d.sigq = (float)(sqrt(2.0 * (double)h) * r.C * sq::kSqrt2Ln2);
    d.k0 = (uint32_t)r.seed;
    d.k1 = (uint32_t)(r.seed >> 32);
    d.step = r.step;
    return d;
}

// Bring the device records up to rep[] (the stream is idle: every entry point synchronises it).
int ens_sync_recs(sq_phi4_ens *e) {
    if (!e->rec_dirty) return SQ_OK;
    std::vector<sq::Phi4EnsRec> h((size_t)e->R);
    for (int r = 0; r < e->R; ++r) h[r] = ens_rec(e->rep[r]);
    SQ_HIP(hipMemcpy(e->rec, h.data(), sizeof(sq::Phi4EnsRec) * h.size(), hipMemcpyHostToDevice));
    e->rec_dirty = false;
    e->adv = 0;
    return SQ_OK;
}

sq::Phi4EnsArgs ens_args(const sq_phi4_ens *e) {
    sq::Phi4EnsArgs a{};
    a.field = e->field;
    a.rec = e->rec;
    a.flags = e->flags;
    a.Lx = e->Lx;
    a.Ly = e->Ly;
    a.Lz = e->Lz;
    a.clampv = (float)e->p.clamp;
    a.adv = e->adv;
    return a;
}

void release_phi4_ens(sq_phi4_ens *e) {
    if (e->stream) {
        (void)hipStreamSynchronize(e->stream);
        (void)hipStreamDestroy(e->stream);
        e->stream = nullptr;
    }
    (void)hipFree(e->field);
    (void)hipFree(e->rec);
    (void)hipFree(e->flags);
    (void)hipHostFree(e->series);
    (void)hipFree(e->mom);
    (void)hipFree(e->fst_dev);
    (void)hipFree(e->frecs);
    (void)hipFree(e->fr_stable);
    (void)hipFree(e->fr_dtau);
    (void)hipFree(e->cG);
    (void)hipFree(e->cS1);
    (void)hipFree(e->cN);
    (void)hipFree(e->ctmp);
    (void)hipFree(e->ptab);
    (void)hipFree(e->pG);
    (void)hipFree(e->pN);
    (void)hipFree(e->ptmp);
    (void)hipFree(e->frec);
    (void)hipFree(e->fG);
    (void)hipFree(e->fS1);
    (void)hipFree(e->fN);
    (void)hipFree(e->ftmp);
    (void)hipFree(e->mstat);
    (void)hipHostFree(e->mrec);
    e->mstat = nullptr;
    e->mrec = nullptr;
    e->mrec_cap = 0;
    (void)hipFree(e->hstat);
    (void)hipHostFree(e->hrec);
    e->hstat = nullptr;
    e->hrec = nullptr;
    e->hrec_cap = 0;
    (void)hipFree(e->xstat);
    (void)hipFree(e->walker);
    (void)hipHostFree(e->xrec);
    e->xstat = nullptr;
    e->walker = nullptr;
    e->xrec = nullptr;
    e->xrec_cap = 0;
    (void)hipFree(e->cstat);
    (void)hipFree(e->cbonds);
    (void)hipFree(e->clabels);
    e->cstat = nullptr;
    e->cbonds = nullptr;
    e->clabels = nullptr;
    e->cbonds_cap = e->clabels_cap = 0;
    e->frec = nullptr;
    e->fG = e->fS1 = e->ftmp = nullptr;
    e->fN = nullptr;
    e->fG_cap = e->ftmp_cap = 0;
    e->ptab = e->pG = e->ptmp = nullptr;
    e->pN = nullptr;
    e->pG_cap = e->ptmp_cap = 0;
    e->cG = e->cS1 = e->ctmp = nullptr;
    e->cN = nullptr;
    e->ctmp_cap = 0;
    e->fst_dev = nullptr;
    e->frecs = nullptr;
    e->fr_stable = nullptr;
    e->fr_dtau = nullptr;
    e->fr_cap = 0;
    e->field = nullptr;
    e->rec = nullptr;
    e->flags = nullptr;
    e->series = e->mom = nullptr;
    e->series_cap = 0;
}

sq::Phi4EnsCorrArgs ens_corr_args(const sq_phi4_ens *e) {
    sq::Phi4EnsCorrArgs c{};
    c.G = e->cG;
    c.S1 = e->cS1;
    c.nmeas = e->cN;
    return c;
}

// The handle's momenta for a launch; corr: the zero-momentum accumulators advance as well.
sq::Phi4EnsPCorrArgs ens_pcorr_args(const sq_phi4_ens *e, bool corr) {
    sq::Phi4EnsPCorrArgs p{};
    const size_t nx = (size_t)SQ_PHI4_ENS_MAX_MOMENTA * (size_t)e->Lx, ny = (size_t)SQ_PHI4_ENS_MAX_MOMENTA * (size_t)e->Ly;
    p.Gp = e->pG;
    p.nmeas_p = e->pN;
    p.cx = e->ptab;
    p.sx = e->ptab + nx;
    p.cy = e->ptab + 2 * nx;
    p.sy = e->ptab + 2 * nx + ny;
    p.M = e->pM;
    if (corr) p.corr = ens_corr_args(e);
    return p;
}

// sq_phi4_ens_step (corr = false), sq_phi4_ens_step_corr (corr = true) and sq_phi4_ens_step_pcorr (pcorr = true,
// corr its `correlate`); with either measurement every >= 1, checked by the caller.  heun: the same call with
// the Heun kernel (sq_phi4_ens_step_heun); one Heun step counts as one step everywhere on the host.
int ens_step(sq_phi4_ens *e, int nsteps, int every, double *series, bool corr, bool pcorr = false,
             bool heun = false) {
    if (nsteps == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    int rc = ens_sync_recs(e);
    if (rc) return rc;
    const size_t nrec = (every > 0 && series) ? (size_t)(nsteps / every) : 0;
    const size_t nd = nrec * (size_t)e->R * 4;
    if (nd > e->series_cap) {
        // the records go straight to pinned host memory (32 B per replica and record, posted writes), visible
        // once the stream is idle: a device buffer and its copy back cost a fixed 15-20 us per call (a 200-step
        // call of one 8^3 lattice with every = 20: 24 % over every = 0 with the copy, 13 % without)
        (void)hipHostFree(e->series);
        e->series = nullptr;
        e->series_cap = 0;
        SQ_HIP(hipHostMalloc(&e->series, sizeof(double) * nd, hipHostMallocDefault));
        e->series_cap = nd;
    }
    sq::Phi4EnsArgs a = ens_args(e);
    a.nsteps = nsteps;
    a.every = (nd || corr || pcorr) ? every : 0;
    a.series = nd ? e->series : nullptr;
    if (heun) {
        const sq::Phi4EnsCorrArgs c = ens_corr_args(e);
        const sq::Phi4EnsPCorrArgs p = pcorr ? ens_pcorr_args(e, corr) : sq::Phi4EnsPCorrArgs{};
        SQ_HIP(sq::phi4_ens_heun_launch(a, (corr && !pcorr) ? &c : nullptr, pcorr ? &p : nullptr, e->R, e->stream));
    } else if (pcorr) SQ_HIP(sq::phi4_ens_step_pcorr_launch(a, ens_pcorr_args(e, corr), e->R, e->stream));
    else if (corr) SQ_HIP(sq::phi4_ens_step_corr_launch(a, ens_corr_args(e), e->R, e->stream));
    else SQ_HIP(sq::phi4_ens_step_launch(a, e->R, e->stream));
    e->launches++;
    SQ_HIP(hipStreamSynchronize(e->stream));
    if (nd) memcpy(series, e->series, sizeof(double) * nd);
    e->adv += (unsigned long long)nsteps;
    for (auto &r : e->rep) r.step += (unsigned long long)nsteps;
    e->steps_total += (long long)nsteps * e->R;
    return SQ_OK;
}

}  // namespace

extern "C" {

int sq_phi4_ens_create(const sq_params *p, int nrep, const unsigned long long *seeds, sq_phi4_ens **out) {
    if (!p || !out) return fail(SQ_E_ARG, "null argument");
    *out = nullptr;
    if (p->struct_size != (int)sizeof(sq_params)) return fail(SQ_E_ARG, "sq_params size mismatch");
    if (p->model != SQ_MODEL_PHI4) return fail(SQ_E_ARG, "a phi^4 ensemble needs SQ_MODEL_PHI4");
    if (p->comm != SQ_COMM_NONE) return fail(SQ_E_ARG, "a phi^4 ensemble needs SQ_COMM_NONE");
    const long long Lx = p->dims[0], Ly = p->dims[1], Lz = p->dims[2];
    if (const char *why = ens_dims_error(Lx, Ly, Lz)) return fail(SQ_E_ARG, why);
    if (nrep < 1) return fail(SQ_E_ARG, "nrep must be >= 1");
    if (!ens_params_ok(p->clamp, p->deltatau, p->m2, p->lambda, p->C))
        return fail(SQ_E_ARG, "PHI4 parameters must be finite with dtau > 0, clamp^2 finite in fp32 and "
                              "dtau * drift(clamp) < 1e30");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SQ_E_NODEV, "no HIP device");
    if (p->device < 0 || p->device >= ndev) return fail(SQ_E_ARG, "device ordinal out of range");
    DeviceGuard g(p->device);
    sq_phi4_ens *e = new sq_phi4_ens();
    e->p = *p;
    e->dev = p->device;
    e->Lx = (int)Lx;
    e->Ly = (int)Ly;
    e->Lz = (int)Lz;
    e->R = nrep;
    e->sites = (size_t)(Lx * Ly * Lz);
    e->rep.resize((size_t)nrep);
    e->fst.assign((size_t)nrep, sq::Phi4EnsFrameState{});
    for (auto &f : e->fst) f.fired = -1;
    for (int r = 0; r < nrep; ++r)
        e->rep[r] = sq_phi4_ens::Rep{p->deltatau, p->m2, p->lambda, p->C,
                                     seeds ? seeds[r] : p->seed + (unsigned long long)r, 0ull};
    int rc = [&]() -> int {
        const size_t bytes = sizeof(float) * e->sites * (size_t)nrep;
        SQ_HIP(hipMalloc(&e->field, bytes));
        SQ_HIP(hipMalloc(&e->rec, sizeof(sq::Phi4EnsRec) * (size_t)nrep));
        SQ_HIP(hipMalloc(&e->flags, sizeof(int) * (size_t)nrep));
        SQ_HIP(hipMalloc(&e->mom, sizeof(double) * 5 * (size_t)nrep));
        SQ_HIP(hipMalloc(&e->fst_dev, sizeof(sq::Phi4EnsFrameState) * (size_t)nrep));
        e->nt = e->Lz / 2 + 1;
        SQ_HIP(hipMalloc(&e->cG, sizeof(double) * (size_t)e->nt * (size_t)nrep));
        SQ_HIP(hipMalloc(&e->cS1, sizeof(double) * (size_t)nrep));
        SQ_HIP(hipMalloc(&e->cN, sizeof(long long) * (size_t)nrep));
        SQ_HIP(hipMemset(e->cG, 0, sizeof(double) * (size_t)e->nt * (size_t)nrep));
        SQ_HIP(hipMemset(e->cS1, 0, sizeof(double) * (size_t)nrep));
        SQ_HIP(hipMemset(e->cN, 0, sizeof(long long) * (size_t)nrep));
        SQ_HIP(hipMalloc(&e->pN, sizeof(long long) * (size_t)nrep));
        SQ_HIP(hipMemset(e->pN, 0, sizeof(long long) * (size_t)nrep));
        SQ_HIP(hipMalloc(&e->xstat, sizeof(long long) * 2 * (size_t)nrep));
        SQ_HIP(hipMemset(e->xstat, 0, sizeof(long long) * 2 * (size_t)nrep));
        SQ_HIP(hipMalloc(&e->cstat, sizeof(long long) * 5 * (size_t)nrep));
        SQ_HIP(hipMemset(e->cstat, 0, sizeof(long long) * 5 * (size_t)nrep));
        SQ_HIP(hipMalloc(&e->walker, sizeof(int) * (size_t)nrep));
        {
            std::vector<int> id((size_t)nrep);
            for (int r = 0; r < nrep; ++r) id[(size_t)r] = r;
            SQ_HIP(hipMemcpy(e->walker, id.data(), sizeof(int) * (size_t)nrep, hipMemcpyHostToDevice));
        }
        SQ_HIP(hipMemset(e->field, 0, bytes));
        SQ_HIP(hipMemset(e->flags, 0, sizeof(int) * (size_t)nrep));
        SQ_HIP(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
        SQ_HIP(hipDeviceSynchronize());  // the set-up memsets ran on the null stream
        return ens_sync_recs(e);
    }();
    if (rc) {
        const std::string msg = sq_last_error();
        sq_phi4_ens_destroy(e);
        return fail(rc, msg);
    }
    *out = e;
    return SQ_OK;
}

int sq_phi4_ens_shape_info(const int dims[3], int out[8]) {
    if (!dims || !out) return fail(SQ_E_ARG, "null argument");
    if (const char *why = ens_dims_error(dims[0], dims[1], dims[2])) return fail(SQ_E_ARG, why);
    const sq::Phi4EnsShape s = sq::phi4_ens_shape(dims[0] * dims[1] * dims[2]);
    out[0] = s.K;
    out[1] = s.T;
    out[2] = s.two ? 2 : 1;
    out[3] = s.lds_bytes;
    out[4] = s.fr_two ? 2 : 1;
    out[5] = s.fr_lds_bytes;
    out[6] = s.mom_lds_bytes;
    out[7] = sq::kPhi4EnsLdsBytes;
    return SQ_OK;
}

int sq_phi4_ens_destroy(sq_phi4_ens *e) {
    if (!e) return SQ_OK;
    DeviceGuard g(e->dev);
    release_phi4_ens(e);
    delete e;
    return SQ_OK;
}

int sq_phi4_ens_upload(sq_phi4_ens *e, int first, int count, const float *phi) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!phi) return fail(SQ_E_ARG, "null argument");
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    SQ_HIP(hipMemcpy(e->field + (size_t)first * e->sites, phi, sizeof(float) * (size_t)count * e->sites,
                     hipMemcpyHostToDevice));
    return SQ_OK;
}

int sq_phi4_ens_download(sq_phi4_ens *e, int first, int count, float *phi) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!phi) return fail(SQ_E_ARG, "null argument");
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    SQ_HIP(hipMemcpy(phi, e->field + (size_t)first * e->sites, sizeof(float) * (size_t)count * e->sites,
                     hipMemcpyDeviceToHost));
    return SQ_OK;
}

int sq_phi4_ens_init_field(sq_phi4_ens *e, float amp) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    DeviceGuard g(e->dev);
    int rc = ens_sync_recs(e);
    if (rc) return rc;
    SQ_HIP(sq::phi4_ens_init_launch(ens_args(e), e->R, amp, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_set_params(sq_phi4_ens *e, int first, int count, const double *dtau, const double *m2,
                           const double *lambda, const double *C) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    for (int r = 0; r < count; ++r) {  // all of the range or none of it
        const sq_phi4_ens::Rep &o = e->rep[(size_t)(first + r)];
        if (!ens_params_ok(e->p.clamp, dtau ? dtau[r] : o.dtau, m2 ? m2[r] : o.m2, lambda ? lambda[r] : o.lambda,
                           C ? C[r] : o.C))
            return fail(SQ_E_ARG, "PHI4 parameters must be finite with dtau > 0 and dtau * drift(clamp) < 1e30");
        // the replica's flow coefficients follow its m² and λ where the flow has none of its own
        if (e->fF > 0 && !ens_params_ok(e->p.clamp, e->feps, std::isnan(e->fm2) ? (m2 ? m2[r] : o.m2) : e->fm2,
                                        std::isnan(e->flam) ? (lambda ? lambda[r] : o.lambda) : e->flam, 0.0))
            return fail(SQ_E_ARG, "the parameters would make the replica's flow coefficients illegal "
                                  "(sq_phi4_ens_set_flow)");
    }
    for (int r = 0; r < count; ++r) {
        sq_phi4_ens::Rep &o = e->rep[(size_t)(first + r)];
        if (dtau) o.dtau = dtau[r];
        if (m2) o.m2 = m2[r];
        if (lambda) o.lambda = lambda[r];
        if (C) o.C = C[r];
    }
    if (count && (dtau || m2 || lambda || C)) e->rec_dirty = true;
    if (count && (m2 || lambda)) e->frec_dirty = true;
    return SQ_OK;
}

int sq_phi4_ens_get_params(sq_phi4_ens *e, int first, int count, double *dtau, double *m2, double *lambda,
                           double *C) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    for (int r = 0; r < count; ++r) {
        const sq_phi4_ens::Rep &o = e->rep[(size_t)(first + r)];
        if (dtau) dtau[r] = o.dtau;
        if (m2) m2[r] = o.m2;
        if (lambda) lambda[r] = o.lambda;
        if (C) C[r] = o.C;
    }
    return SQ_OK;
}

int sq_phi4_ens_get_step(sq_phi4_ens *e, int first, int count, unsigned long long *step) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!step) return fail(SQ_E_ARG, "null argument");
    for (int r = 0; r < count; ++r) step[r] = e->rep[(size_t)(first + r)].step;
    return SQ_OK;
}

int sq_phi4_ens_set_step(sq_phi4_ens *e, int first, int count, const unsigned long long *step) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!step) return fail(SQ_E_ARG, "null argument");
    for (int r = 0; r < count; ++r) e->rep[(size_t)(first + r)].step = step[r];
    if (count) e->rec_dirty = true;
    return SQ_OK;
}

int sq_phi4_ens_step(sq_phi4_ens *e, int nsteps, int every, double *series) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nsteps < 0) return fail(SQ_E_ARG, "nsteps must be >= 0");
    if (every < 0) return fail(SQ_E_ARG, "every must be >= 0");
    return ens_step(e, nsteps, every, series, false);
}

int sq_phi4_ens_step_corr(sq_phi4_ens *e, int nsteps, int every, double *series) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nsteps < 0) return fail(SQ_E_ARG, "nsteps must be >= 0");
    if (every < 1) return fail(SQ_E_ARG, "a correlator measurement needs every >= 1");
    return ens_step(e, nsteps, every, series, true);
}

namespace {
int ens_run_frames(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series, bool corr,
                   bool pcorr = false, bool heun = false, bool flow = false);
int ens_sync_flow(sq_phi4_ens *e);
sq::Phi4EnsFlowArgs ens_flow_args(const sq_phi4_ens *e);
}

int sq_phi4_ens_run_frames(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series) {
    return ens_run_frames(e, nframes, stable, dtau, series, false);
}

int sq_phi4_ens_run_frames_corr(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series) {
    return ens_run_frames(e, nframes, stable, dtau, series, true);
}

}  // extern "C"

namespace {

// heun: the same call with the Heun frames kernel (sq_phi4_ens_run_frames_heun); one Heun step counts as one
// step everywhere on the host.  flow (sq_phi4_ens_run_frames_flow; a flow is set, series or corr given, no
// pcorr): the flow launch of the scheme, series [nframes][F][R][4], corr the flow accumulators'.
int ens_run_frames(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series, bool corr, bool pcorr,
                   bool heun, bool flow) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nframes < 0) return fail(SQ_E_ARG, "nframes < 0");
    if (e->p.loops < 1) return fail(SQ_E_ARG, "frames need loops >= 1");
    if (pcorr && e->pM == 0) return fail(SQ_E_STATE, "no momenta set (sq_phi4_ens_set_momenta)");
    if (nframes == 0) return SQ_OK;
    if (!stable || !dtau) return fail(SQ_E_ARG, "null argument");
    DeviceGuard g(e->dev);
    const int L = e->p.loops;
    const size_t R = (size_t)e->R, n = (size_t)nframes;
    int rc = ens_sync_recs(e);
    if (!rc && flow) rc = ens_sync_flow(e);
    if (rc) return rc;
    if (!e->frecs) {
        SQ_HIP(hipMalloc(&e->frecs, sizeof(float) * 3 * (size_t)L * R));
        SQ_HIP(hipMemset(e->frecs, 0, sizeof(float) * 3 * (size_t)L * R));
        SQ_HIP(hipDeviceSynchronize());  // the memset ran on the null stream
    }
    if (n > e->fr_cap) {
        (void)hipFree(e->fr_stable);
        (void)hipFree(e->fr_dtau);
        e->fr_stable = nullptr;
        e->fr_dtau = nullptr;
        e->fr_cap = 0;
        SQ_HIP(hipMalloc(&e->fr_stable, sizeof(int) * n * R));
        SQ_HIP(hipMalloc(&e->fr_dtau, sizeof(double) * n * R));
        e->fr_cap = n;
    }
    const size_t nd = series ? n * (flow ? (size_t)e->fF : 1) * R * 4 : 0;
    if (nd > e->series_cap) {  // pinned, written by the kernel (sq_phi4_ens_step)
        (void)hipHostFree(e->series);
        e->series = nullptr;
        e->series_cap = 0;
        SQ_HIP(hipHostMalloc(&e->series, sizeof(double) * nd, hipHostMallocDefault));
        e->series_cap = nd;
    }
    for (size_t r = 0; r < R; ++r) {  // a setter may have changed them since the last call
        e->fst[r].dtau = e->rep[r].dtau;
        e->fst[r].C = e->rep[r].C;
    }
    SQ_HIP(hipMemcpyAsync(e->fst_dev, e->fst.data(), sizeof(sq::Phi4EnsFrameState) * R, hipMemcpyHostToDevice,
                          e->stream));
    sq::Phi4EnsArgs a = ens_args(e);
    a.series = nd ? e->series : nullptr;
    sq::Phi4EnsFrameArgs f{};
    f.st = e->fst_dev;
    f.stable = e->fr_stable;
    f.dtau = e->fr_dtau;
    f.recs = e->frecs;
    f.nframes = nframes;
    f.loops = L;
    f.adapt = e->p.adapt_dtau ? 1 : 0;
    if (flow) {
        SQ_HIP(sq::phi4_ens_frames_flow_launch(a, f, ens_flow_args(e), corr, heun, e->R, e->stream));
    } else if (heun) {
        const sq::Phi4EnsCorrArgs c = ens_corr_args(e);
        const sq::Phi4EnsPCorrArgs p = pcorr ? ens_pcorr_args(e, corr) : sq::Phi4EnsPCorrArgs{};
        SQ_HIP(sq::phi4_ens_heun_frames_launch(a, f, (corr && !pcorr) ? &c : nullptr, pcorr ? &p : nullptr, e->R,
                                               e->stream));
    } else if (pcorr) SQ_HIP(sq::phi4_ens_frames_pcorr_launch(a, f, ens_pcorr_args(e, corr), e->R, e->stream));
    else if (corr) SQ_HIP(sq::phi4_ens_frames_corr_launch(a, f, ens_corr_args(e), e->R, e->stream));
    else SQ_HIP(sq::phi4_ens_frames_launch(a, f, e->R, e->stream));
    e->launches++;
    SQ_HIP(hipMemcpyAsync(e->fst.data(), e->fst_dev, sizeof(sq::Phi4EnsFrameState) * R, hipMemcpyDeviceToHost,
                          e->stream));
    SQ_HIP(hipMemcpyAsync(stable, e->fr_stable, sizeof(int) * n * R, hipMemcpyDeviceToHost, e->stream));
    SQ_HIP(hipMemcpyAsync(dtau, e->fr_dtau, sizeof(double) * n * R, hipMemcpyDeviceToHost, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    if (nd) memcpy(series, e->series, sizeof(double) * nd);
    for (size_t r = 0; r < R; ++r) {
        e->rep[r].dtau = e->fst[r].dtau;
        e->rep[r].step += (unsigned long long)nframes * (unsigned long long)L;  // rolled-back frames too
        e->steps_total += e->fst[r].exec;
    }
    e->rec_dirty = true;  // Δτ and the counters moved
    return SQ_OK;
}

// Replica statistics of one accumulator row (sq_phi4_ens_correlator, sq_phi4_ens_pcorrelator): replica r's
// entries at G[r * stride + t], t < n; the u replicas with N[r] > 0 in index order; S1 non-null: the connected
// form.  err nullable.
void ens_replica_stats(const sq_phi4_ens *e, const double *G, size_t stride, const double *S1, const long long *N,
                       int u, int n, double *mean, double *err) {
    const size_t R = (size_t)e->R;
    const double V = (double)e->sites, Lz = (double)e->Lz;
    std::vector<double> c((size_t)u);
    for (int t = 0; t < n; ++t) {
        size_t k = 0;
        double sum = 0.0;
        for (size_t r = 0; r < R; ++r) {
            if (N[r] <= 0) continue;
            const double nm = (double)N[r];
            double v = G[r * stride + (size_t)t] / (nm * V);
            if (S1) {
                const double sb = S1[r] / nm;
                v -= sb * sb / (Lz * V);
            }
            c[k++] = v;
            sum += v;
        }
        const double m = sum / (double)u;
        mean[t] = m;
        if (err) {
            double q = 0.0;
            for (int i = 0; i < u; ++i) q += (c[(size_t)i] - m) * (c[(size_t)i] - m);
            err[t] = u > 1 ? sqrt(q / ((double)u * (double)(u - 1))) : 0.0;
        }
    }
}

}  // namespace

extern "C" {

int sq_phi4_ens_corr_sums(sq_phi4_ens *e, int first, int count, double *G, double *S1, long long *nmeas) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    const size_t nt = (size_t)e->nt, n = (size_t)count, f = (size_t)first;
    if (G) SQ_HIP(hipMemcpy(G, e->cG + f * nt, sizeof(double) * n * nt, hipMemcpyDeviceToHost));
    if (S1) SQ_HIP(hipMemcpy(S1, e->cS1 + f, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (nmeas) SQ_HIP(hipMemcpy(nmeas, e->cN + f, sizeof(long long) * n, hipMemcpyDeviceToHost));
    return SQ_OK;
}

int sq_phi4_ens_corr_reset(sq_phi4_ens *e, int first, int count) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    const size_t nt = (size_t)e->nt, n = (size_t)count, f = (size_t)first;
    SQ_HIP(hipMemsetAsync(e->cG + f * nt, 0, sizeof(double) * n * nt, e->stream));
    SQ_HIP(hipMemsetAsync(e->cS1 + f, 0, sizeof(double) * n, e->stream));
    SQ_HIP(hipMemsetAsync(e->cN + f, 0, sizeof(long long) * n, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_slices(sq_phi4_ens *e, int first, int count, double *S, double *g) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0 || (!S && !g)) return SQ_OK;
    DeviceGuard dg(e->dev);
    const size_t nt = (size_t)e->nt, Lz = (size_t)e->Lz, n = (size_t)count;
    if (n > e->ctmp_cap) {
        (void)hipFree(e->ctmp);
        e->ctmp = nullptr;
        e->ctmp_cap = 0;
        SQ_HIP(hipMalloc(&e->ctmp, sizeof(double) * n * (Lz + nt)));
        e->ctmp_cap = n;
    }
    double *devS = e->ctmp, *devg = e->ctmp + n * Lz;
    SQ_HIP(sq::phi4_ens_slices_launch(ens_args(e), first, count, devS, devg, e->stream));
    if (S) SQ_HIP(hipMemcpyAsync(S, devS, sizeof(double) * n * Lz, hipMemcpyDeviceToHost, e->stream));
    if (g) SQ_HIP(hipMemcpyAsync(g, devg, sizeof(double) * n * nt, hipMemcpyDeviceToHost, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_correlator(sq_phi4_ens *e, int connected, double *mean, double *err, int n, int *used) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (n < 0 || n > e->nt) return fail(SQ_E_ARG, "n must lie in [0, Lz / 2 + 1]");
    if (!mean && n > 0) return fail(SQ_E_ARG, "null argument");
    const size_t R = (size_t)e->R, nt = (size_t)e->nt;
    std::vector<double> G(R * nt), S1(R);
    std::vector<long long> N(R);
    int rc = sq_phi4_ens_corr_sums(e, 0, e->R, G.data(), S1.data(), N.data());
    if (rc) return rc;
    int u = 0;
    for (size_t r = 0; r < R; ++r) u += N[r] > 0 ? 1 : 0;
    if (used) *used = u;
    if (u == 0) return fail(SQ_E_STATE, "no replica has a correlator measurement");
    ens_replica_stats(e, G.data(), nt, connected ? S1.data() : nullptr, N.data(), u, n, mean, err);
    return SQ_OK;
}

int sq_phi4_ens_momentum_table(int L, int n, double *c, double *s) {
    if (L < 2 || n < 0 || n >= L) return fail(SQ_E_ARG, "a momentum table needs L >= 2 and 0 <= n < L");
    if (!c || !s) return fail(SQ_E_ARG, "null argument");
    for (int k = 0; k < L; ++k) {
        const long long j = ((long long)n * (long long)k) % (long long)L;
        if ((4 * j) % L == 0) {  // a multiple of a quarter turn: exact
            const int q = (int)(4 * j / L);
            c[k] = q == 0 ? 1.0 : (q == 2 ? -1.0 : 0.0);
            s[k] = q == 1 ? 1.0 : (q == 3 ? -1.0 : 0.0);
        } else {
            const double a = 2.0 * M_PI * (double)j / (double)L;
            c[k] = cos(a);
            s[k] = sin(a);
        }
    }
    return SQ_OK;
}

int sq_phi4_ens_set_momenta(sq_phi4_ens *e, int M, const int *nxy) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (M < 0 || M > SQ_PHI4_ENS_MAX_MOMENTA) return fail(SQ_E_ARG, "0 <= M <= SQ_PHI4_ENS_MAX_MOMENTA momenta");
    if (M > 0 && !nxy) return fail(SQ_E_ARG, "null argument");
    for (int m = 0; m < M; ++m)
        if (nxy[2 * m] < 0 || nxy[2 * m] >= e->Lx || nxy[2 * m + 1] < 0 || nxy[2 * m + 1] >= e->Ly)
            return fail(SQ_E_ARG, "a momentum needs 0 <= nx < Lx and 0 <= ny < Ly");
    if (!sq::phi4_ens_shape((int)e->sites, e->Lz).pc_ok)
        return fail(SQ_E_ARG, "the lattice shape leaves no LDS for the momentum projections (16 Lz bytes)");
    DeviceGuard g(e->dev);
    const size_t Lx = (size_t)e->Lx, Ly = (size_t)e->Ly, R = (size_t)e->R, nt = (size_t)e->nt;
    const size_t nx = SQ_PHI4_ENS_MAX_MOMENTA * Lx, ny = SQ_PHI4_ENS_MAX_MOMENTA * Ly;
    if (!e->ptab) SQ_HIP(hipMalloc(&e->ptab, sizeof(double) * 2 * (nx + ny)));
    if ((size_t)M > e->pG_cap) {
        (void)hipFree(e->pG);
        e->pG = nullptr;
        e->pG_cap = 0;
        SQ_HIP(hipMalloc(&e->pG, sizeof(double) * R * (size_t)M * nt));
        e->pG_cap = (size_t)M;
    }
    std::vector<double> tab(2 * (nx + ny), 0.0);
    for (int m = 0; m < M; ++m) {
        int rc = sq_phi4_ens_momentum_table(e->Lx, nxy[2 * m], &tab[(size_t)m * Lx], &tab[nx + (size_t)m * Lx]);
        if (!rc)
            rc = sq_phi4_ens_momentum_table(e->Ly, nxy[2 * m + 1], &tab[2 * nx + (size_t)m * Ly],
                                            &tab[2 * nx + ny + (size_t)m * Ly]);
        if (rc) return rc;
    }
    SQ_HIP(hipMemcpy(e->ptab, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
    e->pM = M;  // the accumulators' layout is [R][M][nt] from here on: all of them start over
    for (int i = 0; i < 2 * M; ++i) e->pn[i] = nxy[i];
    if (M > 0) SQ_HIP(hipMemsetAsync(e->pG, 0, sizeof(double) * R * (size_t)M * nt, e->stream));
    SQ_HIP(hipMemsetAsync(e->pN, 0, sizeof(long long) * R, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_get_momenta(sq_phi4_ens *e, int *M, int *nxy) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (!M) return fail(SQ_E_ARG, "null argument");
    *M = e->pM;
    if (nxy)
        for (int i = 0; i < 2 * e->pM; ++i) nxy[i] = e->pn[i];
    return SQ_OK;
}

int sq_phi4_ens_step_pcorr(sq_phi4_ens *e, int nsteps, int every, double *series, int correlate) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nsteps < 0) return fail(SQ_E_ARG, "nsteps must be >= 0");
    if (every < 1) return fail(SQ_E_ARG, "a momentum measurement needs every >= 1");
    if (e->pM == 0) return fail(SQ_E_STATE, "no momenta set (sq_phi4_ens_set_momenta)");
    return ens_step(e, nsteps, every, series, correlate != 0, true);
}

int sq_phi4_ens_step_heun(sq_phi4_ens *e, int nsteps, int every, double *series, int measure) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nsteps < 0) return fail(SQ_E_ARG, "nsteps must be >= 0");
    if (measure & ~3) return fail(SQ_E_ARG, "measure holds bit 0 (correlator) and bit 1 (momenta) only");
    if (measure ? every < 1 : every < 0)
        return fail(SQ_E_ARG, measure ? "a correlator or momentum measurement needs every >= 1" : "every must be >= 0");
    if ((measure & 2) && e->pM == 0) return fail(SQ_E_STATE, "no momenta set (sq_phi4_ens_set_momenta)");
    return ens_step(e, nsteps, every, series, (measure & 1) != 0, (measure & 2) != 0, true);
}

int sq_phi4_ens_run_frames_pcorr(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series,
                                 int correlate) {
    return ens_run_frames(e, nframes, stable, dtau, series, correlate != 0, true);
}

int sq_phi4_ens_run_frames_heun(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series,
                                int measure) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (measure & ~3) return fail(SQ_E_ARG, "measure holds bit 0 (correlator) and bit 1 (momenta) only");
    return ens_run_frames(e, nframes, stable, dtau, series, (measure & 1) != 0, (measure & 2) != 0, true);
}

int sq_phi4_ens_heun_frames_shape_info(const int dims[3], int out[4]) {
    if (!dims || !out) return fail(SQ_E_ARG, "null argument");
    if (const char *why = ens_dims_error(dims[0], dims[1], dims[2])) return fail(SQ_E_ARG, why);
    const sq::Phi4EnsShape s = sq::phi4_ens_shape(dims[0] * dims[1] * dims[2], dims[2]);
    out[0] = s.fr_two ? 2 : 1;
    out[1] = s.fr_lds_bytes;
    out[2] = s.pc_ok ? 0xf : 0x3;  // bit m: measure = m runs on this shape; momenta need their LDS region
    out[3] = 0;
    return SQ_OK;
}

int sq_phi4_ens_pcorr_sums(sq_phi4_ens *e, int first, int count, double *G, long long *nmeas) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    const size_t row = (size_t)e->pM * (size_t)e->nt, n = (size_t)count, f = (size_t)first;
    if (G && row) SQ_HIP(hipMemcpy(G, e->pG + f * row, sizeof(double) * n * row, hipMemcpyDeviceToHost));
    if (nmeas) SQ_HIP(hipMemcpy(nmeas, e->pN + f, sizeof(long long) * n, hipMemcpyDeviceToHost));
    return SQ_OK;
}

int sq_phi4_ens_pcorr_reset(sq_phi4_ens *e, int first, int count) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    const size_t row = (size_t)e->pM * (size_t)e->nt, n = (size_t)count, f = (size_t)first;
    if (row) SQ_HIP(hipMemsetAsync(e->pG + f * row, 0, sizeof(double) * n * row, e->stream));
    SQ_HIP(hipMemsetAsync(e->pN + f, 0, sizeof(long long) * n, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_pslices(sq_phi4_ens *e, int first, int count, double *AB, double *g) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (e->pM == 0) return fail(SQ_E_STATE, "no momenta set (sq_phi4_ens_set_momenta)");
    if (count == 0 || (!AB && !g)) return SQ_OK;
    DeviceGuard dg(e->dev);
    const size_t nab = (size_t)count * (size_t)e->pM * 2 * (size_t)e->Lz, ng = (size_t)count * (size_t)e->pM * (size_t)e->nt;
    if (nab + ng > e->ptmp_cap) {
        (void)hipFree(e->ptmp);
        e->ptmp = nullptr;
        e->ptmp_cap = 0;
        SQ_HIP(hipMalloc(&e->ptmp, sizeof(double) * (nab + ng)));
        e->ptmp_cap = nab + ng;
    }
    double *devAB = e->ptmp, *devg = e->ptmp + nab;
    SQ_HIP(sq::phi4_ens_pslices_launch(ens_args(e), ens_pcorr_args(e, false), first, count, devAB, devg, e->stream));
    if (AB) SQ_HIP(hipMemcpyAsync(AB, devAB, sizeof(double) * nab, hipMemcpyDeviceToHost, e->stream));
    if (g) SQ_HIP(hipMemcpyAsync(g, devg, sizeof(double) * ng, hipMemcpyDeviceToHost, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_pcorrelator(sq_phi4_ens *e, double *mean, double *err, int n, int *used) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (n < 0 || n > e->nt) return fail(SQ_E_ARG, "n must lie in [0, Lz / 2 + 1]");
    if (!mean && n > 0) return fail(SQ_E_ARG, "null argument");
    if (e->pM == 0) return fail(SQ_E_STATE, "no momenta set (sq_phi4_ens_set_momenta)");
    const size_t R = (size_t)e->R, nt = (size_t)e->nt, M = (size_t)e->pM;
    std::vector<double> G(R * M * nt);
    std::vector<long long> N(R);
    int rc = sq_phi4_ens_pcorr_sums(e, 0, e->R, G.data(), N.data());
    if (rc) return rc;
    int u = 0;
    for (size_t r = 0; r < R; ++r) u += N[r] > 0 ? 1 : 0;
    if (used) *used = u;
    if (u == 0) return fail(SQ_E_STATE, "no replica has a momentum measurement");
    for (size_t m = 0; m < M; ++m)
        ens_replica_stats(e, G.data() + m * nt, M * nt, nullptr, N.data(), u, n, mean + m * (size_t)n,
                          err ? err + m * (size_t)n : nullptr);
    return SQ_OK;
}

int sq_phi4_ens_pcorr_shape_info(const int dims[3], int out[6]) {
    if (!dims || !out) return fail(SQ_E_ARG, "null argument");
    if (const char *why = ens_dims_error(dims[0], dims[1], dims[2])) return fail(SQ_E_ARG, why);
    const sq::Phi4EnsShape s = sq::phi4_ens_shape(dims[0] * dims[1] * dims[2], dims[2]);
    if (!s.pc_ok) return fail(SQ_E_ARG, "the lattice shape leaves no LDS for the momentum projections (16 Lz bytes)");
    out[0] = s.pc_two ? 2 : 1;
    out[1] = s.pc_lds_bytes;
    out[2] = s.pc_fr_two ? 2 : 1;
    out[3] = s.pc_fr_lds_bytes;
    out[4] = s.pc_sl_lds_bytes;
    out[5] = dims[2] / 2 + 1;
    return SQ_OK;
}

int sq_phi4_ens_corr_shape_info(const int dims[3], int out[6]) {
    if (!dims || !out) return fail(SQ_E_ARG, "null argument");
    if (const char *why = ens_dims_error(dims[0], dims[1], dims[2])) return fail(SQ_E_ARG, why);
    const sq::Phi4EnsShape s = sq::phi4_ens_shape(dims[0] * dims[1] * dims[2], dims[2]);
    out[0] = s.co_two ? 2 : 1;
    out[1] = s.co_lds_bytes;
    out[2] = s.co_fr_two ? 2 : 1;
    out[3] = s.co_fr_lds_bytes;
    out[4] = s.sl_lds_bytes;
    out[5] = dims[2] / 2 + 1;
    return SQ_OK;
}

int sq_phi4_ens_stability(sq_phi4_ens *e, int first, int count, double *TV, int *fired, float *M, float *D, float *A,
                          int n) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!M || !D || !A))) return fail(SQ_E_ARG, "bad record arguments");
    if (n > (e->frecs ? e->p.loops : 0)) return fail(SQ_E_ARG, "n exceeds the last frame's steps");
    for (int r = 0; r < count; ++r) {
        const sq::Phi4EnsFrameState &f = e->fst[(size_t)(first + r)];
        if (TV) {
            TV[2 * r] = f.T;
            TV[2 * r + 1] = f.V;
        }
        if (fired) fired[r] = f.fired;
    }
    if (n == 0 || count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    const size_t L = (size_t)e->p.loops;
    std::vector<float> h((size_t)count * 3 * L);
    SQ_HIP(hipMemcpy(h.data(), e->frecs + (size_t)first * 3 * L, sizeof(float) * h.size(), hipMemcpyDeviceToHost));
    float *rows[3] = {M, D, A};
    for (int r = 0; r < count; ++r)
        for (int k = 0; k < 3; ++k)
            memcpy(rows[k] + (size_t)r * (size_t)n, h.data() + ((size_t)r * 3 + (size_t)k) * L, sizeof(float) * (size_t)n);
    return SQ_OK;
}

int sq_phi4_ens_set_stability(sq_phi4_ens *e, int first, int count, const double *T, const double *V) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!T || !V) return fail(SQ_E_ARG, "null argument");
    for (int r = 0; r < count; ++r) {
        sq::Phi4EnsFrameState &f = e->fst[(size_t)(first + r)];
        f.T = (float)T[r];
        f.V = (float)V[r];
        f.init = 1;
    }
    return SQ_OK;
}

int sq_phi4_ens_moments(sq_phi4_ens *e, int first, int count, double *out5) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!out5) return fail(SQ_E_ARG, "null argument");
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    SQ_HIP(sq::phi4_ens_moments_launch(ens_args(e), first, count, e->mom, e->stream));
    SQ_HIP(hipMemcpyAsync(out5, e->mom, sizeof(double) * 5 * (size_t)count, hipMemcpyDeviceToHost, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_flags(sq_phi4_ens *e, int first, int count, int *flags, int clear) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    if (flags) SQ_HIP(hipMemcpy(flags, e->flags + first, sizeof(int) * (size_t)count, hipMemcpyDeviceToHost));
    if (clear) SQ_HIP(hipMemset(e->flags + first, 0, sizeof(int) * (size_t)count));
    if (clear) SQ_HIP(hipDeviceSynchronize());  // the memset ran on the null stream
    return SQ_OK;
}

}  // extern "C"

// ---- gradient-flow measurements (sq_phi4_ens_flow.hip) ----
namespace {

// Replica r's flow coefficients: phi4_base_args' expressions of (eps, m², λ), sig = 0.
sq::Phi4EnsFlowRec ens_flow_rec(const sq_phi4_ens *e, const sq_phi4_ens::Rep &r) {
    sq::Phi4EnsFlowRec d{};
    d.h = (float)e->feps;
    d.m2 = (float)(std::isnan(e->fm2) ? r.m2 : e->fm2);
    d.lam6 = (float)((double)(float)(std::isnan(e->flam) ? r.lambda : e->flam) / 6.0);
    return d;
}

sq::Phi4EnsFlowArgs ens_flow_args(const sq_phi4_ens *e) {
    sq::Phi4EnsFlowArgs w{};
    w.rec = e->frec;
    w.nlev = e->fF;
    for (int l = 0; l < e->fF; ++l) w.lev[l] = e->flev[l];
    w.G = e->fG;
    w.S1 = e->fS1;
    w.nmeas = e->fN;
    return w;
}

// Bring the device's flow records up to rep[] and the flow parameters (the stream is idle).
int ens_sync_flow(sq_phi4_ens *e) {
    if (e->frec && !e->frec_dirty) return SQ_OK;
    if (!e->frec) SQ_HIP(hipMalloc(&e->frec, sizeof(sq::Phi4EnsFlowRec) * (size_t)e->R));
    std::vector<sq::Phi4EnsFlowRec> h((size_t)e->R);
    for (int r = 0; r < e->R; ++r) h[(size_t)r] = ens_flow_rec(e, e->rep[(size_t)r]);
    SQ_HIP(hipMemcpy(e->frec, h.data(), sizeof(sq::Phi4EnsFlowRec) * h.size(), hipMemcpyHostToDevice));
    e->frec_dirty = false;
    return SQ_OK;
}

int ens_flow_tmp(sq_phi4_ens *e, size_t bytes) {
    if (bytes <= e->ftmp_cap) return SQ_OK;
    (void)hipFree(e->ftmp);
    e->ftmp = nullptr;
    e->ftmp_cap = 0;
    SQ_HIP(hipMalloc(&e->ftmp, bytes));
    e->ftmp_cap = bytes;
    return SQ_OK;
}

}  // namespace

extern "C" {

int sq_phi4_ens_set_flow(sq_phi4_ens *e, double eps, int nlevels, const int *levels, const double *m2,
                         const double *lambda) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nlevels < 0 || nlevels > SQ_PHI4_ENS_MAX_FLOW_LEVELS)
        return fail(SQ_E_ARG, "0 <= nlevels <= SQ_PHI4_ENS_MAX_FLOW_LEVELS flow levels");
    DeviceGuard g(e->dev);
    const size_t R = (size_t)e->R, nt = (size_t)e->nt, F = (size_t)nlevels;
    if (nlevels > 0) {
        if (!levels) return fail(SQ_E_ARG, "null argument");
        for (int l = 0; l < nlevels; ++l)
            if (levels[l] < (l ? levels[l - 1] + 1 : 0) || levels[l] > SQ_PHI4_ENS_MAX_FLOW_STEPS)
                return fail(SQ_E_ARG, "flow levels must ascend strictly within [0, SQ_PHI4_ENS_MAX_FLOW_STEPS]");
        const double fm2 = m2 ? *m2 : NAN, flam = lambda ? *lambda : NAN;
        if ((m2 && !std::isfinite(fm2)) || (lambda && !std::isfinite(flam)))
            return fail(SQ_E_ARG, "the flow's m2 and lambda must be finite");
        for (const auto &r : e->rep)  // every replica's flow coefficients or none
            if (!ens_params_ok(e->p.clamp, eps, m2 ? fm2 : r.m2, lambda ? flam : r.lambda, 0.0))
                return fail(SQ_E_ARG, "flow parameters must be finite with eps > 0 and eps * drift(clamp) < 1e30");
        if (F > e->fG_cap) {
            double *G = nullptr, *S1 = nullptr;
            long long *N = nullptr;
            if (hipMalloc(&G, sizeof(double) * R * F * nt) != hipSuccess ||
                hipMalloc(&S1, sizeof(double) * R * F) != hipSuccess ||
                hipMalloc(&N, sizeof(long long) * R * F) != hipSuccess) {
                (void)hipFree(G);
                (void)hipFree(S1);
                (void)hipFree(N);
                return fail(SQ_E_HIP, "hipMalloc of the flow accumulators failed");
            }
            (void)hipFree(e->fG);
            (void)hipFree(e->fS1);
            (void)hipFree(e->fN);
            e->fG = G;
            e->fS1 = S1;
            e->fN = N;
            e->fG_cap = F;
        }
        e->feps = eps;
        e->fm2 = fm2;
        e->flam = flam;
        for (int l = 0; l < nlevels; ++l) e->flev[l] = levels[l];
    }
    e->fF = nlevels;  // the accumulators' layout is [R][F][...] from here on: all of them start over
    e->frec_dirty = true;
    if (F > 0) {
        SQ_HIP(hipMemsetAsync(e->fG, 0, sizeof(double) * R * F * nt, e->stream));
        SQ_HIP(hipMemsetAsync(e->fS1, 0, sizeof(double) * R * F, e->stream));
        SQ_HIP(hipMemsetAsync(e->fN, 0, sizeof(long long) * R * F, e->stream));
        SQ_HIP(hipStreamSynchronize(e->stream));
    }
    return SQ_OK;
}

int sq_phi4_ens_get_flow(sq_phi4_ens *e, double *eps, int *nlevels, int *levels, double *m2, double *lambda) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (!nlevels) return fail(SQ_E_ARG, "null argument");
    *nlevels = e->fF;
    if (eps) *eps = e->fF ? e->feps : 0.0;
    if (levels)
        for (int l = 0; l < e->fF; ++l) levels[l] = e->flev[l];
    if (m2) *m2 = e->fF ? e->fm2 : NAN;
    if (lambda) *lambda = e->fF ? e->flam : NAN;
    return SQ_OK;
}

}  // extern "C"

namespace {
// sq_phi4_ens_step_flow, and with heun sq_phi4_ens_step_flow_heun: the same call with the Heun kernels.
int ens_step_flow(sq_phi4_ens *e, int nsteps, int every, double *series, int correlate, bool heun) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nsteps < 0) return fail(SQ_E_ARG, "nsteps must be >= 0");
    if (every < 1) return fail(SQ_E_ARG, "a flow measurement needs every >= 1");
    if (e->fF == 0) return fail(SQ_E_STATE, "no flow set (sq_phi4_ens_set_flow)");
    if (nsteps == 0) return SQ_OK;
    if (!series && !correlate) return ens_step(e, nsteps, 0, nullptr, false, false, heun);  // nothing to measure
    DeviceGuard g(e->dev);
    int rc = ens_sync_recs(e);
    if (!rc) rc = ens_sync_flow(e);
    if (rc) return rc;
    const size_t nrec = series ? (size_t)(nsteps / every) : 0;
    const size_t nd = nrec * (size_t)e->fF * (size_t)e->R * 4;
    if (nd > e->series_cap) {  // pinned, written by the kernel (ens_step)
        (void)hipHostFree(e->series);
        e->series = nullptr;
        e->series_cap = 0;
        SQ_HIP(hipHostMalloc(&e->series, sizeof(double) * nd, hipHostMallocDefault));
        e->series_cap = nd;
    }
    if (!nd && !correlate) return ens_step(e, nsteps, 0, nullptr, false, false, heun);  // an incomplete tail only
    sq::Phi4EnsArgs a = ens_args(e);
    a.nsteps = nsteps;
    a.every = every;
    a.series = nd ? e->series : nullptr;
    if (heun) SQ_HIP(sq::phi4_ens_heun_flow_launch(a, ens_flow_args(e), correlate != 0, e->R, e->stream));
    else SQ_HIP(sq::phi4_ens_step_flow_launch(a, ens_flow_args(e), correlate != 0, e->R, e->stream));
    e->launches++;
    SQ_HIP(hipStreamSynchronize(e->stream));
    if (nd) memcpy(series, e->series, sizeof(double) * nd);
    e->adv += (unsigned long long)nsteps;
    for (auto &r : e->rep) r.step += (unsigned long long)nsteps;
    e->steps_total += (long long)nsteps * e->R;
    return SQ_OK;
}
}  // namespace

extern "C" {

int sq_phi4_ens_step_flow(sq_phi4_ens *e, int nsteps, int every, double *series, int correlate) {
    return ens_step_flow(e, nsteps, every, series, correlate, false);
}

int sq_phi4_ens_step_flow_heun(sq_phi4_ens *e, int nsteps, int every, double *series, int correlate) {
    return ens_step_flow(e, nsteps, every, series, correlate, true);
}

int sq_phi4_ens_run_frames_flow(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series, int correlate,
                                int scheme) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (scheme != SQ_SCHEME_EULER && scheme != SQ_SCHEME_HEUN)
        return fail(SQ_E_ARG, "scheme must be SQ_SCHEME_EULER or SQ_SCHEME_HEUN");
    if (nframes < 0) return fail(SQ_E_ARG, "nframes < 0");
    if (e->p.loops < 1) return fail(SQ_E_ARG, "frames need loops >= 1");
    if (e->fF == 0) return fail(SQ_E_STATE, "no flow set (sq_phi4_ens_set_flow)");
    const bool heun = scheme == SQ_SCHEME_HEUN;
    if (!series && !correlate) return ens_run_frames(e, nframes, stable, dtau, nullptr, false, false, heun);
    const sq::Phi4EnsFramesFlowShape sh = sq::phi4_ens_frames_flow_shape((int)e->sites, e->Lz);
    if (!((sh.mask >> (2 * (heun ? 1 : 0) + (correlate ? 1 : 0))) & 1))
        return fail(SQ_E_ARG, "the lattice shape has no frames-flow launch of this scheme and correlator choice "
                              "(sq_phi4_ens_frames_flow_shape_info)");
    return ens_run_frames(e, nframes, stable, dtau, series, correlate != 0, false, heun, true);
}

int sq_phi4_ens_frames_flow_shape_info(const int dims[3], int out[8]) {
    if (!dims || !out) return fail(SQ_E_ARG, "null argument");
    if (const char *why = ens_dims_error(dims[0], dims[1], dims[2])) return fail(SQ_E_ARG, why);
    const sq::Phi4EnsFramesFlowShape s = sq::phi4_ens_frames_flow_shape(dims[0] * dims[1] * dims[2], dims[2]);
    out[0] = s.fr_two ? 2 : 1;
    out[1] = s.fr_lds_bytes;
    out[2] = s.co_fr_two ? 2 : 1;
    out[3] = s.co_fr_lds_bytes;
    out[4] = (s.hs_two ? 2 : 1) | ((s.co_hs_two ? 2 : 1) << 8);
    out[5] = s.co_hs_lds_bytes;
    out[6] = s.fr_stash | (s.hfr_stash << 1) | (s.hs_stash << 2);
    out[7] = s.mask;
    return SQ_OK;
}

int sq_phi4_ens_flowed(sq_phi4_ens *e, int first, int count, double *sums, double *S, double *gt) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (e->fF == 0) return fail(SQ_E_STATE, "no flow set (sq_phi4_ens_set_flow)");
    if (count == 0 || (!sums && !S && !gt)) return SQ_OK;
    DeviceGuard dg(e->dev);
    rc = ens_sync_flow(e);
    if (rc) return rc;
    const size_t n = (size_t)count * (size_t)e->fF, Lz = (size_t)e->Lz, nt = (size_t)e->nt;
    rc = ens_flow_tmp(e, sizeof(double) * n * (4 + Lz + nt));
    if (rc) return rc;
    double *dsum = e->ftmp, *dS = dsum + 4 * n, *dg_ = dS + n * Lz;
    SQ_HIP(sq::phi4_ens_flowed_launch(ens_args(e), ens_flow_args(e), first, count, dsum, dS, dg_, e->stream));
    if (sums) SQ_HIP(hipMemcpyAsync(sums, dsum, sizeof(double) * 4 * n, hipMemcpyDeviceToHost, e->stream));
    if (S) SQ_HIP(hipMemcpyAsync(S, dS, sizeof(double) * n * Lz, hipMemcpyDeviceToHost, e->stream));
    if (gt) SQ_HIP(hipMemcpyAsync(gt, dg_, sizeof(double) * n * nt, hipMemcpyDeviceToHost, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_flow_field(sq_phi4_ens *e, int first, int count, int nsteps, float *phi) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (nsteps < 0 || nsteps > SQ_PHI4_ENS_MAX_FLOW_STEPS)
        return fail(SQ_E_ARG, "0 <= nsteps <= SQ_PHI4_ENS_MAX_FLOW_STEPS flow steps");
    if (!phi) return fail(SQ_E_ARG, "null argument");
    if (e->fF == 0) return fail(SQ_E_STATE, "no flow set (sq_phi4_ens_set_flow)");
    if (count == 0) return SQ_OK;
    DeviceGuard dg(e->dev);
    rc = ens_sync_flow(e);
    if (rc) return rc;
    const size_t bytes = sizeof(float) * (size_t)count * e->sites;
    rc = ens_flow_tmp(e, bytes);
    if (rc) return rc;
    float *out = reinterpret_cast<float *>(e->ftmp);
    SQ_HIP(sq::phi4_ens_flow_field_launch(ens_args(e), ens_flow_args(e), first, count, nsteps, out, e->stream));
    SQ_HIP(hipMemcpyAsync(phi, out, bytes, hipMemcpyDeviceToHost, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_fcorr_sums(sq_phi4_ens *e, int first, int count, double *G, double *S1, long long *nmeas) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (e->fF == 0) return fail(SQ_E_STATE, "no flow set (sq_phi4_ens_set_flow)");
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    const size_t F = (size_t)e->fF, nt = (size_t)e->nt, n = (size_t)count, f = (size_t)first;
    if (G) SQ_HIP(hipMemcpy(G, e->fG + f * F * nt, sizeof(double) * n * F * nt, hipMemcpyDeviceToHost));
    if (S1) SQ_HIP(hipMemcpy(S1, e->fS1 + f * F, sizeof(double) * n * F, hipMemcpyDeviceToHost));
    if (nmeas) {  // every level of a replica has the same count: the first one's
        std::vector<long long> N(n * F);
        SQ_HIP(hipMemcpy(N.data(), e->fN + f * F, sizeof(long long) * n * F, hipMemcpyDeviceToHost));
        for (size_t r = 0; r < n; ++r) nmeas[r] = N[r * F];
    }
    return SQ_OK;
}

int sq_phi4_ens_fcorr_reset(sq_phi4_ens *e, int first, int count) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0 || e->fF == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    const size_t F = (size_t)e->fF, nt = (size_t)e->nt, n = (size_t)count, f = (size_t)first;
    SQ_HIP(hipMemsetAsync(e->fG + f * F * nt, 0, sizeof(double) * n * F * nt, e->stream));
    SQ_HIP(hipMemsetAsync(e->fS1 + f * F, 0, sizeof(double) * n * F, e->stream));
    SQ_HIP(hipMemsetAsync(e->fN + f * F, 0, sizeof(long long) * n * F, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_fcorrelator(sq_phi4_ens *e, int connected, double *mean, double *err, int n, int *used) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (n < 0 || n > e->nt) return fail(SQ_E_ARG, "n must lie in [0, Lz / 2 + 1]");
    if (!mean && n > 0) return fail(SQ_E_ARG, "null argument");
    if (e->fF == 0) return fail(SQ_E_STATE, "no flow set (sq_phi4_ens_set_flow)");
    const size_t R = (size_t)e->R, nt = (size_t)e->nt, F = (size_t)e->fF;
    std::vector<double> G(R * F * nt), S1(R * F), s1(R);
    std::vector<long long> N(R);
    int rc = sq_phi4_ens_fcorr_sums(e, 0, e->R, G.data(), S1.data(), N.data());
    if (rc) return rc;
    int u = 0;
    for (size_t r = 0; r < R; ++r) u += N[r] > 0 ? 1 : 0;
    if (used) *used = u;
    if (u == 0) return fail(SQ_E_STATE, "no replica has a flow correlator measurement");
    for (size_t l = 0; l < F; ++l) {  // sq_phi4_ens_correlator's rule, level by level
        for (size_t r = 0; r < R; ++r) s1[r] = S1[r * F + l];
        ens_replica_stats(e, G.data() + l * nt, F * nt, connected ? s1.data() : nullptr, N.data(), u, n,
                          mean + l * (size_t)n, err ? err + l * (size_t)n : nullptr);
    }
    return SQ_OK;
}

int sq_phi4_ens_flow_shape_info(const int dims[3], int out[6]) {
    if (!dims || !out) return fail(SQ_E_ARG, "null argument");
    if (const char *why = ens_dims_error(dims[0], dims[1], dims[2])) return fail(SQ_E_ARG, why);
    const sq::Phi4EnsFlowShape s = sq::phi4_ens_flow_shape(dims[0] * dims[1] * dims[2], dims[2]);
    out[0] = s.two ? 2 : 1;
    out[1] = s.lds_bytes;
    out[2] = s.co_two ? 2 : 1;
    out[3] = s.co_lds_bytes;
    out[4] = s.fl_lds_bytes;
    out[5] = s.stash;
    return SQ_OK;
}

int sq_phi4_ens_perf(sq_phi4_ens *e, sq_perf_t *out) {
    if (!e || !out) return fail(SQ_E_ARG, "null argument");
    memset(out, 0, sizeof *out);
    out->steps = e->steps_total;
    out->site_updates = e->steps_total * (long long)e->sites;
    out->kernel_launches = e->launches;
    return SQ_OK;
}

}  // extern "C"

namespace {

// The MALA counters, allocated and zeroed at the first use.
int ens_mala_stat(sq_phi4_ens *e) {
    if (e->mstat) return SQ_OK;
    const size_t bytes = sizeof(long long) * 3 * (size_t)e->R;
    SQ_HIP(hipMalloc(&e->mstat, bytes));
    SQ_HIP(hipMemset(e->mstat, 0, bytes));
    SQ_HIP(hipDeviceSynchronize());  // the memset ran on the null stream
    return SQ_OK;
}

}  // namespace

extern "C" {

int sq_phi4_ens_step_mala(sq_phi4_ens *e, int nsteps, int every, double *series, int measure, double *rec) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nsteps < 0) return fail(SQ_E_ARG, "nsteps must be >= 0");
    if (measure & ~1) return fail(SQ_E_ARG, "measure holds bit 0 (correlator) only: a MALA step measures no momenta");
    if (measure ? every < 1 : every < 0)
        return fail(SQ_E_ARG, measure ? "a correlator measurement needs every >= 1" : "every must be >= 0");
    for (int r = 0; r < e->R; ++r)
        if (ens_rec(e->rep[(size_t)r]).sig == 0.0f)
            return fail(SQ_E_STATE, "a MALA step needs C != 0 in every replica (sig = sqrt(2 dtau) C is zero in fp32): "
                                    "without noise there is no proposal density");
    if (nsteps == 0) return SQ_OK;
    const bool corr = (measure & 1) != 0;
    DeviceGuard g(e->dev);
    int rc = ens_sync_recs(e);
    if (rc) return rc;
    rc = ens_mala_stat(e);
    if (rc) return rc;
    const size_t nrec = (every > 0 && series) ? (size_t)(nsteps / every) : 0;
    const size_t nd = nrec * (size_t)e->R * 4;
    if (nd > e->series_cap) {  // as ens_step
        (void)hipHostFree(e->series);
        e->series = nullptr;
        e->series_cap = 0;
        SQ_HIP(hipHostMalloc(&e->series, sizeof(double) * nd, hipHostMallocDefault));
        e->series_cap = nd;
    }
    const size_t nm = rec ? (size_t)nsteps * (size_t)e->R * 3 : 0;
    if (nm > e->mrec_cap) {
        (void)hipHostFree(e->mrec);
        e->mrec = nullptr;
        e->mrec_cap = 0;
        SQ_HIP(hipHostMalloc(&e->mrec, sizeof(double) * nm, hipHostMallocDefault));
        e->mrec_cap = nm;
    }
    sq::Phi4EnsArgs a = ens_args(e);
    a.nsteps = nsteps;
    a.every = (nd || corr) ? every : 0;
    a.series = nd ? e->series : nullptr;
    sq::Phi4EnsMalaArgs w{};
    w.stat = e->mstat;
    w.rec = nm ? e->mrec : nullptr;
    const sq::Phi4EnsCorrArgs c = ens_corr_args(e);
    SQ_HIP(sq::phi4_ens_mala_launch(a, w, corr ? &c : nullptr, e->R, e->stream));
    e->launches++;
    SQ_HIP(hipStreamSynchronize(e->stream));
    if (nd) memcpy(series, e->series, sizeof(double) * nd);
    if (nm) memcpy(rec, e->mrec, sizeof(double) * nm);
    e->adv += (unsigned long long)nsteps;
    for (auto &r : e->rep) r.step += (unsigned long long)nsteps;
    e->steps_total += (long long)nsteps * e->R;
    return SQ_OK;
}

int sq_phi4_ens_mala_stats(sq_phi4_ens *e, int first, int count, long long *out) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!out) return fail(SQ_E_ARG, "null argument");
    if (count == 0) return SQ_OK;
    if (!e->mstat) {  // no MALA step yet
        memset(out, 0, sizeof(long long) * 3 * (size_t)count);
        return SQ_OK;
    }
    DeviceGuard g(e->dev);
    SQ_HIP(hipMemcpy(out, e->mstat + 3 * (size_t)first, sizeof(long long) * 3 * (size_t)count, hipMemcpyDeviceToHost));
    return SQ_OK;
}

int sq_phi4_ens_mala_reset(sq_phi4_ens *e, int first, int count) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0 || !e->mstat) return SQ_OK;
    DeviceGuard g(e->dev);
    SQ_HIP(hipMemset(e->mstat + 3 * (size_t)first, 0, sizeof(long long) * 3 * (size_t)count));
    SQ_HIP(hipDeviceSynchronize());
    return SQ_OK;
}

}  // extern "C"

namespace {

// The HMC counters, allocated and zeroed at the first use.
int ens_hmc_stat(sq_phi4_ens *e) {
    if (e->hstat) return SQ_OK;
    const size_t bytes = sizeof(long long) * 4 * (size_t)e->R;
    SQ_HIP(hipMalloc(&e->hstat, bytes));
    SQ_HIP(hipMemset(e->hstat, 0, bytes));
    SQ_HIP(hipDeviceSynchronize());  // the memset ran on the null stream
    return SQ_OK;
}

}  // namespace

extern "C" {

int sq_phi4_ens_step_hmc(sq_phi4_ens *e, int ntraj, int nleap, int randomize, int every, double *series, int measure,
                         double *rec) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (ntraj < 0) return fail(SQ_E_ARG, "ntraj must be >= 0");
    if (nleap < 1 || nleap > SQ_PHI4_ENS_MAX_LEAP) return fail(SQ_E_ARG, "nleap must lie in [1, 4096]");
    if (measure & ~1) return fail(SQ_E_ARG, "measure holds bit 0 (correlator) only: a trajectory measures no momenta");
    if (measure ? every < 1 : every < 0)
        return fail(SQ_E_ARG, measure ? "a correlator measurement needs every >= 1" : "every must be >= 0");
    for (int r = 0; r < e->R; ++r)
        if (ens_rec(e->rep[(size_t)r]).sig == 0.0f)
            return fail(SQ_E_STATE, "a trajectory needs C != 0 in every replica (sig = sqrt(2 dtau) C is zero in fp32): "
                                    "without noise there is no momentum to draw");
    if (ntraj == 0) return SQ_OK;
    const bool corr = (measure & 1) != 0;
    DeviceGuard g(e->dev);
    int rc = ens_sync_recs(e);
    if (rc) return rc;
    rc = ens_hmc_stat(e);
    if (rc) return rc;
    const size_t nrec = (every > 0 && series) ? (size_t)(ntraj / every) : 0;
    const size_t nd = nrec * (size_t)e->R * 4;
    if (nd > e->series_cap) {  // as ens_step
        (void)hipHostFree(e->series);
        e->series = nullptr;
        e->series_cap = 0;
        SQ_HIP(hipHostMalloc(&e->series, sizeof(double) * nd, hipHostMallocDefault));
        e->series_cap = nd;
    }
    const size_t nm = rec ? (size_t)ntraj * (size_t)e->R * 4 : 0;
    if (nm > e->hrec_cap) {
        (void)hipHostFree(e->hrec);
        e->hrec = nullptr;
        e->hrec_cap = 0;
        SQ_HIP(hipHostMalloc(&e->hrec, sizeof(double) * nm, hipHostMallocDefault));
        e->hrec_cap = nm;
    }
    sq::Phi4EnsArgs a = ens_args(e);
    a.nsteps = ntraj;
    a.every = (nd || corr) ? every : 0;
    a.series = nd ? e->series : nullptr;
    sq::Phi4EnsHmcArgs w{};
    w.stat = e->hstat;
    w.rec = nm ? e->hrec : nullptr;
    w.nleap = nleap;
    w.randomize = randomize != 0 ? 1 : 0;
    const sq::Phi4EnsCorrArgs c = ens_corr_args(e);
    SQ_HIP(sq::phi4_ens_hmc_launch(a, w, corr ? &c : nullptr, e->R, e->stream));
    e->launches++;
    SQ_HIP(hipStreamSynchronize(e->stream));
    if (nd) memcpy(series, e->series, sizeof(double) * nd);
    if (nm) memcpy(rec, e->hrec, sizeof(double) * nm);
    e->adv += (unsigned long long)ntraj;  // one count per trajectory
    for (auto &r : e->rep) r.step += (unsigned long long)ntraj;
    e->steps_total += (long long)ntraj * e->R;
    return SQ_OK;
}

int sq_phi4_ens_hmc_stats(sq_phi4_ens *e, int first, int count, long long *out) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!out) return fail(SQ_E_ARG, "null argument");
    if (count == 0) return SQ_OK;
    if (!e->hstat) {  // no trajectory yet
        memset(out, 0, sizeof(long long) * 4 * (size_t)count);
        return SQ_OK;
    }
    DeviceGuard g(e->dev);
    SQ_HIP(hipMemcpy(out, e->hstat + 4 * (size_t)first, sizeof(long long) * 4 * (size_t)count, hipMemcpyDeviceToHost));
    return SQ_OK;
}

int sq_phi4_ens_hmc_reset(sq_phi4_ens *e, int first, int count) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0 || !e->hstat) return SQ_OK;
    DeviceGuard g(e->dev);
    SQ_HIP(hipMemset(e->hstat + 4 * (size_t)first, 0, sizeof(long long) * 4 * (size_t)count));
    SQ_HIP(hipDeviceSynchronize());
    return SQ_OK;
}

}  // extern "C"

// ---- replica exchange (sq_phi4_ens_exchange.hip) ----
namespace {

// A pinned host buffer of at least n doubles (the kernels write their records there, as ens_step's series).
int ens_pinned(double *&buf, size_t &cap, size_t n) {
    if (n <= cap) return SQ_OK;
    (void)hipHostFree(buf);
    buf = nullptr;
    cap = 0;
    SQ_HIP(hipHostMalloc(&buf, sizeof(double) * n, hipHostMallocDefault));
    cap = n;
    return SQ_OK;
}

// What stands against an exchange round, checked before any device work.
int ens_xchg_state(const sq_phi4_ens *e) {
    if (e->nlad == 0)
        return fail(SQ_E_STATE, "an exchange round needs ladders: call sq_phi4_ens_set_ladder first");
    for (int r = 0; r < e->R; ++r)
        if (ens_rec(e->rep[(size_t)r]).sig == 0.0f)
            return fail(SQ_E_STATE, "an exchange round needs C != 0 in every replica (sig = sqrt(2 dtau) C is zero in "
                                    "fp32): beta = 2 dtau / sig^2 has no value");
    return SQ_OK;
}

// Enqueue round e->xround + i; rec: the round's [R][5] rows in pinned memory, nullable.
int ens_xchg_enqueue(sq_phi4_ens *e, int i, double *rec) {
    sq::Phi4EnsXchgArgs w{};
    w.stat = e->xstat;
    w.walker = e->walker;
    w.rec = rec;
    w.nlad = e->nlad;
    w.x = e->xround + (unsigned long long)i;
    if (sq::phi4_ens_xchg_pairs(w.nlad, w.x) == 0) return SQ_OK;  // nothing to launch
    SQ_HIP(sq::phi4_ens_exchange_launch(ens_args(e), w, e->R, e->stream));
    e->launches++;
    return SQ_OK;
}

// The rows of the slots without a partner, round by round behind the synchronisation: verdict -1, partner -1,
// Delta = u = 0 and the label the slot held before the round (lab: the labels at the call's start, updated here).
void ens_xchg_fill(const sq_phi4_ens *e, int nrounds, double *rec, std::vector<int> &lab) {
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
}

}  // namespace

extern "C" {

int sq_phi4_ens_set_ladder(sq_phi4_ens *e, int nlad) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nlad != 0 && (nlad < 2 || nlad > e->R || e->R % nlad != 0))
        return fail(SQ_E_ARG, "nlad must be 0 (no ladders) or lie in [2, nrep] and divide nrep");
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
    if (rc) return rc;
    if (nrounds == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    rc = ens_sync_recs(e);
    if (rc) return rc;
    const size_t nx = rec ? (size_t)nrounds * (size_t)e->R * 5 : 0;
    rc = ens_pinned(e->xrec, e->xrec_cap, nx);
    if (rc) return rc;
    std::vector<int> lab;
    if (nx) {
        lab.resize((size_t)e->R);
        SQ_HIP(hipMemcpy(lab.data(), e->walker, sizeof(int) * (size_t)e->R, hipMemcpyDeviceToHost));
    }
    for (int i = 0; i < nrounds; ++i) {
        rc = ens_xchg_enqueue(e, i, nx ? e->xrec + 5 * (size_t)i * (size_t)e->R : nullptr);
        if (rc) break;
    }
    const hipError_t he = hipStreamSynchronize(e->stream);
    if (rc) return rc;
    SQ_HIP(he);
    if (nx) {
        ens_xchg_fill(e, nrounds, e->xrec, lab);
        memcpy(rec, e->xrec, sizeof(double) * nx);
    }
    e->xround += (unsigned long long)nrounds;
    return SQ_OK;
}

int sq_phi4_ens_step_hmc_exchange(sq_phi4_ens *e, int nrounds, int ntraj, int nleap, int randomize, int every,
                                  double *series, int measure, double *rec_hmc, double *rec_x) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nrounds < 0) return fail(SQ_E_ARG, "nrounds must be >= 0");
    if (ntraj < 0) return fail(SQ_E_ARG, "ntraj must be >= 0");
    if (nleap < 1 || nleap > SQ_PHI4_ENS_MAX_LEAP) return fail(SQ_E_ARG, "nleap must lie in [1, 4096]");
    if (measure & ~1) return fail(SQ_E_ARG, "measure holds bit 0 (correlator) only: a trajectory measures no momenta");
    if (measure ? every < 1 : every < 0)
        return fail(SQ_E_ARG, measure ? "a correlator measurement needs every >= 1" : "every must be >= 0");
    if (every > 0 && ntraj % every != 0)
        return fail(SQ_E_ARG, "every must divide ntraj: the measurements are those of the separate calls");
    int rc = ens_xchg_state(e);  // the trajectories' C != 0 as well
    if (rc) return rc;
    if (nrounds == 0) return SQ_OK;
    const bool corr = (measure & 1) != 0;
    DeviceGuard g(e->dev);
    rc = ens_sync_recs(e);
    if (rc) return rc;
    rc = ens_hmc_stat(e);
    if (rc) return rc;
    const size_t per = (every > 0 && series) ? (size_t)(ntraj / every) * (size_t)e->R * 4 : 0;  // a round's series
    const size_t nd = per * (size_t)nrounds;
    const size_t perh = rec_hmc ? (size_t)ntraj * (size_t)e->R * 4 : 0;
    const size_t nm = perh * (size_t)nrounds;
    const size_t nx = rec_x ? (size_t)nrounds * (size_t)e->R * 5 : 0;
    rc = ens_pinned(e->series, e->series_cap, nd);
    if (rc) return rc;
    rc = ens_pinned(e->hrec, e->hrec_cap, nm);
    if (rc) return rc;
    rc = ens_pinned(e->xrec, e->xrec_cap, nx);
    if (rc) return rc;
    std::vector<int> lab;
    if (nx) {
        lab.resize((size_t)e->R);
        SQ_HIP(hipMemcpy(lab.data(), e->walker, sizeof(int) * (size_t)e->R, hipMemcpyDeviceToHost));
    }
    sq::Phi4EnsHmcArgs w{};
    w.stat = e->hstat;
    w.nleap = nleap;
    w.randomize = randomize != 0 ? 1 : 0;
    const sq::Phi4EnsCorrArgs c = ens_corr_args(e);
    for (int i = 0; i < nrounds && !rc; ++i) {
        if (ntraj > 0) {
            sq::Phi4EnsArgs a = ens_args(e);
            a.adv = e->adv + (unsigned long long)i * (unsigned long long)ntraj;
            a.nsteps = ntraj;
            a.every = (nd || corr) ? every : 0;
            a.series = nd ? e->series + per * (size_t)i : nullptr;
            w.rec = nm ? e->hrec + perh * (size_t)i : nullptr;
            const hipError_t he = sq::phi4_ens_hmc_launch(a, w, corr ? &c : nullptr, e->R, e->stream);
            if (he != hipSuccess) {
                rc = fail(SQ_E_HIP, std::string("phi4_ens_hmc_launch: ") + hipGetErrorString(he));
                break;
            }
            e->launches++;
        }
        rc = ens_xchg_enqueue(e, i, nx ? e->xrec + 5 * (size_t)i * (size_t)e->R : nullptr);
    }
    const hipError_t he = hipStreamSynchronize(e->stream);
    if (rc) return rc;
    SQ_HIP(he);
    if (nd) memcpy(series, e->series, sizeof(double) * nd);
    if (nm) memcpy(rec_hmc, e->hrec, sizeof(double) * nm);
    if (nx) {
        ens_xchg_fill(e, nrounds, e->xrec, lab);
        memcpy(rec_x, e->xrec, sizeof(double) * nx);
    }
    const unsigned long long tot = (unsigned long long)nrounds * (unsigned long long)ntraj;
    e->adv += tot;  // one count per trajectory
    for (auto &r : e->rep) r.step += tot;
    e->steps_total += (long long)tot * e->R;
    e->xround += (unsigned long long)nrounds;
    return SQ_OK;
}

int sq_phi4_ens_exchange_stats(sq_phi4_ens *e, int first, int count, long long *out) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!out) return fail(SQ_E_ARG, "null argument");
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    SQ_HIP(hipMemcpy(out, e->xstat + 2 * (size_t)first, sizeof(long long) * 2 * (size_t)count, hipMemcpyDeviceToHost));
    return SQ_OK;
}

int sq_phi4_ens_walkers(sq_phi4_ens *e, int first, int count, int *out) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!out) return fail(SQ_E_ARG, "null argument");
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    SQ_HIP(hipMemcpy(out, e->walker + first, sizeof(int) * (size_t)count, hipMemcpyDeviceToHost));
    return SQ_OK;
}

int sq_phi4_ens_exchange_reset(sq_phi4_ens *e, int first, int count, int walkers) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    SQ_HIP(hipMemset(e->xstat + 2 * (size_t)first, 0, sizeof(long long) * 2 * (size_t)count));
    if (walkers) {
        std::vector<int> id((size_t)count);
        for (int r = 0; r < count; ++r) id[(size_t)r] = first + r;
        SQ_HIP(hipMemcpy(e->walker + first, id.data(), sizeof(int) * (size_t)count, hipMemcpyHostToDevice));
    }
    SQ_HIP(hipDeviceSynchronize());
    return SQ_OK;
}

int sq_phi4_ens_exchange_shape_info(const int dims[3], int out[4]) {
    if (!dims || !out) return fail(SQ_E_ARG, "null argument");
    if (const char *why = ens_dims_error(dims[0], dims[1], dims[2])) return fail(SQ_E_ARG, why);
    const sq::Phi4EnsShape s = sq::phi4_ens_shape(dims[0] * dims[1] * dims[2]);
    out[0] = s.K;
    out[1] = s.T;
    out[2] = s.mom_lds_bytes;
    out[3] = sq::kPhi4EnsLdsBytes;
    return SQ_OK;
}

}  // extern "C"

// ---- Swendsen-Wang cluster sweeps (sq_phi4_ens_cluster.hip) ----
namespace {

// What stands against a cluster sweep, checked before any device work.
int ens_cluster_state(const sq_phi4_ens *e) {
    for (int r = 0; r < e->R; ++r)
        if (ens_rec(e->rep[(size_t)r]).sig == 0.0f)
            return fail(SQ_E_STATE, "a cluster sweep needs C != 0 in every replica (sig = sqrt(2 dtau) C is zero in "
                                    "fp32): beta = 2 dtau / sig^2 has no value");
    return SQ_OK;
}

// The device buffers of a call's records: nsweeps sweeps of [R][sites] each, either nullable.
int ens_cluster_bufs(sq_phi4_ens *e, size_t nb, size_t nl) {
    if (nb > e->cbonds_cap) {
        (void)hipFree(e->cbonds);
        e->cbonds = nullptr;
        e->cbonds_cap = 0;
        SQ_HIP(hipMalloc(&e->cbonds, nb));
        e->cbonds_cap = nb;
    }
    if (nl > e->clabels_cap) {
        (void)hipFree(e->clabels);
        e->clabels = nullptr;
        e->clabels_cap = 0;
        SQ_HIP(hipMalloc(&e->clabels, sizeof(int) * nl));
        e->clabels_cap = nl;
    }
    return SQ_OK;
}

// Enqueue sweep e->csweep + i; bonds, labels: the call's device buffers, nullable.
int ens_cluster_enqueue(sq_phi4_ens *e, int i, bool bonds, bool labels) {
    const size_t per = (size_t)e->R * e->sites;
    sq::Phi4EnsClusterArgs w{};
    w.stat = e->cstat;
    w.bonds = bonds ? e->cbonds + per * (size_t)i : nullptr;
    w.labels = labels ? e->clabels + per * (size_t)i : nullptr;
    w.c = e->csweep + (unsigned long long)i;
    const hipError_t he = sq::phi4_ens_cluster_launch(ens_args(e), w, e->R, e->stream);
    if (he != hipSuccess) return fail(SQ_E_HIP, std::string("phi4_ens_cluster_launch: ") + hipGetErrorString(he));
    e->launches++;
    return SQ_OK;
}

// The records of nsweeps sweeps back to the caller, behind the synchronisation.
int ens_cluster_readback(sq_phi4_ens *e, int nsweeps, unsigned char *bonds, int *labels) {
    const size_t n = (size_t)nsweeps * (size_t)e->R * e->sites;
    if (bonds) SQ_HIP(hipMemcpy(bonds, e->cbonds, n, hipMemcpyDeviceToHost));
    if (labels) SQ_HIP(hipMemcpy(labels, e->clabels, sizeof(int) * n, hipMemcpyDeviceToHost));
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
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nsweeps < 0) return fail(SQ_E_ARG, "nsweeps must be >= 0");
    int rc = ens_cluster_state(e);
    if (rc) return rc;
    if (nsweeps == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    rc = ens_sync_recs(e);
    if (rc) return rc;
    const size_t n = (size_t)nsweeps * (size_t)e->R * e->sites;
    rc = ens_cluster_bufs(e, bonds ? n : 0, labels ? n : 0);
    if (rc) return rc;
    for (int i = 0; i < nsweeps && !rc; ++i) rc = ens_cluster_enqueue(e, i, bonds != nullptr, labels != nullptr);
    const hipError_t he = hipStreamSynchronize(e->stream);
    if (rc) return rc;
    SQ_HIP(he);
    rc = ens_cluster_readback(e, nsweeps, bonds, labels);
    if (rc) return rc;
    e->csweep += (unsigned long long)nsweeps;
    return SQ_OK;
}

int sq_phi4_ens_step_hmc_cluster(sq_phi4_ens *e, int nrounds, int ntraj, int nleap, int randomize, int every,
                                 double *series, int measure, double *rec_hmc, unsigned char *bonds, int *labels) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (nrounds < 0) return fail(SQ_E_ARG, "nrounds must be >= 0");
    if (ntraj < 0) return fail(SQ_E_ARG, "ntraj must be >= 0");
    if (nleap < 1 || nleap > SQ_PHI4_ENS_MAX_LEAP) return fail(SQ_E_ARG, "nleap must lie in [1, 4096]");
    if (measure & ~1) return fail(SQ_E_ARG, "measure holds bit 0 (correlator) only: a trajectory measures no momenta");
    if (measure ? every < 1 : every < 0)
        return fail(SQ_E_ARG, measure ? "a correlator measurement needs every >= 1" : "every must be >= 0");
    if (every > 0 && ntraj % every != 0)
        return fail(SQ_E_ARG, "every must divide ntraj: the measurements are those of the separate calls");
    int rc = ens_cluster_state(e);  // the trajectories' C != 0 as well
    if (rc) return rc;
    if (nrounds == 0) return SQ_OK;
    const bool corr = (measure & 1) != 0;
    DeviceGuard g(e->dev);
    rc = ens_sync_recs(e);
    if (rc) return rc;
    rc = ens_hmc_stat(e);
    if (rc) return rc;
    const size_t per = (every > 0 && series) ? (size_t)(ntraj / every) * (size_t)e->R * 4 : 0;  // a round's series
    const size_t nd = per * (size_t)nrounds;
    const size_t perh = rec_hmc ? (size_t)ntraj * (size_t)e->R * 4 : 0;
    const size_t nm = perh * (size_t)nrounds;
    const size_t n = (size_t)nrounds * (size_t)e->R * e->sites;
    rc = ens_pinned(e->series, e->series_cap, nd);
    if (rc) return rc;
    rc = ens_pinned(e->hrec, e->hrec_cap, nm);
    if (rc) return rc;
    rc = ens_cluster_bufs(e, bonds ? n : 0, labels ? n : 0);
    if (rc) return rc;
    sq::Phi4EnsHmcArgs w{};
    w.stat = e->hstat;
    w.nleap = nleap;
    w.randomize = randomize != 0 ? 1 : 0;
    const sq::Phi4EnsCorrArgs c = ens_corr_args(e);
    for (int i = 0; i < nrounds && !rc; ++i) {
        if (ntraj > 0) {
            sq::Phi4EnsArgs a = ens_args(e);
            a.adv = e->adv + (unsigned long long)i * (unsigned long long)ntraj;
            a.nsteps = ntraj;
            a.every = (nd || corr) ? every : 0;
            a.series = nd ? e->series + per * (size_t)i : nullptr;
            w.rec = nm ? e->hrec + perh * (size_t)i : nullptr;
            const hipError_t he = sq::phi4_ens_hmc_launch(a, w, corr ? &c : nullptr, e->R, e->stream);
            if (he != hipSuccess) {
                rc = fail(SQ_E_HIP, std::string("phi4_ens_hmc_launch: ") + hipGetErrorString(he));
                break;
            }
            e->launches++;
        }
        rc = ens_cluster_enqueue(e, i, bonds != nullptr, labels != nullptr);
    }
    const hipError_t he = hipStreamSynchronize(e->stream);
    if (rc) return rc;
    SQ_HIP(he);
    if (nd) memcpy(series, e->series, sizeof(double) * nd);
    if (nm) memcpy(rec_hmc, e->hrec, sizeof(double) * nm);
    rc = ens_cluster_readback(e, nrounds, bonds, labels);
    if (rc) return rc;
    const unsigned long long tot = (unsigned long long)nrounds * (unsigned long long)ntraj;
    e->adv += tot;  // one count per trajectory
    for (auto &r : e->rep) r.step += tot;
    e->steps_total += (long long)tot * e->R;
    e->csweep += (unsigned long long)nrounds;
    return SQ_OK;
}

int sq_phi4_ens_cluster_stats(sq_phi4_ens *e, int first, int count, long long *out) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (!out) return fail(SQ_E_ARG, "null argument");
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    SQ_HIP(hipMemcpy(out, e->cstat + 5 * (size_t)first, sizeof(long long) * 5 * (size_t)count, hipMemcpyDeviceToHost));
    return SQ_OK;
}

int sq_phi4_ens_cluster_reset(sq_phi4_ens *e, int first, int count) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    SQ_HIP(hipMemset(e->cstat + 5 * (size_t)first, 0, sizeof(long long) * 5 * (size_t)count));
    SQ_HIP(hipDeviceSynchronize());
    return SQ_OK;
}

int sq_phi4_ens_cluster_shape_info(const int dims[3], int out[4]) {
    if (!dims || !out) return fail(SQ_E_ARG, "null argument");
    if (const char *why = ens_dims_error(dims[0], dims[1], dims[2])) return fail(SQ_E_ARG, why);
    const sq::Phi4EnsShape s = sq::phi4_ens_shape(dims[0] * dims[1] * dims[2]);
    out[0] = s.K;
    out[1] = s.T;
    out[2] = s.mom_lds_bytes;
    out[3] = sq::kPhi4EnsLdsBytes;
    return SQ_OK;
}

}  // extern "C"
