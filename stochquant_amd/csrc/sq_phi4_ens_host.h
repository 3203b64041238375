// sq_phi4_ens_host.h -- the phi^4 lattice ensemble's handle and the helpers its host files share:
// sq_phi4_ens.cpp (the handle, parameters, Euler and Heun steps), sq_phi4_ens_frames.cpp,
// sq_phi4_ens_corr.cpp (correlator, momenta), sq_phi4_ens_flow.cpp, sq_phi4_ens_samplers.cpp (MALA, HMC,
// exchange, cluster) and sq_phi4_ens_ckpt.cpp (digest, save, load).  Host only; the kernels' side is sq_phi4_ens.h.
//
// Every buffer of the handle is a Buf: it grows with reserve() and the handle's destructor frees it.  Nothing is
// freed by hand.
#pragma once
#include <cmath>
#include <cstring>
#include <vector>

#include "sq_buf.h"
#include "sq_ctx.h"
#include "sq_phi4_ens.h"

// the handle, its buffer types and the helpers stay inside the library: no dynamic symbol comes from here
#pragma GCC visibility push(hidden)
namespace sq {

struct DevAlloc {
    static bool alloc(void **p, size_t bytes) { return hipMalloc(p, bytes) == hipSuccess; }
    static void free(void *p) { (void)hipFree(p); }
};
struct PinAlloc {
    static bool alloc(void **p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault) == hipSuccess; }
    static void free(void *p) { (void)hipHostFree(p); }
};
template <class T>
using DevBuf = Buf<T, DevAlloc>;  // device memory
// Pinned host memory.  The kernels write their records straight there (32 B per replica and record, posted
// writes), visible once the stream is idle: a device buffer and its copy back cost a fixed 15-20 us per call (a
// 200-step call of one 8^3 lattice with every = 20: 24 % over every = 0 with the copy, 13 % without).
template <class T>
using PinBuf = Buf<T, PinAlloc>;

}  // namespace sq

struct sq_phi4_ens {
    sq_params p{};
    int dev = 0, Lx = 0, Ly = 0, Lz = 0, R = 0;
    size_t sites = 0;
    struct Rep {
        double dtau, m2, lambda, C;
        unsigned long long seed, step;
    };
    std::vector<Rep> rep;                // [R]
    sq::DevBuf<float> field;             // [R][Lz][Ly][Lx]
    sq::DevBuf<sq::Phi4EnsRec> rec;      // [R]
    sq::DevBuf<int> flags;               // [R]
    sq::PinBuf<double> series;           // the last step call's records, written by the kernel
    sq::DevBuf<double> mom;              // [R][5]
    sq::DevBuf<unsigned long long> dig;  // [R] sq_phi4_ensemble_digest's device buffer (first digest on)
    bool rec_dirty = true;               // the device records are behind rep[]
    std::vector<sq::Phi4EnsFrameState> fst;  // [R] frame state, current between calls
    sq::DevBuf<sq::Phi4EnsFrameState> fst_dev;
    sq::DevBuf<float> frecs;             // [R][3][loops] the last frame's records (first frames call on)
    sq::DevBuf<int> fr_stable;           // [nframes][R] a frames call's verdicts ...
    sq::DevBuf<double> fr_dtau;          // ... and Δτ
    unsigned long long adv = 0;          // steps run since the records were written
    int nt = 0;                          // Lz / 2 + 1 correlator distances
    sq::DevBuf<double> cG;               // [R][nt] correlator accumulators: zero at creation, cleared by
    sq::DevBuf<double> cS1;              // [R]     sq_phi4_ens_corr_reset only
    sq::DevBuf<long long> cN;            // [R]
    sq::DevBuf<double> ctmp;             // sq_phi4_ens_slices' device buffer: [count][Lz] then [count][nt]
    int pM = 0;                          // momenta set (sq_phi4_ens_set_momenta), 0 .. SQ_PHI4_ENS_MAX_MOMENTA
    int pn[2 * SQ_PHI4_ENS_MAX_MOMENTA] = {};  // their (nx, ny)
    sq::DevBuf<double> ptab;             // twiddle tables: cx | sx [8][Lx], cy | sy [8][Ly] (first set_momenta on)
    sq::DevBuf<double> pG;               // [R][pM][nt] momentum accumulators: zeroed by set_momenta and
    sq::DevBuf<long long> pN;            // [R]         sq_phi4_ens_pcorr_reset only
    sq::DevBuf<double> ptmp;             // sq_phi4_ens_pslices' device buffer: [count][pM][Lz][2] then [count][pM][nt]
    int fF = 0;                          // flow levels set (sq_phi4_ens_set_flow), 0: no flow
    int flev[SQ_PHI4_ENS_MAX_FLOW_LEVELS] = {};  // ... strictly ascending flow steps
    double feps = 0.0, fm2 = NAN, flam = NAN;    // flow step; the flow's m², λ (NaN: each replica's own)
    sq::DevBuf<sq::Phi4EnsFlowRec> frec;  // [R] flow coefficients (first set_flow on)
    bool frec_dirty = true;              // ... are behind rep[] / the flow parameters
    sq::DevBuf<double> fG;               // [R][fF][nt] flow accumulators: zeroed by set_flow and
    sq::DevBuf<double> fS1;              // [R][fF]     sq_phi4_ens_fcorr_reset only
    sq::DevBuf<long long> fN;            // [R][fF]
    sq::DevBuf<unsigned char> ftmp;      // sq_phi4_ens_flowed's / _flow_field's device buffer
    sq::DevBuf<long long> mstat;         // [R][3] MALA counters: proposed, accepted, guard trips (first MALA call on);
                                         // cleared by sq_phi4_ens_mala_reset only
    sq::PinBuf<double> mrec;             // the last MALA call's per-step records, written by the kernel
    sq::DevBuf<long long> hstat;         // [R][4] HMC counters: trajectories, accepted, guard trips, leapfrog steps
                                         // (first HMC call on); cleared by sq_phi4_ens_hmc_reset only
    sq::PinBuf<double> hrec;             // the last HMC call's per-trajectory records
    int nlad = 0;                        // slots per exchange ladder (sq_phi4_ens_set_ladder), 0: no ladders
    unsigned long long xround = 0;       // the exchange-round counter
    sq::DevBuf<long long> xstat;         // [R][2] attempts, acceptances of the pair (r, r + 1); zero at creation,
                                         // cleared by sq_phi4_ens_exchange_reset only
    sq::DevBuf<int> walker;              // [R] the label of the field each slot holds; r at creation
    sq::PinBuf<double> xrec;             // the last exchange call's records, written by the kernel
    unsigned long long csweep = 0;       // the cluster-sweep counter
    sq::DevBuf<long long> cstat;         // [R][5] sweeps, clusters, flipped clusters, flipped sites, unconverged
                                         // sweeps; zero at creation, cleared by sq_phi4_ens_cluster_reset only
    sq::DevBuf<unsigned char> cbonds;    // the last cluster call's bond records: device memory, read back once
    sq::DevBuf<int> clabels;             // ... and its label records
    sq::PinBuf<double> cser;             // the last improved cluster call's records, written by the kernel
    sq::DevBuf<long long> cweights;      // ... and its cluster sums: device memory, read back once
    sq::DevBuf<double> ctab;             // the unit momentum's tables c | s of x, y, z (first improved call on)
    sq::DevBuf<int> cpark;               // [R][sites] the parked labels of a shape that parks them (likewise)
    hipStream_t stream = nullptr;
    long long steps_total = 0, launches = 0;
};

namespace sq {

// ---- buffers ----
int ens_alloc_failed(const char *call);
template <class T>
int ens_reserve(DevBuf<T> &b, size_t n) {
    return b.reserve(n) ? SQ_OK : ens_alloc_failed("hipMalloc");
}
template <class T>
int ens_reserve(PinBuf<T> &b, size_t n) {
    return b.reserve(n) ? SQ_OK : ens_alloc_failed("hipHostMalloc");
}
// A table of n elements, allocated and zeroed at its first use.
template <class T>
int ens_zeroed(DevBuf<T> &b, size_t n) {
    if (b.data()) return SQ_OK;
    int rc = ens_reserve(b, n);
    if (rc) return rc;
    SQ_HIP(hipMemset(b.data(), 0, sizeof(T) * n));
    SQ_HIP(hipDeviceSynchronize());  // the memset ran on the null stream
    return SQ_OK;
}

// ---- sq_phi4_ens.cpp ----
int ens_range(const sq_phi4_ens *e, int first, int count);
// The preamble of every *_shape_info: both pointers given, and a legal lattice shape.
int ens_shape_dims(const int dims[3], const void *out);
// create_phi4's parameter bound, per replica (the guard needs every update of a field inside [-clamp, clamp] to
// be finite or an infinity, never NaN)
bool ens_params_ok(double cl, double h, double m2, double lambda, double C);
Phi4EnsRec ens_rec(const sq_phi4_ens::Rep &r);
// Bring the device records up to rep[] (the stream is idle: every entry point synchronises it).
int ens_sync_recs(sq_phi4_ens *e);
Phi4EnsArgs ens_args(const sq_phi4_ens *e);
// SQ_E_STATE unless C != 0 in every replica: "<subject> needs C != 0 in every replica (...): <reason>".
int ens_needs_noise(const sq_phi4_ens *e, const char *subject, const char *reason);
// n steps (or trajectories) ran in every replica.
void ens_advance(sq_phi4_ens *e, unsigned long long n);
// Rows first .. first + count of a [R][w] counter table: to out (a table never allocated reads as zeros), or
// cleared (one never allocated stays so).
int ens_read_rows(sq_phi4_ens *e, DevBuf<long long> sq_phi4_ens::*tab, int w, int first, int count, long long *out);
int ens_clear_rows(sq_phi4_ens *e, DevBuf<long long> sq_phi4_ens::*tab, int w, int first, int count);

// What a step or a frames call measures: the ABI's `measure` bits, and kEnsFlow for the flow launch of the
// scheme (a flow is set, series or kEnsCorr given, no kEnsMom; kEnsCorr then means the flow accumulators).
constexpr int kEnsCorr = 1, kEnsMom = 2, kEnsFlow = 4;
// sq_phi4_ens_step and its _corr, _pcorr and _heun forms; with a measurement every >= 1, checked by the caller.
// scheme: SQ_SCHEME_EULER or SQ_SCHEME_HEUN; one Heun step counts as one step everywhere on the host.
int ens_step(sq_phi4_ens *e, int nsteps, int every, double *series, int measure, int scheme);

// ---- sq_phi4_ens_frames.cpp ----
// Every sq_phi4_ens_run_frames*; with kEnsFlow the series is [nframes][F][R][4].
int ens_run_frames(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series, int measure, int scheme);

// ---- sq_phi4_ens_corr.cpp ----
// What stands against momenta on a lattice of this shape, nullptr where they run (sq_phi4_ens_set_momenta, a load).
const char *ens_momenta_shape_error(int sites, int Lz);
// sq_phi4_ens_set_momenta behind its checks: the tables, the layout, the accumulators zeroed.  Only an allocation
// or the runtime can fail it; M = 0 is applied on any shape (a load of a handle without momenta).
int ens_apply_momenta(sq_phi4_ens *e, int M, const int *nxy);
Phi4EnsCorrArgs ens_corr_args(const sq_phi4_ens *e);
// The handle's momenta for a launch; corr: the zero-momentum accumulators advance as well.
Phi4EnsPCorrArgs ens_pcorr_args(const sq_phi4_ens *e, bool corr);
// The replicas with N[r] > 0, to *used (nullable) as well; none: SQ_E_STATE "no replica has a <what> measurement".
int ens_replicas_used(const std::vector<long long> &N, const char *what, int *used, int *u);
// Replica statistics of one accumulator row: replica r's entries at G[r * stride + t], t < n; the u replicas with
// N[r] > 0 in index order; S1 non-null: the connected form.  err nullable.
void ens_replica_stats(const sq_phi4_ens *e, const double *G, size_t stride, const double *S1, const long long *N,
                       int u, int n, double *mean, double *err);

// ---- sq_phi4_ens_flow.cpp ----
Phi4EnsFlowArgs ens_flow_args(const sq_phi4_ens *e);
// Bring the device's flow records up to rep[] and the flow parameters (the stream is idle).
int ens_sync_flow(sq_phi4_ens *e);
// sq_phi4_ens_set_flow behind its checks (fm2, flam NaN: each replica's own); only an allocation can fail it.
int ens_apply_flow(sq_phi4_ens *e, double eps, int nlevels, const int *levels, double fm2, double flam);

}  // namespace sq
#pragma GCC visibility pop
