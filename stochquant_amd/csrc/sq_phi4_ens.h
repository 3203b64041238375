// sq_phi4_ens.h -- the phi^4 lattice ensemble (sq_phi4_ens.hip, the
// sq_phi4_ens_* entry points of sq_phi4_ens.cpp): R independent periodic
// lattices of one shape advanced together, one launch per call, one work-group
// per lattice, the field on-chip between the call's first and last step.
// Raw steps (phi4_ens_step_launch) or whole frames decided in the kernel
// (phi4_ens_frames_launch: per replica the stability rule, the rollback and
// the Δτ controller of DESIGN.md §7), either with Euler steps or with
// second-order Heun steps (phi4_ens_heun_launch, phi4_ens_heun_frames_launch).
// Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sq {

constexpr int kPhi4EnsMaxSites = 32768;  // 128 KiB of fp32: one LDS image of the lattice
constexpr int kPhi4EnsMaxLanes = 1024;
constexpr int kPhi4EnsLdsBytes = 160 * 1024;
// LDS behind the image(s): per wave 4 doubles (the sums) and one float (max |phi|), for 16 waves
constexpr int kPhi4EnsScratchBytes = 16 * 4 * 8 + 16 * 4;
// the frames kernel's words behind that: three rotating step records (u64 key, u32 max |phi'|) and the two
// maxima of the first frame's start field
constexpr int kPhi4EnsFrameScratchBytes = kPhi4EnsScratchBytes + 3 * 8 + 3 * 4 + 2 * 4 + 4;

// One replica's step coefficients, derived from its Δτ, m², λ, C as
// phi4_base_args derives a context's (sq_phi4_steps.cpp), its Philox key and
// its step counter at the time the records were last written; the kernels
// only read them.
struct Phi4EnsRec {
    float h, m2, lam6, sig, sigq;
    uint32_t k0, k1;
    uint32_t pad;
    unsigned long long step;
};

struct Phi4EnsArgs {
    float *field;            // [R][Lz][Ly][Lx], replica r at offset r * sites
    const Phi4EnsRec *rec;   // [R]
    int *flags;              // [R] guard flags: set to 1, never cleared, by the step and frames kernels
    double *series;          // [nsteps / every][R][4] = S1, S2, S4, NN, device-visible (pinned host memory);
                             // nullable: no measurements
    int Lx, Ly, Lz;
    int nsteps, every;
    float clampv;
    unsigned long long adv;  // steps every replica has run since the records were written
};

// One replica's frame state, read at the start of a frames launch and written
// back at its end (the host keeps a mirror and uploads it before every launch).
struct Phi4EnsFrameState {
    double dtau, C;  // Δτ of the next frame (the controller's double), noise amplitude
    float T, V;      // stability rule: last step's max phi', running max |phi'| (never rolled back)
    int init;        // T, V are set (else the first frame takes them from its start field)
    int cnt;         // stable frames since the last Δτ change by the controller
    int fired;       // the last frame's firing step, -1 none
    int flag;        // its guard flag
    int exec;        // steps the last launch executed (early exits run fewer than nframes * loops)
    int pad;
};

struct Phi4EnsFrameArgs {
    Phi4EnsFrameState *st;  // [R]
    int *stable;            // [nframes][R] verdicts
    double *dtau;           // [nframes][R] Δτ after the frame
    float *recs;            // [R][3][loops]: M | D | A of the replica's last frame, through its firing step
    int nframes, loops, adapt;
};

// One replica's correlator accumulators: G(t) += g(t), S1 += sum_z S(z), nmeas += 1 per
// measurement, nt = Lz / 2 + 1.  An argument of its own: Phi4EnsArgs is the plain instances' and stays.
struct Phi4EnsCorrArgs {
    double *G;          // [R][nt]
    double *S1;         // [R]
    long long *nmeas;   // [R]
};

constexpr int kPhi4EnsMaxMomenta = 8;  // SQ_PHI4_ENS_MAX_MOMENTA

// The momentum-projected correlator: per replica Gp[m][t] += g_m(t) for the M momenta set
// on the handle and nmeas_p += 1 per measurement.  The twiddle tables are one row per momentum (row m the
// table of n_x / n_y of momentum m, sq_phi4_ens_momentum_table's values), so the kernels need no list of the
// momenta themselves.  corr.G non-null: the zero-momentum accumulators advance as well (`correlate`).
struct Phi4EnsPCorrArgs {
    double *Gp;              // [R][M][nt]
    long long *nmeas_p;      // [R]
    const double *cx, *sx;   // [M][Lx]
    const double *cy, *sy;   // [M][Ly]
    int M;                   // 1 .. kPhi4EnsMaxMomenta
    Phi4EnsCorrArgs corr;    // nullable (G == nullptr)
};

// The dynamic LDS of a launch: the image(s) of the lattice, the launch's
// scratch, then what the launch's measurement keeps behind the scratch.  One
// rule for every launch: two images (one barrier per step instead of two)
// exactly when they fit in kPhi4EnsLdsBytes with the rest, and never for a
// launch that works on the stored field.
enum Phi4EnsLdsKind {
    kPhi4EnsLdsStep,    // the step launches of every sampler: kPhi4EnsScratchBytes behind the image(s)
    kPhi4EnsLdsFrames,  // the frames launches: kPhi4EnsFrameScratchBytes
    kPhi4EnsLdsStored   // moments, slices, pslices, exchange, cluster: one image, kPhi4EnsScratchBytes
};
// The bytes behind the scratch: none without a measurement, else ...
constexpr int phi4_ens_corr_bytes(int Lz) { return 8 * Lz; }    // ens_corr: Lz doubles, the slice sums
// ens_pcorr: 2 Lz doubles (S, then each momentum's A and B in turn: the need does not depend on their number)
constexpr int phi4_ens_pcorr_bytes(int Lz) { return 16 * Lz; }
constexpr int kPhi4EnsClusterSumBytes = 4 * 8;                  // the cluster sums: the per-weight totals
struct Phi4EnsLds {
    int images, bytes;
};
inline Phi4EnsLds phi4_ens_lds(int sites, Phi4EnsLdsKind kind, int behind = 0) {
    const int rest = (kind == kPhi4EnsLdsFrames ? kPhi4EnsFrameScratchBytes : kPhi4EnsScratchBytes) + behind;
    const int images = kind != kPhi4EnsLdsStored && 2 * 4 * sites + rest <= kPhi4EnsLdsBytes ? 2 : 1;
    return Phi4EnsLds{images, images * 4 * sites + rest};
}

// Work-group shape of a lattice of `sites` sites (a multiple of 8): K float4
// quads per lane (1, 2, 4 or 8), T lanes (a multiple of 64, <= 1024).  Every
// launcher and every *_shape_info entry point asks lds() for its layout.
struct Phi4EnsShape {
    int K, T, sites;
    bool pc_ok;  // Lz > 0 and one image fits in the step, frames and pslices launches with momenta
    Phi4EnsLds lds(Phi4EnsLdsKind kind, int behind = 0) const { return phi4_ens_lds(sites, kind, behind); }
};
Phi4EnsShape phi4_ens_shape(int sites, int Lz = 0);

// nsteps steps of every replica in one launch (grid = nrep work-groups).
hipError_t phi4_ens_step_launch(const Phi4EnsArgs &a, int nrep, hipStream_t s);
// nframes frames of every replica in one launch (grid = nrep work-groups); a.series nullable:
// [nframes][R][4] sums of the field after each frame's verdict.  a.nsteps / a.every are not used.
hipError_t phi4_ens_frames_launch(const Phi4EnsArgs &a, const Phi4EnsFrameArgs &f, int nrep, hipStream_t s);
// The two above with one correlator measurement (ens_corr) after each every-th step (a.every >= 1; a.series
// nullable) / after every stable frame of a replica, accumulated in place into c's rows.
hipError_t phi4_ens_step_corr_launch(const Phi4EnsArgs &a, const Phi4EnsCorrArgs &c, int nrep, hipStream_t s);
hipError_t phi4_ens_frames_corr_launch(const Phi4EnsArgs &a, const Phi4EnsFrameArgs &f, const Phi4EnsCorrArgs &c,
                                       int nrep, hipStream_t s);
// One measurement of the stored fields of replicas first .. first + count, accumulating nothing:
// S[r][Lz] slice sums, g[r][nt] (device memory, both non-null).
hipError_t phi4_ens_slices_launch(const Phi4EnsArgs &a, int first, int count, double *S, double *g, hipStream_t s);
// The step and frames launches with one momentum measurement (ens_pcorr) where the correlator launches take
// theirs, after the sums and after the zero-momentum measurement when p.corr is given.  A shape that cannot
// hold momenta (Phi4EnsShape::pc_ok) is hipErrorInvalidValue.
hipError_t phi4_ens_step_pcorr_launch(const Phi4EnsArgs &a, const Phi4EnsPCorrArgs &p, int nrep, hipStream_t s);
hipError_t phi4_ens_frames_pcorr_launch(const Phi4EnsArgs &a, const Phi4EnsFrameArgs &f, const Phi4EnsPCorrArgs &p,
                                        int nrep, hipStream_t s);
// One momentum measurement of the stored fields of replicas first .. first + count, accumulating nothing:
// AB[r][M][Lz][2] projections, g[r][M][nt] (device memory, both non-null); p.Gp, p.nmeas_p, p.corr are not used.
hipError_t phi4_ens_pslices_launch(const Phi4EnsArgs &a, const Phi4EnsPCorrArgs &p, int first, int count, double *AB,
                                   double *g, hipStream_t s);
// nsteps stochastic Heun steps of every replica in one launch (phi4_ens_heun_kernel): per step
// phi' = guard(0.5 (phi + E(E(phi)))), E the step launch's update, both applications with the normals of the
// step's counter, which advances by one.  c, p nullable, at most one of them: the measurements of
// phi4_ens_step_corr_launch / phi4_ens_step_pcorr_launch after each every-th Heun step.  The work-group shape,
// the LDS layout and the argument rules are those of the three step launches.
hipError_t phi4_ens_heun_launch(const Phi4EnsArgs &a, const Phi4EnsCorrArgs *c, const Phi4EnsPCorrArgs *p, int nrep,
                                hipStream_t s);
// nframes frames of Heun steps of every replica in one launch (phi4_ens_heun_frames_kernel): the frames launch
// with every step the Heun step above, the step's record taken of phi' against the step's input (DESIGN.md
// §4.3).  c, p nullable, at most one of them: the measurements of phi4_ens_frames_corr_launch /
// phi4_ens_frames_pcorr_launch after every stable frame.  The work-group shape, the LDS layout and the argument
// rules are those of the three frames launches; the image count selects the instance.
hipError_t phi4_ens_heun_frames_launch(const Phi4EnsArgs &a, const Phi4EnsFrameArgs &f, const Phi4EnsCorrArgs *c,
                                       const Phi4EnsPCorrArgs *p, int nrep, hipStream_t s);
// ---- the Metropolis-adjusted Langevin step (sq_phi4_ens_mala.hip) ----
// The replicas' counters, accumulated in place, and the launch's optional per-step record.
struct Phi4EnsMalaArgs {
    long long *stat;  // [R][3] = proposed, accepted, guard trips (device memory)
    double *rec;      // [nsteps][R][3] = dH, u, verdict (0 rejected, 1 accepted, 2 guard trip), device-visible
                      // (pinned host memory); nullable
};
// nsteps MALA steps of every replica in one launch (phi4_ens_mala_kernel): per step the Euler update of the step
// launch as the proposal, accepted or rejected per replica inside the kernel; the counter advances by one per
// step whatever the verdict.  Every replica's sig must be non-zero (the caller checks: the kernel divides by
// sig^2).  c nullable: the measurement of phi4_ens_step_corr_launch after each every-th step, of the field the
// replica then holds.  The work-group shape, the LDS layout and the argument rules are those of the step launches.
hipError_t phi4_ens_mala_launch(const Phi4EnsArgs &a, const Phi4EnsMalaArgs &w, const Phi4EnsCorrArgs *c, int nrep,
                                hipStream_t s);

// ---- hybrid Monte Carlo trajectories (sq_phi4_ens_hmc.hip) ----
constexpr int kPhi4EnsMaxLeap = 4096;  // leapfrog steps per trajectory
// The replicas' counters, accumulated in place, the trajectory length and the launch's optional record.
struct Phi4EnsHmcArgs {
    long long *stat;  // [R][4] = trajectories, accepted, guard trips, leapfrog steps (device memory)
    double *rec;      // [nsteps][R][4] = dH, u, verdict (0 rejected, 1 accepted, 2 guard trip), L, device-visible
                      // (pinned host memory); nullable
    int nleap;        // 1 .. kPhi4EnsMaxLeap
    int randomize;    // != 0: L = 1 + (o.y nleap >> 32) per trajectory, else L = nleap
};
// nsteps trajectories of every replica in one launch (phi4_ens_hmc_kernel): the Euler update of the step launch as
// the first leapfrog step, L - 1 noise-free steps in displacement form, one Metropolis test; the counter advances
// by one per trajectory whatever L and the verdict.  L = 1 is phi4_ens_mala_launch's step bit for bit.  The
// replica's row of a.field holds the trajectory's start field during the call.  Every replica's sig must be
// non-zero (the caller checks).  c, the work-group shape, the LDS layout and the argument rules: as
// phi4_ens_mala_launch.
hipError_t phi4_ens_hmc_launch(const Phi4EnsArgs &a, const Phi4EnsHmcArgs &w, const Phi4EnsCorrArgs *c, int nrep,
                               hipStream_t s);

// ---- gradient-flow measurements (sq_phi4_ens_flow.hip) ----
constexpr int kPhi4EnsMaxFlowLevels = 4;   // SQ_PHI4_ENS_MAX_FLOW_LEVELS
constexpr int kPhi4EnsMaxFlowSteps = 4096;  // SQ_PHI4_ENS_MAX_FLOW_STEPS

// One replica's flow coefficients: phi4_base_args' expressions of the flow step, its m² and λ; sig = 0.
struct Phi4EnsFlowRec {
    float h, m2, lam6, pad;
};

// The flow of a launch: nlev strictly ascending levels (flow steps), lev[nlev - 1] <= kPhi4EnsMaxFlowSteps, and
// the per-replica, per-level accumulators of the step launch's correlator measurements (nullable without them):
// G[r][l][t] += g(t), S1[r][l] += s1, nmeas[r][l] += 1.
struct Phi4EnsFlowArgs {
    const Phi4EnsFlowRec *rec;  // [R]
    int nlev;
    int lev[kPhi4EnsMaxFlowLevels];
    double *G;          // [R][nlev][nt]
    double *S1;         // [R][nlev]
    long long *nmeas;   // [R][nlev]
};

// What the flow launches ask for beside phi4_ens_shape: the step launch keeps the step launches' layout without
// the correlator and with it, the flowed launch takes the latter, the flow-field launch the former.  stash:
// where the lane's quads wait during a flow inside the step kernel, 0 registers, 1 the replica's row of the
// field in device memory (K = 8: no 32 registers to spare).
struct Phi4EnsFlowShape : Phi4EnsShape {
    int stash;
};
Phi4EnsFlowShape phi4_ens_flow_shape(int sites, int Lz);

// phi4_ens_step_launch with a flow measurement after each every-th step (a.every >= 1): the lane's quads put
// aside, w.lev[nlev - 1] steps of ens_step<K, false> with the replica's flow coefficients on the on-chip copy,
// at each level the four sums to a.series ([nsteps / every][nlev][R][4], nullable) and, corr, one ens_corr
// measurement into w's accumulators; then the quads and the image restored.  Fields, counters and flags are those
// of phi4_ens_step_launch; a.series == nullptr && !corr measures nothing and is hipErrorInvalidValue.
hipError_t phi4_ens_step_flow_launch(const Phi4EnsArgs &a, const Phi4EnsFlowArgs &w, bool corr, int nrep,
                                     hipStream_t s);
// One measurement per level of the stored fields of replicas first .. first + count, which are not written:
// sums[r][l][4], S[r][l][Lz], g[r][l][nt] (device memory, all non-null).  w.G, w.S1, w.nmeas are not used.
hipError_t phi4_ens_flowed_launch(const Phi4EnsArgs &a, const Phi4EnsFlowArgs &w, int first, int count, double *sums,
                                  double *S, double *g, hipStream_t s);
// The stored fields of replicas first .. first + count after nsteps flow steps to out[r][sites] (device memory);
// the stored fields are not written.  Only w.rec is used.
hipError_t phi4_ens_flow_field_launch(const Phi4EnsArgs &a, const Phi4EnsFlowArgs &w, int first, int count,
                                      int nsteps, float *out, hipStream_t s);

// ---- flow measurements in frames and Heun steps (sq_phi4_ens_flow_frames.hip) ----
// What those launches ask for beside phi4_ens_shape.  The frames launches of both schemes keep the frames
// launches' layout without the correlator and with it; the Heun step launch keeps the step launches' as
// phi4_ens_step_flow_launch does.  *_stash: where the un-flowed field waits, 0 registers, 1 the replica's row of
// the field in device memory.  mask: bit 2 scheme + corr set when the frames launch of that scheme (0 Euler,
// 1 Heun) and correlator choice runs on the shape.
struct Phi4EnsFramesFlowShape : Phi4EnsShape {
    int fr_stash, hfr_stash, hs_stash;  // Euler frames, Heun frames, Heun steps
    int mask;
};
Phi4EnsFramesFlowShape phi4_ens_frames_flow_shape(int sites, int Lz);

// phi4_ens_frames_launch (heun: phi4_ens_heun_frames_launch) with a flow measurement behind every frame's
// verdict: a.series ([nframes][nlev][R][4], nullable) takes each level's sums of the field the replica then
// holds, after every frame; corr: one ens_corr measurement per level into w's accumulators after every stable
// frame.  With a.series == nullptr a rolled-back frame runs no flow step.  The simulation is that of the launch
// without the flow, bit for bit.  a.series == nullptr && !corr measures nothing and is hipErrorInvalidValue, as
// is a combination the shape's mask lacks.
hipError_t phi4_ens_frames_flow_launch(const Phi4EnsArgs &a, const Phi4EnsFrameArgs &f, const Phi4EnsFlowArgs &w,
                                       bool corr, bool heun, int nrep, hipStream_t s);
// phi4_ens_step_flow_launch with every step the Heun step of phi4_ens_heun_launch.
hipError_t phi4_ens_heun_flow_launch(const Phi4EnsArgs &a, const Phi4EnsFlowArgs &w, bool corr, int nrep,
                                     hipStream_t s);

// out[5 r ..] = S1, S2, S4, NN, max |phi| of replica first + r's field, r < count.
hipError_t phi4_ens_moments_launch(const Phi4EnsArgs &a, int first, int count, double *out, hipStream_t s);
// out[r] = the 64-bit digest of replica first + r's field, r < count (sq_phi4_ens_digest.hip; include/stochquant.h
// has the definition): field [nrep][sites] and out in device memory, one work-group per replica, nothing written
// but out.  The caller checks the range against its nrep.
hipError_t phi4_ens_digest_launch(const float *field, int sites, int first, int count, unsigned long long *out,
                                  hipStream_t s);
// phi = amp * Philox normal(replica's key, stream 2, site): phi4_init_kernel's field per replica.
hipError_t phi4_ens_init_launch(const Phi4EnsArgs &a, int nrep, float amp, hipStream_t s);

// ---- replica exchange (sq_phi4_ens_exchange.hip) ----
// The Philox stream of the pair test's uniform: counter {0, kPhi4EnsStreamExchange << 24, x lo, x hi} under the
// key of the pair's lower slot.  The fifth stream, behind the four of sq_noise_consts.h.
constexpr uint32_t kPhi4EnsStreamExchange = 4;

// One exchange round: the ladders, the round's counter, the slots' counters and labels, the optional record.
struct Phi4EnsXchgArgs {
    long long *stat;       // [R][2] = attempts, acceptances of the pair (r, r + 1), at r (device memory)
    int *walker;           // [R] the label of the field each slot holds (device memory)
    double *rec;           // [R][5] = Delta, u, verdict, partner, walker after the round: the rows of paired slots
                           // only, device-visible (pinned host memory); nullable
    int nlad;              // slots per ladder, >= 2, divides nrep
    unsigned long long x;  // the round: pairs (l nlad + o + 2 j, + 1), o = x & 1
};
// Pairs of one ladder of nlad slots in round x: (nlad - (x & 1)) / 2.
inline int phi4_ens_xchg_pairs(int nlad, unsigned long long x) { return (nlad - (int)(x & 1ull)) / 2; }
// Round w.x of every ladder in one launch (phi4_ens_exchange_kernel): one work-group per pair, the moments
// launch's work-group shape and LDS layout.  Both rows of a pair are read and written by that work-group alone.
// Every replica's sig must be non-zero (the caller checks: the kernel divides by sig^2).  A round without a pair
// launches nothing and is hipSuccess.  a.flags, a.series, a.nsteps, a.every, a.adv are not used.
hipError_t phi4_ens_exchange_launch(const Phi4EnsArgs &a, const Phi4EnsXchgArgs &w, int nrep, hipStream_t s);

// ---- Swendsen-Wang cluster sweeps (sq_phi4_ens_cluster.hip) ----
// The Philox stream of a sweep's per-site blocks: counter {site, kPhi4EnsStreamCluster << 24, c lo, c hi} under the
// replica's key, words 0 .. 2 the uniforms of the site's forward bonds x, y, z, word 3 the flip bit of the cluster
// the site is the root of.  The sixth stream.
constexpr uint32_t kPhi4EnsStreamCluster = 5;

// One sweep: its counter, the replicas' counters and the optional records of this sweep.
struct Phi4EnsClusterArgs {
    long long *stat;         // [R][5] = sweeps, clusters, flipped clusters, flipped sites, unconverged sweeps
                             // (device memory)
    unsigned char *bonds;    // [R][sites] bits 0 .. 2 = the site's forward bonds x, y, z (device memory); nullable
    int *labels;             // [R][sites] the smallest site index of the site's cluster (device memory); nullable
    unsigned long long c;    // the sweep counter
};
// Sweep w.c of every replica in one launch (phi4_ens_cluster_kernel): one work-group per replica, the moments
// launch's work-group shape and LDS layout.  Only sign bits of a.field change.  Every replica's sig must be
// non-zero (the caller checks: the kernel divides by sig^2).  a.flags, a.series, a.nsteps, a.every, a.adv are not
// used.
hipError_t phi4_ens_cluster_launch(const Phi4EnsArgs &a, const Phi4EnsClusterArgs &w, int nrep, hipStream_t s);

// ---- the sweep with cluster sums (sq_phi4_ens_cluster_improved.hip) ----
// What the sums of one sweep need beside Phi4EnsClusterArgs: an argument of its own, the plain instances keep
// their argument list.
struct Phi4EnsClusterSumArgs {
    double *series;      // [R][8] = I2, I4, Fx, Fy, Fz, Mmax, Mtot, nsat, device-visible (pinned host memory)
    long long *weights;  // [R][sites][7] = M, A_x, B_x, A_y, B_y, A_z, B_z at the root's index, 0 elsewhere (device
                         // memory); nullable
    const double *tab;   // c | s of the unit momentum of x [2][Lx], then y [2][Ly], then z [2][Lz]
                         // (sq_phi4_ens_momentum_table's values, device memory)
    int *park;           // [R][sites] where a lane's labels and its roots' partial sums wait when the shape parks
                         // them (device memory); else not used
};
// Where the labels wait while the image serves as the accumulators: the lane's registers (K <= 4) or device
// memory (K = 8: no 32 registers to spare).  The work-group shape is the plain sweep's, the LDS
// kPhi4EnsClusterSumBytes more.
struct Phi4EnsClusterSumShape : Phi4EnsShape {
    int park;  // 0 registers, 1 device memory
};
Phi4EnsClusterSumShape phi4_ens_cluster_sum_shape(int sites);
// phi4_ens_cluster_launch with the cluster sums of the sweep's labels (the kernel's second kind of instance):
// fields, statistics and records are the plain launch's bit for bit.
hipError_t phi4_ens_cluster_improved_launch(const Phi4EnsArgs &a, const Phi4EnsClusterArgs &w,
                                            const Phi4EnsClusterSumArgs &x, int nrep, hipStream_t s);

}  // namespace sq
