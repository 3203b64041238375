/*
 * stochquant.h -- C ABI of libstochquant.so, the MI355X-native (gfx950) drop-in
 * for SebTanz/StochQuant's Langevin path.
 *
 * The reference has no library API: its host program tauhost.c drives one
 * OpenCL kernel inline from main() (clCreateBuffer / clEnqueueWriteBuffer /
 * clEnqueueNDRangeKernel / clEnqueueReadBuffer, tauhost.c:255-560) and its
 * Python driver talks to that program over argv + stdout (taumain.py:132).
 * Each entry point below names the reference code it replaces.  All functions
 * are extern "C", take plain pointers and sizes, never throw, and return 0 on
 * success or a negative SQ_E* code; sq_last_error() gives the message
 * (thread-local).  A context is not thread-safe; the library owns all device
 * memory, HIP streams and RCCL communicators; host arrays are only copied
 * in/out and never retained.
 */
#ifndef STOCHQUANT_H
#define STOCHQUANT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SQ_ABI_VERSION 6

/* status codes */
#define SQ_OK 0
#define SQ_E_ARG -1      /* invalid argument / unsupported shape */
#define SQ_E_HIP -2      /* HIP runtime error */
#define SQ_E_COMM -3     /* RCCL / halo-exchange error */
#define SQ_E_STATE -4    /* call not valid for this context's model/state */
#define SQ_E_NODEV -5    /* no HIP device */

/* models */
#define SQ_MODEL_QM1D 0  /* the reference's 1-D chain + collective coordinate (tau_kernel.cl:25-175), fp64 */
#define SQ_MODEL_PHI4 1  /* 3-D phi^4 lattice, fp32 (north-star extension) */

/* QM1D sweep order (sq_qm1d_set_ordering) */
#define SQ_ORDER_JACOBI 0   /* default: Jacobi sweep, counter-based Philox noise, one launch per frame */
#define SQ_ORDER_SERIAL 1   /* the reference's serial order: Gauss-Seidel sweep, shared 48-bit LCG
                               (tau_kernel.cl:25-175,269-284 with items run in id order) */

/* halo transport for slab decomposition (SQ_MODEL_PHI4 only) */
#define SQ_COMM_NONE 0      /* one slab, periodic z handled in-kernel */
#define SQ_COMM_LOOPBACK 1  /* nslabs slabs on this device, halos by D2D copies */
#define SQ_COMM_RCCL 2      /* one slab per process, halos by ncclSend/ncclRecv over xGMI */
#define SQ_COMM_P2P 3       /* one slab per process, halos pulled from the neighbours' memory through
                               IPC peer pointers (copy engines, no CUs), cross-process ordering by
                               stream-ordered flag writes/waits; frame collectives through peer
                               memory too (no RCCL); bootstrap: sq_p2p_handle / sq_p2p_connect */

typedef struct sq_params {
    int struct_size;            /* = sizeof(sq_params) */
    int model;                  /* SQ_MODEL_* */
    long long dims[3];          /* QM1D: {N,1,1} (argv[1]); PHI4: global {Lx, Ly, Lz} */
    double deltat;              /* QM1D lattice spacing Δt (argv[2]); PHI4: unused (a = 1) */
    double deltatau;            /* Langevin step Δτ (argv[3]) */
    int pot;                    /* QM1D potID 0 = harmonic, 3 = double well (argv[5]) */
    double C;                   /* noise amplitude (argv[6]) */
    int loops;                  /* Langevin steps per frame (argv[10]) */
    unsigned long long seed;    /* Philox key (tauhost.c:185 seeds from rand()) */
    double m2, lambda;          /* PHI4: V = m2/2 phi^2 + lambda/24 phi^4 */
    double clamp;               /* guard: |v| > clamp -> +-clamp, NaN -> clamp (tau_kernel.cl:119-133); 1000 */
    int device;                 /* HIP device ordinal (argv[7] was an OpenCL platform index) */
    int adapt_dtau;             /* 1: reference Δτ controller in sq_run_frame (tauhost.c:523-541) */
    int comm;                   /* SQ_COMM_* */
    int nranks, rank;           /* SQ_COMM_RCCL / SQ_COMM_P2P: processes, this process' rank */
    int nslabs;                 /* SQ_COMM_LOOPBACK: slabs on this device */
    unsigned char comm_id[128]; /* SQ_COMM_RCCL: ncclUniqueId from sq_comm_unique_id on rank 0 */
} sq_params;

typedef struct sq_perf_t {
    long long steps;            /* Langevin steps executed since the last sq_perf_reset */
    long long site_updates;     /* local sites x steps (ghost-zone recomputation not counted) */
    double step_kernel_ms;      /* sum of hipEvent-timed durations of the step kernels (profiling on) */
    long long step_kernel_launches; /* steps covered by step_kernel_ms (profiling on) */
    double frame_ms;            /* wall time inside sq_run_frame / sq_step (host clock) */
    double halo_bytes;          /* bytes sent by halo exchange */
    long long kernel_launches;  /* step-kernel launches issued (any profiling mode): steps / this =
                                   steps per launch (2 for two-step fused launches; a slab block of
                                   G steps issues its core, rim, pairs and edge launches) */
    long long fused_steps;      /* steps executed inside two-step fused launches */
} sq_perf_t;

/* One operation of a deep-halo block (PHI4 slab decompositions),
 * in an issue order that is also a valid sequential order; each op runs on
 * stream A (interior, stream = 0) or stream B (exchange and rims, stream = 1).
 * See sq_phi4_block_plan. */
#define SQ_OP_EXCHANGE 0       /* after the previous block's SQ_OP_EDGES_DONE, send the ghost-depth edge
                                  planes of the latest field to both z-neighbours, receive their ghosts */
#define SQ_OP_STEP 1           /* step `step` on planes [lo, hi) (and [lo2, hi2) when lo2 < hi2) */
#define SQ_OP_PAIR 2           /* steps `step`, `step`+1 in one launch; output [lo, hi), reads [lo-2, hi+2)
                                  of the field the previous launch group wrote */
#define SQ_OP_WAIT_EXCHANGE 3  /* waits for this block's exchange (and, loopback, the neighbours') */
#define SQ_OP_EDGES_DONE 4     /* the planes the next exchange sends are final (event) */
#define SQ_OP_WAIT_STAGED 5    /* waits until the exchange has copied its edge planes aside (an EXCHANGE
                                  op with lo = 1 sends from that staged copy) */
#define SQ_OP_SIGNAL 6         /* records event slot `lo` on the op's stream */
#define SQ_OP_WAIT 7           /* the op's stream waits for event slot `lo` */
typedef struct sq_block_op {
    int kind;                  /* SQ_OP_* */
    int step;                  /* block-relative index of the (first) step computed */
    int lo, hi, lo2, hi2;      /* local plane ranges; negative = lower ghost zone, >= nz = upper */
    int stream;                /* 0: stream A (interior), 1: stream B (exchange, rims) */
} sq_block_op;

typedef struct sq_ctx sq_ctx;

/* Defaults: QM1D, reference constants (clamp 1000, adapt_dtau 1, comm none). */
void sq_params_init(sq_params *p);
const char *sq_last_error(void);
int sq_abi_version(void);

/* Replaces the OpenCL context/queue/buffer/program/kernel set-up,
 * tauhost.c:196-453 (clGetPlatformIDs ... clSetKernelArg). */
int sq_create(const sq_params *p, sq_ctx **out);
/* Replaces the clRelease* tail, tauhost.c:587-612. */
int sq_destroy(sq_ctx *ctx);

/* QM1D state upload: replaces the initial clEnqueueWriteBuffer calls
 * tauhost.c:319-377 and the per-frame re-upload :550-554.  f, x, xx0 have N
 * doubles; runs is the running-mean count (nr_mem_obj). */
int sq_upload(sq_ctx *ctx, const double *f, const double *x, const double *xx0, double omega, long runs);
/* QM1D state download: replaces clEnqueueReadBuffer of newf/newx/newxx0/omega,
 * tauhost.c:508-515.  Any pointer may be NULL. */
int sq_download(sq_ctx *ctx, double *f, double *x, double *xx0, double *omega, long *runs);
/* QM1D carried stability-scan state (lrgEl/lrgVl, tauhost.c:65-66,350-354)
 * and the Philox step counter; for tests and checkpoint/resume. */
int sq_qm1d_get_scan(sq_ctx *ctx, int *lrgEl, double *lrgVl, unsigned long long *tick);
int sq_qm1d_set_scan(sq_ctx *ctx, int lrgEl, double lrgVl, unsigned long long tick);

/* QM1D sweep order.  SQ_ORDER_SERIAL reproduces the
 * serial semantics of time_dev: Gauss-Seidel order,
 * the last step of a frame Jacobi, the racy stability scan as the in-order
 * scan, the break after the first unstable item, newf / lrgEl / lrgVl / the
 * seed never rolled back.  2 <= N <= 4096.  Its noise is the reference's
 * random() (tau_kernel.cl:269-284) on the shared seed rand1 (tauhost.c:185):
 * sq_qm1d_set_lcg_seed sets it, each frame advances it by the calls it made
 * (sq_qm1d_noise_consumed).  sq_qm1d_inject_noise replaces the next frame's
 * draws with a caller-supplied stream in call order (k = round*(N+1) + item,
 * n >= (N+1)*loops); the seed is then left alone. */
int sq_qm1d_set_ordering(sq_ctx *ctx, int ordering);
int sq_qm1d_set_lcg_seed(sq_ctx *ctx, unsigned long long seed);
int sq_qm1d_get_lcg_seed(sq_ctx *ctx, unsigned long long *seed);
int sq_qm1d_inject_noise(sq_ctx *ctx, const double *xi, size_t n);
int sq_qm1d_noise_consumed(sq_ctx *ctx, unsigned long long *n);

/* One frame = `loops` Langevin steps (one clEnqueueNDRangeKernel + clFinish,
 * tauhost.c:481-483) with the stability read-back :504-505, adoption of the
 * new state on success :506-532, rollback to the frame-start snapshot on
 * failure :533-554 (kept on device, no host round trip), and, if
 * adapt_dtau, the reference Δτ controller :523-541. */
int sq_run_frame(sq_ctx *ctx, int *stable);
/* nframes frames back to back, as nframes sq_run_frame calls (same field,
 * verdicts, Δτ sequence, stability state and last-frame records, bit for
 * bit): stable[f] is frame f's verdict, dtau[f] (nullable) the Δτ after it
 * (what the next frame runs at).  PHI4, one slab without an exchange: the
 * verdict, rollback and Δτ controller run on the device between frames (no
 * host round trip; one read-back per call).  Replaces a caller's loop over
 * tauhost.c:479-560 when no per-frame observable is needed in between. */
int sq_run_frames(sq_ctx *ctx, int nframes, int *stable, double *dtau);

/* PHI4: raw Langevin steps without frame control (the bench's hot path). */
int sq_step(sq_ctx *ctx, int nsteps);
/* PHI4 field I/O of this process' slab(s): nz_local*Ly*Lx floats, z slowest.
 * In multi-rank contexts (SQ_COMM_RCCL / SQ_COMM_P2P, nranks > 1) sq_upload_field,
 * sq_init_field and sq_load_field are collective like sq_step: every rank calls
 * them before its next step call, which agrees across the ranks on whether the
 * field (and so every rank's ghost planes) is known to be guarded. */
int sq_upload_field(sq_ctx *ctx, const float *phi, size_t count);
int sq_download_field(sq_ctx *ctx, float *phi, size_t count);
/* PHI4: phi = amp * Philox normal(seed, stream 2, site), generated on device. */
int sq_init_field(sq_ctx *ctx, float amp);
/* PHI4: phi = amp * (h - 2^23) / 2^23, h = the top 24 bits of splitmix64(i ^ key)
 * for global site index i = (z Ly + y) Lx + x: a field any host reproduces
 * bit for bit without the device's RNG (bench.py's oracle_check starts the
 * noise-off parity protocol from it).  Collective like sq_init_field. */
int sq_init_field_hash(sq_ctx *ctx, double amp, unsigned long long key);
/* PHI4 local slab geometry: nz_local and the global z of its first plane. */
int sq_slab(sq_ctx *ctx, long long *nz_local, long long *z0);
/* PHI4 register tile of the step kernel: out = {lanes per x segment, rows
 * per lane, z planes per wave, float4 segments per lane per row}. */
int sq_phi4_tile(sq_ctx *ctx, int out[4]);
/* PHI4: the step kernel's template instance, as rocprofv3 names it, plus its
 * z-chunk, e.g. "phi4_step_kernel<64, 1, 1, false, true, 3> zc=4". */
int sq_phi4_kernel(sq_ctx *ctx, char *name, size_t cap);
/* PHI4 slab decompositions: the ghost-zone depth G in use (= steps per halo
 * exchange; multi-rank RCCL contexts pick it by timed trial blocks during the
 * first sq_step / sq_run_frame calls) and the depth allocated; 0, 0 for a
 * single periodic slab. */
int sq_phi4_ghost(sq_ctx *ctx, int *active, int *allocated);
/* The rest of a slab decomposition's block schedule: core pairs ahead of
 * each exchange, rims on the exchange stream (1) or the interior stream (0),
 * and whether the timed trials chose them (1) or they are the defaults /
 * SQ_CORE_PAIRS / SQ_RIMS_B (0).  Single periodic slab: 0, 0, 0. */
int sq_phi4_schedule(sq_ctx *ctx, int *core_pairs, int *rims_b, int *tuned);
/* Whether the block's last pair computes the slab's edge planes first, so the
 * next exchange starts before the middle (1), or runs whole (0).  Default: 1,
 * except 0 for one rank's RCCL self-exchange; the timed trials of multi-rank
 * contexts try both; SQ_EDGE_FIRST=0|1 pins it.  Single periodic slab: 0. */
int sq_phi4_edge_first(sq_ctx *ctx, int *edge_first);
/* Where a deep-halo block's exchange runs: in_order 1 = in order on the
 * interior stream between the block's last pair and the next block's first
 * (no core / rim split, no cross-stream event), 0 = on the exchange stream,
 * overlapped with the core pairs.  Default: 1 for one rank's RCCL or P2P
 * self-exchange, 0 for ranks on a link, where the timed trials also try 1;
 * SQ_XCHG_ON_A=0|1 pins it.  kstaged (P2P): the block's last pair also
 * writes the next exchange's staging slot (no staging copy); default: with
 * in_order, SQ_P2P_KSTAGE=0|1 pins it.  Single slab / loopback: 0, 0. */
int sq_phi4_exchange_stream(sq_ctx *ctx, int *in_order, int *kstaged);
/* The launch schedule of one deep-halo block (pure host logic, no device
 * needed; the product's phi4_block executes exactly this list): a slab of nz
 * planes with a ghost zone of `ghost` planes (the exchange depth G) running
 * g <= G steps; fuse2 != 0 runs the steps as two-step pairs, the first
 * core_pairs of them on the ghost-free core ahead of the exchange (0: no
 * core/rim split, the first launch waits for the exchange), their rims on the
 * exchange stream when rims_b != 0; edge_first != 0 computes the last step's
 * edge planes first.  Writes *nops ops (at most cap).  sq_phi4_pick_ghost returns the index of the fastest candidate of the
 * rank-max-reduced per-step times ms[n] (the ghost-depth trial, identical on
 * every rank once the times are reduced). */
int sq_phi4_block_plan(int nz, int ghost, int g, int fuse2, int edge_first, int core_pairs, int rims_b,
                       sq_block_op *ops, int cap, int *nops);
int sq_phi4_pick_ghost(const double *ms, int n);
/* PHI4 frame stability (the heuristic of tau_kernel.cl:135-143 restated for
 * the 3-D lattice).  Every frame records per step j the maximum
 * M_j of phi', the drift increment D_j = |phi' - phi - sigma xi| at the sites
 * attaining it (the largest on ties) and A_j = max |phi'|, reduced over all
 * slabs and ranks (RCCL max); the frame is unstable -- rolled back like a
 * clamp / NaN hit -- at the first step with M_j > T and D_j > V, where T is
 * the previous step's maximum and V the running max |phi| of the steps before
 * (carried across frames and never rolled back, as lrgEl / lrgVl; initialised
 * from the field at the first frame).  sq_phi4_stability returns {T, V}, the
 * step at which the last frame fired (-1: none) and that frame's records
 * (n <= loops); sq_phi4_set_stability sets T and V. */
int sq_phi4_stability(sq_ctx *ctx, double state[2], int *fired_step, float *M, float *D, float *A, int n);
int sq_phi4_set_stability(sq_ctx *ctx, double T, double V);
/* PHI4 observables over this process' slab: out[0] = sum phi, out[1] = sum
 * phi^2, out[2] = max |phi| (double accumulation on device). */
int sq_moments(sq_ctx *ctx, double out[3]);

/* The context's parameters (deltatau = the current, possibly adapted, Δτ). */
int sq_get_params(sq_ctx *ctx, sq_params *out);

/* PHI4 binary checkpoint of this process' slab: <path>
 * is a NumPy .npy float32 array of shape (nz, Ly, Lx); <path>.json holds the
 * lattice dims, z0, the Philox step counter, Δτ and the seed.  Replaces the
 * reference's text end/start file (tauhost.c:91-173,562-581) for 3-D fields.
 * sq_load_field with restore_counters != 0 also restores step and Δτ, and the
 * frame state carried across frames (the stability heuristic's T, V and the Δτ
 * controller's stable-frame count; files without it restart that state). */
int sq_save_field(sq_ctx *ctx, const char *path);
int sq_load_field(sq_ctx *ctx, const char *path, int restore_counters);

/* Δτ (dt_mem_obj, tauhost.c:346,526,540). */
int sq_set_dtau(sq_ctx *ctx, double dtau);
int sq_get_dtau(sq_ctx *ctx, double *dtau);
int sq_get_step(sq_ctx *ctx, unsigned long long *step);
int sq_set_step(sq_ctx *ctx, unsigned long long step);

/* Correlator of the reference's observables: QM1D out[i] = xx0[i] -
 * x[i]*x[mid] (host xavg, tauhost.c:519-521), n <= N.  PHI4: zero-momentum
 * time-slice correlator over z, out[t] = <S(z) S(z+t)>/V, n <= Lz, where
 * S(z) = sum_{x,y} phi over the whole lattice (slab contexts: one RCCL sum
 * all-reduce of the slice sums; collective, every rank must call it). */
int sq_correlator(sq_ctx *ctx, double *out, int n);

/* Profiling of the step kernels on their stream: mode 1 = every launch timed
 * by hipExtLaunchKernel start/stop events (dispatch timestamps, no extra
 * packets); mode 2 = one event pair around each sq_step call (region average,
 * includes inter-kernel gaps); 0 = off.  Read with sq_perf. */
int sq_set_profiling(sq_ctx *ctx, int mode);
int sq_perf(sq_ctx *ctx, sq_perf_t *out);
int sq_perf_reset(sq_ctx *ctx);
/* Joins the context's streams and reports asynchronous errors.  A slab
 * exchange whose gated rim chunks timed out (SQ_E_COMM) is sticky: the
 * field's rim planes are stale, so sq_sync, sq_download_field, sq_step and
 * the frame calls keep failing with it until sq_upload_field / sq_load_field
 * / sq_init_field(_hash) replaces the field. */
int sq_sync(sq_ctx *ctx);
/* PHI4: the step kernel launched most often since the last sq_perf_reset, as
 * its template instance (e.g. "phi4_tb2_kernel<true, false, 1, false, true,
 * false>", the name rocprofv3 prints inside "void sq::(anonymous
 * namespace)::...(sq::Phi4StepArgs)"), its grid in threads and its launch
 * count (0 and "" when nothing ran).  Ties a profiler record to the launch. */
int sq_phi4_launch_info(sq_ctx *ctx, char *name, size_t cap, long long *grid_threads, long long *launches);
/* Identity of the compiled code: "phi4:<16 hex> lib:<16 hex>", the first a
 * hash of the φ⁴ kernels' code object, the second of every object linked. */
const char *sq_build_id(void);
/* Noise amplitude C (argv[6], sigma = C sqrt(2 Δτ), tau_kernel.cl:112) of an
 * open context; C = 0 runs the deterministic drift-only update (bench.py's
 * oracle_check).  Not collective: every rank sets the same C.  SQ_E_ARG for
 * |C| > 1e12, and (PHI4) when the new C breaks the creation-time bound of the
 * guard's fast path at the current Δτ. */
int sq_set_noise(sq_ctx *ctx, double C);
/* PHI4, one slab without an exchange, fused launches: run the next two steps
 * (one fused launch, as sq_step(ctx, 2)) with per-block stamps of the
 * constant 100 MHz clock: out[2b], out[2b+1] = start / end of block b
 * (cap >= blocks of the launch); *nblocks = blocks.  A measurement hook for
 * the launch's ramp, tail and busy fraction (bench.py roofline). */
int sq_phi4_block_stamps(sq_ctx *ctx, unsigned long long *out, int cap, int *nblocks);
/* The same launch's shader-clock counter (s_memtime) at each block's start and
 * end, out[2b], out[2b+1]: with sq_phi4_block_stamps, the clock the launch ran
 * at under the chip's power management (bench.py clock_MHz_measured). */
int sq_phi4_block_clocks(sq_ctx *ctx, unsigned long long *out, int cap, int *nblocks);

/* QM1D replica ensemble: nrep independent chains (SQ_ORDER_JACOBI, Philox
 * noise, fp64) with the same N, Δt, potID, C, loops and adapt_dtau, advanced
 * together, one frame per launch, one work-group per replica.  Replica r
 * behaves exactly -- bit for bit in f, x, xx0, omega, runs, lrgEl, lrgVl, the
 * tick, every frame's verdict and Δτ after every frame -- as a QM1D context
 * created with seed = seeds[r] (seeds == NULL: p->seed + r) and given the same
 * uploads and the same sequence of frame calls: an unstable frame keeps f, x,
 * xx0, omega and runs but still advances the tick by loops and keeps the new
 * lrgEl / lrgVl, and the Δτ controller acts per replica.  Adoption and the
 * controller run on the device, so sq_ens_run_frames issues nframes launches
 * and reads the verdicts back once.  2 <= N <= 4096, potID 0 or 3.  Not
 * covered: SQ_ORDER_SERIAL, chains above 4096 sites, and tauhost.o, whose
 * command line and stdout stay single-chain.
 * Ranges [first, first + count) outside [0, nrep) give SQ_E_ARG.  Arrays hold
 * count rows of N doubles (state) or count entries (scalars); in sq_ens_upload
 * x, xx0, omega and runs may be NULL (zeros), in the getters any pointer may.
 * stable: nframes * nrep verdicts, frame-major (nullable).  sq_ens_correlator:
 * per site i < n <= N the mean over the replicas of xx0[i] - x[i] x[mid] and
 * (err nullable) its standard error sqrt(sum (c_r - mean)^2 / (R (R - 1))), 0
 * for one replica; sums in double in replica order.  sq_ens_perf: steps = the
 * steps the replicas executed, site_updates = steps x N, kernel_launches. */
typedef struct sq_ens sq_ens;
int sq_ens_create(const sq_params *p, int nrep, const unsigned long long *seeds, sq_ens **out);
int sq_ens_destroy(sq_ens *e);
int sq_ens_upload(sq_ens *e, int first, int count, const double *f, const double *x, const double *xx0,
                  const double *omega, const long *runs);
int sq_ens_download(sq_ens *e, int first, int count, double *f, double *x, double *xx0, double *omega, long *runs);
int sq_ens_get_scan(sq_ens *e, int first, int count, int *lrgEl, double *lrgVl, unsigned long long *tick);
int sq_ens_set_scan(sq_ens *e, int first, int count, const int *lrgEl, const double *lrgVl,
                    const unsigned long long *tick);
int sq_ens_get_dtau(sq_ens *e, int first, int count, double *dtau);
int sq_ens_set_dtau(sq_ens *e, int first, int count, const double *dtau);
int sq_ens_run_frames(sq_ens *e, int nframes, int *stable);
int sq_ens_correlator(sq_ens *e, double *mean, double *err, int n);
int sq_ens_perf(sq_ens *e, sq_perf_t *out);

/* PHI4 lattice ensemble: nrep independent periodic lattices of one shape
 * (Lx, Ly, Lz) = p->dims, each with its own seed, Δτ, m², λ and C (all start
 * from p's; sq_phi4_ens_set_params changes them per replica), advanced
 * together by ONE launch per sq_phi4_ens_step call, one work-group per lattice;
 * a lattice stays in registers and LDS from the call's first step to its last
 * and touches device memory only at the call's start and end.  Replica r is
 * bit for bit the SQ_COMM_NONE PHI4 context with the same shape, parameters,
 * seed = seeds[r] (seeds == NULL: p->seed + r), step counter and start field
 * after the same number of sq_step steps, and sq_phi4_ens_init_field gives it
 * that context's sq_init_field.  Step calls are additive: nsteps in one call
 * equal any split of them into several calls.
 * Shapes: Lx in {8, 16, 32, 64}, Ly >= 2, Lz >= 2, Lx Ly Lz <= 32768; comm must
 * be SQ_COMM_NONE; the parameter bound of a PHI4 context (finite, clamp^2
 * finite in fp32, dtau * drift(clamp) < 1e30) holds per replica at creation
 * and in sq_phi4_ens_set_params, which changes nothing when one replica of
 * its range breaks it.  These are SQ_E_ARG before the device is looked for.
 * The guard flag per replica is: 1 when any executed step since the last
 * clear, raw or in a frame, clamped a site or met a NaN (max |phi'| before the
 * guard >= clamp).
 * Frames: sq_phi4_ens_run_frames runs nframes frames of every replica in ONE
 * launch, each replica decided by its own work-group as sq_run_frames decides
 * a context: a frame is p->loops steps (p->loops < 1: SQ_E_ARG here, not at
 * creation), the stability rule on the replica's carried T and V, the
 * rollback to the frame's start on failure, and with p->adapt_dtau the Δτ
 * controller (x 0.95 on failure, / 0.95 after 11 stable frames).  Replica r
 * equals that context frame for frame in verdicts, Δτ, field, T, V and
 * records.  A frame whose rule has fired skips its remaining steps (the
 * verdict is settled); the step counter advances by p->loops per frame either
 * way, and a retried frame draws fresh noise.  stable and dtau hold nframes *
 * nrep entries, frame-major (dtau: Δτ after the frame); series is nullable and
 * holds nframes * nrep * 4 doubles, S1, S2, S4, NN of the field after each
 * frame's verdict (the adopted field, or the frame's start again after a
 * rollback).  nframes == 0 is a no-op.  Afterwards get_params reports the
 * adapted Δτ and sq_phi4_ens_step runs at it; a Δτ set between calls holds
 * from the next frame on and keeps the count of stable frames, as sq_set_dtau.
 * sq_phi4_ens_stability: per replica of the range TV = {T, V}, the firing step
 * of its last frame (-1: none) and the first n <= p->loops per-step records
 * M, D, A of that frame (count rows of n; valid through the firing step, or
 * all p->loops when the rule did not fire; n > 0 before the first frames call
 * is SQ_E_ARG); every output is nullable.  The records are a device buffer of
 * nrep * p->loops * 3 floats from the first frames call on (12 MB at nrep =
 * 1024, loops = 1000).  sq_phi4_ens_set_stability sets T and V and marks the
 * replicas initialised, as sq_phi4_set_stability; otherwise a replica's first
 * frame takes them from its start field, and an upload does not reset them.
 * Ranges [first, first + count) outside [0, nrep) give SQ_E_ARG.  Field rows
 * hold Lz*Ly*Lx floats, z slowest; in set_params / get_params any array may be
 * NULL (left alone / not reported).  sq_phi4_ens_step: with every = k > 0 and
 * series != NULL the kernel records after each k-th step of the call, from
 * the on-chip field, S1 = sum phi, S2 = sum phi^2, S4 = sum phi^4 and NN = sum
 * over sites and mu = x, y, z of phi(x) phi(x + mu) (sites converted to
 * double, products and sums in double): series holds (nsteps / k) * nrep * 4
 * doubles, measurement-major, read back once at the end of the call.
 * sq_phi4_ens_moments: out5 = count rows of {S1, S2, S4, NN, max |phi|} of the
 * current fields.  sq_phi4_ens_flags: the guard flags (flags nullable), then
 * cleared when clear != 0.  sq_phi4_ens_perf: steps = the steps the replicas
 * executed (a frame that exited early counts the steps it ran, not
 * p->loops), site_updates = steps x sites, kernel_launches.
 *
 * sq_phi4_ens_shape_info needs no device and no handle: for dims = {Lx, Ly,
 * Lz} it reports the work-group shape the launchers give such a lattice, from
 * the function they call themselves: out = {K float4 quads per lane, T lanes,
 * LDS images and dynamic LDS bytes of the step launch, the same two of the
 * frames launch, LDS bytes of the moments launch, the LDS limit in bytes}.
 * SQ_E_ARG for exactly the shapes sq_phi4_ens_create refuses. */
typedef struct sq_phi4_ens sq_phi4_ens;
int sq_phi4_ens_shape_info(const int dims[3], int out[8]);
int sq_phi4_ens_create(const sq_params *p, int nrep, const unsigned long long *seeds, sq_phi4_ens **out);
int sq_phi4_ens_destroy(sq_phi4_ens *e);
int sq_phi4_ens_upload(sq_phi4_ens *e, int first, int count, const float *phi);
int sq_phi4_ens_download(sq_phi4_ens *e, int first, int count, float *phi);
int sq_phi4_ens_init_field(sq_phi4_ens *e, float amp);
int sq_phi4_ens_set_params(sq_phi4_ens *e, int first, int count, const double *dtau, const double *m2,
                           const double *lambda, const double *C);
int sq_phi4_ens_get_params(sq_phi4_ens *e, int first, int count, double *dtau, double *m2, double *lambda,
                           double *C);
int sq_phi4_ens_get_step(sq_phi4_ens *e, int first, int count, unsigned long long *step);
int sq_phi4_ens_set_step(sq_phi4_ens *e, int first, int count, const unsigned long long *step);
int sq_phi4_ens_step(sq_phi4_ens *e, int nsteps, int every, double *series);
int sq_phi4_ens_run_frames(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series);
int sq_phi4_ens_stability(sq_phi4_ens *e, int first, int count, double *TV /*[count][2]*/, int *fired, float *M,
                          float *D, float *A, int n);
int sq_phi4_ens_set_stability(sq_phi4_ens *e, int first, int count, const double *T, const double *V);
int sq_phi4_ens_moments(sq_phi4_ens *e, int first, int count, double *out5);
int sq_phi4_ens_flags(sq_phi4_ens *e, int first, int count, int *flags, int clear);
int sq_phi4_ens_perf(sq_phi4_ens *e, sq_perf_t *out);

/* The ensemble's zero-momentum time-slice correlator over z, accumulated over
 * Langevin time inside the resident kernels.  For one replica of shape (Lx,
 * Ly, Lz): V = Lx Ly Lz, nt = Lz / 2 + 1 (integer division).
 *
 * Slice sums: S(z) = sum_{x,y} phi(x, y, z), in double from the fp32 field, in
 * a fixed order that depends on the lattice shape only: the slice's float4
 * quads (x fastest, then y) q = 0 .. Lx Ly / 4 - 1 are dealt to 64 lanes, lane
 * l adds its quads l, l + 64, ... in ascending order to 0.0, each quad as
 * (x + y) + (z + w), and the 64 lane sums are combined by the inclusive-scan
 * sequence of distances 1, 2, 4, 8 within rows of 16 lanes, then row 0 + row 1
 * and row 2 + row 3 onto rows 1 and 3, then row 1's total onto rows 2 and 3;
 * lane 63 holds S(z).  No floating-point atomics.  The bits of S do not depend
 * on nrep, the replica's index, the work-group shape, whether the measurement
 * ran in flight or stand-alone, or how calls were split.
 *
 * One measurement: g(t) = sum_{z=0}^{Lz-1} S(z) S((z + t) mod Lz) for t = 0 ..
 * nt - 1, z ascending from 0.0, every product and every sum rounded once to
 * double (no fused multiply-add); not divided by V.  g(Lz - t) = g(t), so nt
 * values are kept.  s1 = sum_z S(z), z ascending from 0.0.
 *
 * Accumulators, per replica, in device memory, persistent across calls, zero
 * at creation and cleared by sq_phi4_ens_corr_reset only (uploads, set_params,
 * set_step and set_stability leave them alone): G[nt] doubles, S1 one double,
 * nmeas one 64-bit integer.  A measurement does G[t] = G[t] + g(t), S1 = S1 +
 * s1, nmeas += 1, one addition each, so calls split in any way add up to the
 * same bits.
 *
 * sq_phi4_ens_step_corr: as sq_phi4_ens_step(e, nsteps, every, series) for
 * fields, counters, flags and series (series nullable); additionally one
 * measurement after each every-th step of the call (every >= 1, else
 * SQ_E_ARG; an incomplete tail measures nothing, as for series).
 * sq_phi4_ens_run_frames_corr: as sq_phi4_ens_run_frames for verdicts, dtau,
 * fields, T, V, records and series; additionally one measurement of the
 * adopted field after every STABLE frame of a replica; a rolled-back frame
 * measures nothing.  sq_phi4_ens_corr_sums: the raw accumulators of replicas
 * [first, first + count): G count rows of nt, S1 and nmeas count entries; any
 * may be NULL.  sq_phi4_ens_slices: one measurement of the CURRENT fields,
 * accumulating nothing: S count rows of Lz, g count rows of nt; either may be
 * NULL.  sq_phi4_ens_correlator: replica statistics, on the host in double,
 * replicas in index order, only those with nmeas > 0 (*used = how many; none:
 * SQ_E_STATE): c_r(t) = G_r(t) / (nmeas_r V), minus (S1_r / nmeas_r)^2 / (Lz V)
 * when connected != 0 (tauhost's cbar - Lz sbar^2 / V); mean[t] over those
 * replicas and err[t] = sqrt(sum_r (c_r - mean)^2 / (u (u - 1))), 0 for u = 1;
 * n <= nt; err and used may be NULL.  sq_phi4_ens_corr_shape_info (no device,
 * no handle; SQ_E_ARG as sq_phi4_ens_shape_info): out = {LDS images and dynamic
 * LDS bytes of the step launch with the correlator, the same two of the
 * frames launch with it, LDS bytes of the slices launch, nt}. */
int sq_phi4_ens_step_corr(sq_phi4_ens *e, int nsteps, int every, double *series);
int sq_phi4_ens_run_frames_corr(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series);
int sq_phi4_ens_corr_sums(sq_phi4_ens *e, int first, int count, double *G, double *S1, long long *nmeas);
int sq_phi4_ens_corr_reset(sq_phi4_ens *e, int first, int count);
int sq_phi4_ens_slices(sq_phi4_ens *e, int first, int count, double *S, double *g);
int sq_phi4_ens_correlator(sq_phi4_ens *e, int connected, double *mean, double *err, int n, int *used);
int sq_phi4_ens_corr_shape_info(const int dims[3], int out[6]);

/* The same correlator projected on spatial momenta p = (2 pi nx / Lx, 2 pi ny /
 * Ly): C(p, t) = < sum_z Re S_p(z) S_p*(z + t) > / V with S_p(z) = sum_{x,y}
 * phi(x, y, z) e^{i (px x + py y)} = A(z) + i B(z).  Up to
 * SQ_PHI4_ENS_MAX_MOMENTA momenta are set on the handle and measured together,
 * in flight, into accumulators of their own; V, nt as above.
 *
 * Twiddle tables: sq_phi4_ens_momentum_table(L, n, c, s) (host only, no handle,
 * no device) fills, for k = 0 .. L - 1 with j = (n k) mod L, c[k] = cos(a) and
 * s[k] = sin(a) of the host libm at the double a = 2.0 * M_PI * (double)j /
 * (double)L, except where 4 j is a multiple of L: there (c, s) is exactly
 * (1, 0), (0, 1), (-1, 0) or (0, -1).  SQ_E_ARG for L < 2, n outside [0, L) or a
 * null pointer.  The kernels use exactly these tables (cx, sx of (Lx, nx) and
 * cy, sy of (Ly, ny)), uploaded when the momenta are set.
 *
 * sq_phi4_ens_set_momenta: M pairs nxy[m] = {nx, ny}, 0 <= M <=
 * SQ_PHI4_ENS_MAX_MOMENTA, 0 <= nx < Lx, 0 <= ny < Ly, duplicates allowed; a
 * new handle has M = 0.  Every call, with the same list too, zeroes the
 * momentum accumulators of every replica (their layout depends on M); nothing
 * else clears them but sq_phi4_ens_pcorr_reset.  SQ_E_ARG for a bad argument
 * and, whatever M, for a lattice shape the momentum launches cannot hold (see
 * sq_phi4_ens_pcorr_shape_info).  sq_phi4_ens_get_momenta: *M and, nxy given,
 * the M pairs (room for SQ_PHI4_ENS_MAX_MOMENTA pairs).
 *
 * Projections of slice z for momentum m, in double from the fp32 field: the
 * slice's float4 quads are dealt to 64 lanes exactly as for S(z) above (x
 * fastest, then y; lane l takes quads l, l + 64, ... in ascending order).  Quad
 * i holds the sites x0 .. x0 + 3 of row y, y = i / (Lx / 4), x0 = 4 (i mod (Lx /
 * 4)), values p0 .. p3.  Per quad, every product and every sum rounded once to
 * double (no fused multiply-add):
 *   re = (p0 cx[x0] + p1 cx[x0+1]) + (p2 cx[x0+2] + p3 cx[x0+3])
 *   im = (p0 sx[x0] + p1 sx[x0+1]) + (p2 sx[x0+2] + p3 sx[x0+3])
 *   a  = a + (re cy[y] - im sy[y])
 *   b  = b + (re sy[y] + im cy[y])
 * a and b from 0.0; the 64 lane values of a, and of b, are combined by the
 * scan sequence stated for S; lane 63 holds A_m(z) and B_m(z).  The bits depend
 * on the slice's shape and sites only.  For a finite field, A of momentum
 * (0, 0) is S(z) bit for bit and B is +0.0.
 *
 * One measurement: g_m(t) = sum_{z=0}^{Lz-1} [A(z) A(zt) + B(z) B(zt)], zt = (z
 * + t) mod Lz, t = 0 .. nt - 1, z ascending from acc = 0.0 as acc = (acc +
 * A(z) A(zt)) + B(z) B(zt), every product and every sum rounded once; not
 * divided by V.  For (0, 0) this is g(t) above bit for bit.
 *
 * Accumulators, per replica, in device memory, persistent across calls:
 * Gp[M][nt] doubles and one 64-bit nmeas_p, independent of the zero-momentum
 * G, S1, nmeas.  A measurement does Gp[m][t] = Gp[m][t] + g_m(t) and nmeas_p +=
 * 1, so calls split in any way add up to the same bits.
 *
 * sq_phi4_ens_step_pcorr: as sq_phi4_ens_step(e, nsteps, every, series) for
 * fields, counters, flags and series (series nullable); additionally one
 * momentum measurement after each every-th step (every < 1: SQ_E_ARG; M = 0:
 * SQ_E_STATE; an incomplete tail measures nothing).  correlate != 0: G, S1 and
 * nmeas advance as well, exactly as sq_phi4_ens_step_corr would advance them.
 * sq_phi4_ens_run_frames_pcorr: as sq_phi4_ens_run_frames in everything;
 * additionally one measurement of the adopted field after every STABLE frame
 * of a replica (a rolled-back frame measures nothing), and with correlate != 0
 * what sq_phi4_ens_run_frames_corr adds.  sq_phi4_ens_pcorr_sums: G count rows
 * of [M][nt], nmeas count entries; either may be NULL.
 * sq_phi4_ens_pcorr_reset zeroes the range's accumulators.
 * sq_phi4_ens_pslices: one measurement of the CURRENT fields, accumulating
 * nothing: AB count rows of [M][Lz][2] = {A, B}, g count rows of [M][nt];
 * either may be NULL (M = 0: SQ_E_STATE).  sq_phi4_ens_pcorrelator: for each
 * momentum the statistics of sq_phi4_ens_correlator in its unconnected form
 * over the replicas with nmeas_p > 0 (none, or M = 0: SQ_E_STATE), c_r(m, t) =
 * Gp_r[m][t] / (nmeas_p,r V): mean and err rows of n <= nt per momentum.
 * sq_phi4_ens_pcorr_shape_info (no device, no handle): out = {LDS images and
 * dynamic LDS bytes of the step launch with momenta, the same two of the
 * frames launch, LDS bytes of the pslices launch, nt}.  The layout is the
 * correlator launches' with 2 Lz doubles instead of Lz behind the scratch (S,
 * then each momentum's A and B in turn: the need does not depend on M); two
 * images exactly when they fit.  SQ_E_ARG as sq_phi4_ens_shape_info, and where
 * one image, a launch's scratch and 16 Lz bytes exceed the 160 KiB of LDS in
 * any of the three launches: (8, 2, 2048) is refused, (8, 2, 2000) is not. */
#define SQ_PHI4_ENS_MAX_MOMENTA 8
int sq_phi4_ens_momentum_table(int L, int n, double *c, double *s);
int sq_phi4_ens_set_momenta(sq_phi4_ens *e, int M, const int *nxy /*[M][2] = nx, ny*/);
int sq_phi4_ens_get_momenta(sq_phi4_ens *e, int *M, int *nxy);
int sq_phi4_ens_step_pcorr(sq_phi4_ens *e, int nsteps, int every, double *series, int correlate);
int sq_phi4_ens_run_frames_pcorr(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series,
                                 int correlate);
int sq_phi4_ens_pcorr_sums(sq_phi4_ens *e, int first, int count, double *G /*[count][M][nt]*/, long long *nmeas);
int sq_phi4_ens_pcorr_reset(sq_phi4_ens *e, int first, int count);
int sq_phi4_ens_pslices(sq_phi4_ens *e, int first, int count, double *AB /*[count][M][Lz][2]*/,
                        double *g /*[count][M][nt]*/);
int sq_phi4_ens_pcorrelator(sq_phi4_ens *e, double *mean /*[M][n]*/, double *err, int n, int *used);
int sq_phi4_ens_pcorr_shape_info(const int dims[3], int out[6]);

/* A second-order integrator for the ensemble's raw steps: the stochastic Heun
 * scheme with additive noise.  With E_s the update sq_phi4_ens_step applies at
 * step counter s (the replica's coefficients and key, the normals of s, the
 * guard; the noise-off form where C = 0), one Heun step of a replica is
 *   p    = E_s(phi)
 *   e    = E_s(p)          the same counter, hence the same normals
 *   phi' = guard(0.5f * (phi + e))   one fp32 add, one fp32 multiply per site
 * with the guard of the update itself (NaN -> +clamp, else clipped to [-clamp,
 * clamp]); the counter advances by ONE.  This is phi + dtau/2 (F(phi) + F(p)) +
 * sigma xi: its stationary distribution is off at O(dtau^2) where the Euler
 * step's is off at O(dtau).  A replica's guard flag is set when max |p|, max
 * |e| or max |phi'| reached the clamp.  Replica r is bit for bit that
 * composition of sq_step calls on the single context of the same parameters
 * and seed with the counter set back between them; the bits do not depend on
 * nrep, the replica's index or the work-group shape, Heun and Euler calls may
 * alternate on one handle, and calls split in any way give the same bits.
 *
 * sq_phi4_ens_step_heun: nsteps Heun steps of every replica in one launch.
 * every, series: as sq_phi4_ens_step, counting Heun steps.  measure: bit 0
 * adds what sq_phi4_ens_step_corr adds, bit 1 what sq_phi4_ens_step_pcorr
 * adds (M = 0: SQ_E_STATE), both bits what its correlate != 0 adds; with
 * either bit every >= 1, else SQ_E_ARG; other bits: SQ_E_ARG.  nsteps = 0 does
 * nothing.  sq_phi4_ens_perf counts one step (and `sites` site updates) per
 * Heun step, although each does the work of two.  SQ_SCHEME_*: the names
 * of the two integrators (Phi4Ensemble.step's and run_frames' "euler" /
 * "heun").
 *
 * sq_phi4_ens_run_frames_heun: frames of Heun steps.  A Heun frame of replica
 * r is the Euler frame of sq_phi4_ens_run_frames with every step replaced by
 * one Heun step as above; the counter advances by one per Heun step and by
 * `loops` per frame, whatever the verdict.  The step's record (M, D, A):
 *   M = max over sites of phi', signed;
 *   D = the largest, over the sites attaining M, of
 *       fabsf(fmaf(-sigq, xi, phi' - phi)), phi the Heun step's input, xi the
 *       step's normal, sigq = 0 in the noise-off instance: the Heun step's
 *       drift increment dtau/2 (F(phi) + F(p)) where the Euler record has
 *       dtau F(phi).  If the step's input holds a NaN, D's bits are
 *       unspecified; the verdict is not, because the guard flag settles it;
 *   A = max(max |p|, max |e|, max |phi'|), each taken after its guard, hence
 *       <= clamp; the frame's guard flag is A >= clamp at any executed step.
 * Everything else is the Euler frame's, unchanged and shared: fired = M > T &&
 * D > V, then T = M, V = max(V, A); the early exit at the firing step; stable
 * = no guard trip && not fired; the controller on the double dtau; the new
 * coefficients; the snapshot on a stable frame and the reload from it on an
 * unstable one; the frame state (T and V from the start field at a replica's
 * first frame); the records, valid through the firing step
 * (sq_phi4_ens_stability returns the Heun records after a Heun call); `series`
 * after every verdict; the measurements after stable frames only.  measure:
 * bit 0 adds what sq_phi4_ens_run_frames_corr adds, bit 1 what
 * sq_phi4_ens_run_frames_pcorr adds (M = 0: SQ_E_STATE), both bits what its
 * correlate != 0 adds; other bits or a null handle: SQ_E_ARG.  The other
 * argument rules are those of sq_phi4_ens_run_frames.  Euler and Heun frames
 * calls and raw steps of either scheme alternate freely on one handle and
 * share T, V, the controller's count and dtau.  sq_phi4_ens_perf counts one
 * step per executed Heun step.
 *
 * sq_phi4_ens_heun_frames_shape_info (no device, no handle): out = {LDS images
 * and dynamic LDS bytes of the plain Heun frames launch (those of the frames
 * launch in sq_phi4_ens_shape_info), a mask whose bit m is set when measure =
 * m runs on this shape (0xf, or 0x3 for a shape that cannot hold momenta), 0};
 * SQ_E_ARG exactly where sq_phi4_ens_shape_info gives it. */
#define SQ_SCHEME_EULER 0
#define SQ_SCHEME_HEUN 1
int sq_phi4_ens_step_heun(sq_phi4_ens *e, int nsteps, int every, double *series, int measure);
int sq_phi4_ens_run_frames_heun(sq_phi4_ens *e, int nframes, int *stable, double *dtau, double *series, int measure);
int sq_phi4_ens_heun_frames_shape_info(const int dims[3], int out[4]);

/* The Metropolis-adjusted Langevin (MALA) step of the phi^4 ensemble: the
 * Euler update as a proposal, accepted or rejected per replica inside the
 * resident kernel, so that the chain samples exp(-S / T), T = sig^2 / 2h ~
 * C^2, with no step-size bias.  ABI 6: symbols added, none
 * changed.
 *
 * One MALA step of replica r with record (h, m2, lam6, sig, sigq, key) at
 * counter s holding phi.  Everything below is in double, formed from the
 * float32 fields and the float record values converted to double.
 *   1. Proposal: p = E(phi), the Euler update of sq_phi4_ens_step at counter s
 *      with its normals and its guard: bit for bit what a step would store.
 *   2. d(f)_x = sum_nb f - 6 f_x - f_x (m2 + lam6 f_x^2);
 *      S(f) = (3 + m2 / 2) S2(f) - NN(f) + lam6 / 4 S4(f), S2, S4, NN the sums
 *      of sq_phi4_ens_moments.
 *   3. a_x = p_x - phi_x - h d(phi)_x,  b_x = phi_x - p_x - h d(p)_x.
 *   4. dH = [2 h (S(p) - S(phi)) + 1/2 (sum b^2 - sum a^2)] / sig^2, sig the
 *      record's float in double.  dH depends on (phi, p) and the record only,
 *      not on the normals.  The order of summation is fixed (the head of
 *      sq_phi4_ens_mala.hip states it): the same bits on every call, for any
 *      nrep, and for calls split in any way.
 *   5. u = (w + 0.5) 2^-32, w word 0 of Philox4x32-10 at the counter {0,
 *      3 << 24, s lo, s hi} (stream 3, kStreamAccept) under the replica's key.
 *   6. Verdict 2 (guard trip): the proposal's guard touched a site (max |p|
 *      >= clamp): rejected, the replica's guard flag set.  Verdict 1 (accept):
 *      dH <= 0 or u < exp(-dH), the device's double exp: the replica holds p.
 *      Verdict 0 (reject) otherwise, a NaN dH included: the replica keeps phi
 *      bit for bit.
 *   7. The counter advances by one per MALA step, whatever the verdict.
 *
 * Limits.  A replica with sig == 0 (C = 0, or sqrt(2 dtau) C zero in fp32) has
 * no proposal density: any such replica in the handle makes
 * sq_phi4_ens_step_mala fail with SQ_E_STATE before anything is launched.
 * MALA is for thermalised fields: from a cold (zero) field the first proposal
 * is far rougher than equilibrium and nothing is accepted, so thermalise with
 * Euler or Heun steps first.  At fixed dtau the acceptance falls with the
 * volume; choose dtau by sq_phi4_ens_mala_stats.  Momenta, the gradient flow
 * and frames do not run with MALA steps (the frames' stability rule and dtau
 * controller have no meaning under an accept/reject step): measure with
 * sq_phi4_ens_pslices / sq_phi4_ens_flowed between calls.
 *
 * sq_phi4_ens_step_mala: nsteps MALA steps of every replica in one launch.
 * every, series: as sq_phi4_ens_step, counting MALA steps, the sums taken of
 * the field the replica holds after the verdict.  measure: bit 0 adds what
 * sq_phi4_ens_step_corr adds, of that field (one measurement per every-th
 * step, also when the step was rejected), and needs every >= 1, else SQ_E_ARG;
 * other bits: SQ_E_ARG.  rec, nullable: [nsteps][nrep][3] = dH, u, verdict of
 * every step.  nsteps = 0 does nothing (after the argument and state checks).
 * Calls of the three schemes alternate freely on one handle.
 * sq_phi4_ens_perf counts one step per MALA step.
 *
 * sq_phi4_ens_mala_stats: out[r] = {proposed, accepted, guard trips} of
 * replicas first .. first + count, accumulated over every MALA call since
 * creation or the last sq_phi4_ens_mala_reset of the replica (which clears
 * them; the guard FLAG is sq_phi4_ens_flags').  Range errors: SQ_E_ARG. */
#define SQ_SCHEME_MALA 2
int sq_phi4_ens_step_mala(sq_phi4_ens *e, int nsteps, int every, double *series /*[nsteps/every][R][4]*/,
                          int measure /*bit 0: correlate*/, double *rec /*[nsteps][R][3], nullable*/);
int sq_phi4_ens_mala_stats(sq_phi4_ens *e, int first, int count, long long *out /*[count][3]*/);
int sq_phi4_ens_mala_reset(sq_phi4_ens *e, int first, int count);

/* Hybrid Monte Carlo (HMC) trajectories of the phi^4 ensemble: the momentum
 * drawn once, L leapfrog steps, one Metropolis test, inside the resident
 * kernel.  The MALA proposal is one leapfrog step of step
 * length sig = C sqrt(2 dtau) with force -dS / C^2; a trajectory is L of them,
 * so the chain samples exp(-S / C^2) with no step-size bias and moves
 * ballistically, not diffusively, over L sig.  ABI 6: symbols added, none
 * changed.
 *
 * One trajectory of replica r with record (h = dtau, m2, lam6, sig, sigq, key)
 * at counter s holding phi_0.  d(f) is the Euler update's drift, fp32, in the
 * update's operation order; guard is the update's guard (NaN -> +clamp, else
 * clipped to [-clamp, clamp]).
 *   1. Length: L = nleap, or, with randomize != 0,
 *      L = 1 + ((uint64) o.y * nleap >> 32), o the Philox4x32-10 block of the
 *      accept uniform: counter {0, 3 << 24, s lo, s hi} under the replica's
 *      key; o.x stays the uniform, u = (o.x + 0.5) 2^-32.  1 <= nleap <=
 *      SQ_PHI4_ENS_MAX_LEAP.
 *   2. First step: phi_1 = E_s(phi_0), the Euler update of sq_phi4_ens_step at
 *      counter s: MALA's proposal bit for bit (sig xi = sig pi_0).
 *   3. Interior steps, k = 1 .. L - 1 (Stoermer-Verlet in displacement form):
 *      g = guard(fma(2h, d(phi_k), phi_k)), t = phi_k - phi_{k-1} (fp32),
 *      phi_{k+1} = guard(g + t).  2h is the float h doubled: g is the noise-off
 *      update at step size 2h bit for bit.  No noise is drawn, no counter moves.
 *   4. dH = [2 h (S(phi_L) - S(phi_0)) + 1/2 (sum b^2 - sum a^2)] / sig^2,
 *      a = phi_1 - phi_0 - h d(phi_0), b = phi_{L-1} - phi_L - h d(phi_L), in
 *      double with MALA's per-site term, d and S as in the MALA definition above:
 *      the lane's accumulator takes -t(phi_0, phi_1) behind step 1 and
 *      +t(phi_L, phi_{L-1}) behind the last step; the wave sum and the fold in
 *      wave order are MALA's.  For L = 1 this is MALA's dH operation for
 *      operation.  (sig pi_L = -b: dH = H(phi_L, pi_L) - H(phi_0, pi_0), H =
 *      pi^2 / 2 + S / C^2.)
 *   5. Verdict 2 (guard trip) if phi_1, any g or any phi_k reaches clamp in
 *      magnitude; else 1 (accept) if dH <= 0 or u < exp(-dH); else 0.  On 1 the
 *      replica holds phi_L; on 0 or 2 it keeps phi_0 bit for bit; on 2 its guard
 *      flag is set.
 *   6. The counter advances by one per trajectory, whatever L and the verdict.
 * nleap = 1 is sq_phi4_ens_step_mala bit for bit, with or without randomize.
 *
 * Fixed or random lengths.  A fixed L is non-ergodic where omega L sig comes
 * near a multiple of pi for some mode of frequency omega: that mode returns to
 * where it started (free 8x4x4 lattice, dtau 0.02: nleap = 16 fixed gives
 * <phi^2> = 0.185 against the exact 0.1727).  Fixed lengths are for short
 * trajectories and for tests; use randomize for production: the lengths are
 * then uniform on 1 .. nleap, drawn independently of the momenta, which keeps
 * detailed balance and removes the resonances.
 *
 * Limits: MALA's.  A replica with sig == 0 makes sq_phi4_ens_step_hmc fail with
 * SQ_E_STATE before anything is launched; thermalise with Euler or Heun steps
 * first; momenta, the gradient flow and frames do not run with trajectories.
 *
 * sq_phi4_ens_step_hmc: ntraj trajectories of every replica in one launch.
 * every, series, measure: as sq_phi4_ens_step_mala, counting trajectories, of
 * the field held after the verdict.  rec, nullable: [ntraj][nrep][4] = dH, u,
 * verdict, L.  Errors are MALA's, and nleap outside [1, SQ_PHI4_ENS_MAX_LEAP]:
 * SQ_E_ARG; all before any device work.  ntraj = 0 does nothing (after the
 * checks).  Calls of the four schemes alternate freely on one handle.
 * sq_phi4_ens_perf counts one step per trajectory.
 *
 * sq_phi4_ens_hmc_stats: out[r] = {trajectories, accepted, guard trips,
 * leapfrog steps} of replicas first .. first + count since creation or the last
 * sq_phi4_ens_hmc_reset of the replica.  The MALA counters are separate. */
#define SQ_SCHEME_HMC 3
#define SQ_PHI4_ENS_MAX_LEAP 4096
int sq_phi4_ens_step_hmc(sq_phi4_ens *e, int ntraj, int nleap, int randomize, int every,
                         double *series /*[ntraj/every][R][4]*/, int measure /*bit 0: correlate*/,
                         double *rec /*[ntraj][R][4], nullable*/);
int sq_phi4_ens_hmc_stats(sq_phi4_ens *e, int first, int count, long long *out /*[count][4]*/);
int sq_phi4_ens_hmc_reset(sq_phi4_ens *e, int first, int count);

/* Replica exchange (parallel tempering) of the phi^4 ensemble: neighbouring
 * replicas of a ladder swap their fields with a Metropolis test, decided and
 * carried out on the device.  ABI 6: symbols added, none
 * changed.
 *
 * Ladders.  sq_phi4_ens_set_ladder(e, nlad) cuts the R replicas into R / nlad
 * ladders of nlad consecutive slots: 2 <= nlad <= R and R % nlad == 0, else
 * SQ_E_ARG; nlad = 0 switches ladders off, the state at creation.  The rungs'
 * parameters are whatever sq_phi4_ens_set_params gave the slots: the library
 * neither orders nor checks them.  sq_phi4_ens_get_ladder returns nlad.
 *
 * Rounds.  The handle keeps a 64-bit exchange-round counter x, 0 at creation
 * (sq_phi4_ens_exchange_round, sq_phi4_ens_set_exchange_round).  Round x pairs
 * slots (l nlad + o + 2j, l nlad + o + 2j + 1), o = x & 1, for every ladder l
 * and every j with both slots inside the ladder: pairs never cross a ladder
 * boundary.  A round with no pair (nlad = 2, odd x) launches nothing.  x
 * advances by one per round whatever happened.
 *
 * One pair (a, b = a + 1) holding phi_a, phi_b, with the slots' records
 * (h = dtau, m2, lam6, sig, key) as in the MALA definition above.  Everything
 * in double from the float records, no contraction:
 *   S2, S4, NN of each field: sq_phi4_ens_moments' values bit for bit;
 *   beta_r = 2 h_r / (sig_r sig_r), p_r = beta_r (3 + m2_r / 2),
 *   q_r = beta_r (lam6_r / 4) for r = a, b: MALA's S and MALA's 2h / sig^2, so
 *   the test is exact for the densities exp(-beta_r S_r) = exp(-S_r / C_r^2)
 *   that sq_phi4_ens_step_mala and sq_phi4_ens_step_hmc sample;
 *   Delta = (p_a - p_b)(S2_b - S2_a) - (beta_a - beta_b)(NN_b - NN_a) + (q_a - q_b)(S4_b - S4_a),
 *   the three products summed left to right: E_a(phi_b) + E_b(phi_a) -
 *   E_a(phi_a) - E_b(phi_b) with E_r = beta_r S_r;
 *   u = (o.x + 0.5) 2^-32, o the Philox4x32-10 block at counter
 *   {0, 4 << 24, x lo, x hi} under the key of slot a (stream 4);
 *   verdict 1 if Delta <= 0 or u < exp(-Delta) (the device's double exp), else
 *   0, a NaN Delta included.
 * On verdict 1 row a of the field array gets phi_b and row b gets phi_a, bit for
 * bit, and the two slots' walker labels change places; on verdict 0 no field
 * word is written.  Parameters, keys, step counters, guard flags, frame state,
 * every correlator, momentum and flow accumulator and the MALA / HMC counters
 * are left alone in both cases: they belong to the slot, that is to the
 * parameter set, as they do for sq_phi4_ens_upload.
 *
 * State per slot, in device memory: xstat[r] = {attempts, acceptances} of the
 * pair (r, r + 1), zero at creation; walker[r], r at creation
 * (sq_phi4_ens_exchange_stats, sq_phi4_ens_walkers; sq_phi4_ens_exchange_reset
 * clears the counters of a range and, walkers != 0, sets its labels back to
 * the slot index).
 *
 * Limits.  A replica with sig == 0 makes the exchange calls fail with
 * SQ_E_STATE before anything is launched, as no ladder set does.  The test is
 * meaningful only between equilibrium fields, fields drawn from
 * exp(-beta_r S_r): after sq_phi4_ens_step_mala or sq_phi4_ens_step_hmc, or
 * after Euler / Heun steps up to their dtau bias; exchanging fields that are
 * still thermalising samples nothing in particular.
 *
 * sq_phi4_ens_exchange: nrounds consecutive rounds, enqueued back to back, one
 * synchronisation at the end.  rec, nullable: [nrounds][nrep][5] = Delta, u,
 * verdict, partner slot, the walker label the slot holds after the round; both
 * slots of a pair carry the pair's Delta, u and verdict; a slot without a
 * partner in that round has verdict -1, partner -1, Delta = u = 0.
 *
 * sq_phi4_ens_step_hmc_exchange: per round the sq_phi4_ens_step_hmc launch of
 * ntraj trajectories, then one exchange round; all 2 nrounds launches on the
 * handle's stream, one synchronisation at the end.  every > 0 needs
 * ntraj % every == 0 (SQ_E_ARG), so that series ([nrounds ntraj / every][nrep][4])
 * and the correlator measurements are those of the separate calls: a
 * measurement sees the field a slot holds after its trajectory and before the
 * round's exchange.  rec_hmc: [nrounds ntraj][nrep][4], rec_x as rec above, both
 * nullable.  The call is bit for bit the loop { sq_phi4_ens_step_hmc(ntraj, ..);
 * sq_phi4_ens_exchange(1, ..) } in fields, series, records, accumulators,
 * counters, flags, statistics and walkers.  nleap = 1 serves MALA.
 * sq_phi4_ens_perf counts one step per trajectory and every launch.
 *
 * sq_phi4_ens_exchange_shape_info: out = {K, T, LDS bytes, LDS limit} of the
 * exchange launch (one work-group per pair, the moments launch's shape); needs
 * no device; SQ_E_ARG for the shapes sq_phi4_ens_create refuses.
 * All argument and state checks come before any device work; nrounds = 0 does
 * nothing after them. */
int sq_phi4_ens_set_ladder(sq_phi4_ens *e, int nlad);
int sq_phi4_ens_get_ladder(sq_phi4_ens *e, int *nlad);
int sq_phi4_ens_exchange_round(sq_phi4_ens *e, unsigned long long *x);
int sq_phi4_ens_set_exchange_round(sq_phi4_ens *e, unsigned long long x);
int sq_phi4_ens_exchange(sq_phi4_ens *e, int nrounds, double *rec /*[nrounds][R][5], nullable*/);
int sq_phi4_ens_step_hmc_exchange(sq_phi4_ens *e, int nrounds, int ntraj, int nleap, int randomize, int every,
                                  double *series /*[nrounds ntraj/every][R][4]*/, int measure /*bit 0: correlate*/,
                                  double *rec_hmc /*[nrounds ntraj][R][4], nullable*/,
                                  double *rec_x /*[nrounds][R][5], nullable*/);
int sq_phi4_ens_exchange_stats(sq_phi4_ens *e, int first, int count, long long *out /*[count][2]*/);
int sq_phi4_ens_walkers(sq_phi4_ens *e, int first, int count, int *out /*[count]*/);
int sq_phi4_ens_exchange_reset(sq_phi4_ens *e, int first, int count, int walkers);
int sq_phi4_ens_exchange_shape_info(const int dims[3], int out[4]);

/* Swendsen-Wang cluster sweeps of the phi^4 ensemble: the embedded-Ising
 * update of Brower and Tamayo, the non-local move beside the local samplers
 * (DESIGN.md §4.3).  Write phi = s |phi|, freeze |phi| and run one
 * Swendsen-Wang sweep on the signs s, whose couplings are
 * J_xy = beta |phi_x| |phi_y|; S2 and S4 are even in phi, so the sweep is exact
 * for exp(-beta S).  Bonds, clusters and flips are decided on the device, one
 * work-group per lattice.  ABI 6: symbols added, none changed.
 *
 * Sweeps.  The handle keeps a 64-bit cluster-sweep counter c, 0 at creation
 * (sq_phi4_ens_cluster_sweep, sq_phi4_ens_set_cluster_sweep).
 *
 * One sweep of replica r holding phi, with record (h = dtau, sig, key) as in
 * the MALA definition above.  Everything in double from the float field and
 * the float record, no contraction:
 *   1. beta = 2 h / (sig sig): the exchange's beta_r, so the sweep is exact for
 *      the density exp(-beta S) = exp(-S / C^2) that sq_phi4_ens_step_mala and
 *      sq_phi4_ens_step_hmc sample.
 *   2. Site index i = (z Ly + y) Lx + x, the row order of the field array.
 *      o_i is the Philox4x32-10 block at counter {i, 5 << 24, c lo, c hi} under
 *      the replica's key (stream 5).
 *   3. Every site owns its three forward bonds, mu = x, y, z, to the periodic
 *      neighbour j = i + mu^.  With an extent of 2 the forward and the backward
 *      neighbour are the same site: the two bonds are then separate bonds with
 *      separate uniforms, as NN counts that product twice.
 *      t = phi_i phi_j, u_mu = (word mu of o_i + 0.5) 2^-32; the bond is on iff
 *      t > 0 and u_mu >= exp(-(2 beta) t) (the device's double exp).  A NaN t,
 *      t = 0 and t < 0 give off.
 *   4. Clusters are the connected components of the on-bonds; a cluster's
 *      label is the smallest site index in it.
 *   5. The cluster with label l flips iff word 3 of o_l is odd.  A flipped
 *      site has its sign bit toggled; every other bit stays, NaN payloads
 *      included.  No other field word is written.
 *   6. c advances by one per sweep.
 * Parameters, keys, step counters, guard flags, frame state, walkers, all
 * MALA / HMC / exchange statistics and every accumulator are left alone.
 *
 * State per slot, in device memory: cstat[r] = {sweeps, clusters, flipped
 * clusters, flipped sites, unconverged sweeps}, zero at creation
 * (sq_phi4_ens_cluster_stats; sq_phi4_ens_cluster_reset clears a range).  The
 * labelling runs passes of minimum propagation with a bound of sites + 1
 * passes; a lattice that reached the bound would be left unwritten and
 * counted as one unconverged sweep.  The bound is what the plain propagation
 * needs in the worst case, so the count stays 0.
 *
 * Limits.  A replica with sig == 0 makes the calls fail with SQ_E_STATE before
 * anything is launched.  The sweep is exact only as one of the moves of an
 * exact chain: alternate it with sq_phi4_ens_step_mala or sq_phi4_ens_step_hmc
 * on thermalised fields.  Alone it is not ergodic, because |phi| is frozen.
 *
 * sq_phi4_ens_cluster: nsweeps consecutive sweeps of every replica, enqueued
 * back to back, one synchronisation at the end.  bonds, nullable:
 * [nsweeps][nrep][sites] bytes, bits 0 .. 2 = the site's forward bonds x, y, z;
 * labels, nullable: [nsweeps][nrep][sites]; both are device buffers, read back
 * once.
 *
 * sq_phi4_ens_step_hmc_cluster: per round the sq_phi4_ens_step_hmc launch of
 * ntraj trajectories, then one sweep; all 2 nrounds launches on the handle's
 * stream, one synchronisation at the end.  every > 0 needs ntraj % every == 0
 * (SQ_E_ARG); a measurement sees the field after the trajectory and before the
 * round's sweep.  series, rec_hmc: as sq_phi4_ens_step_hmc_exchange; bonds,
 * labels: [nrounds][nrep][sites].  The call is bit for bit the loop
 * { sq_phi4_ens_step_hmc(ntraj, ..); sq_phi4_ens_cluster(1, ..) } in fields,
 * series, records, accumulators, counters, flags and statistics.  nleap = 1
 * serves MALA.  A sweep after each few trajectories together with an exchange
 * round is the loop of the existing calls.  sq_phi4_ens_perf counts one step
 * per trajectory and every launch.
 *
 * sq_phi4_ens_cluster_shape_info: out = {K, T, LDS bytes, LDS limit} of the
 * sweep's launch (one work-group per replica, the moments launch's shape);
 * needs no device; SQ_E_ARG for the shapes sq_phi4_ens_create refuses.
 * All argument and state checks come before any device work; nsweeps = 0 and
 * nrounds = 0 do nothing after them. */
int sq_phi4_ens_cluster(sq_phi4_ens *e, int nsweeps,
                        unsigned char *bonds /*[nsweeps][R][sites], bits 0..2 = x, y, z forward; nullable*/,
                        int *labels /*[nsweeps][R][sites]; nullable*/);
int sq_phi4_ens_cluster_sweep(sq_phi4_ens *e, unsigned long long *c);
int sq_phi4_ens_set_cluster_sweep(sq_phi4_ens *e, unsigned long long c);
int sq_phi4_ens_cluster_stats(sq_phi4_ens *e, int first, int count, long long *out /*[count][5]*/);
int sq_phi4_ens_cluster_reset(sq_phi4_ens *e, int first, int count);
int sq_phi4_ens_cluster_shape_info(const int dims[3], int out[4] /*K, T, LDS bytes, LDS limit*/);
int sq_phi4_ens_step_hmc_cluster(sq_phi4_ens *e, int nrounds, int ntraj, int nleap, int randomize, int every,
                                 double *series /*[nrounds ntraj/every][R][4]*/, int measure /*bit 0: correlate*/,
                                 double *rec_hmc /*[nrounds ntraj][R][4], nullable*/,
                                 unsigned char *bonds /*[nrounds][R][sites], nullable*/,
                                 int *labels /*[nrounds][R][sites], nullable*/);

/* Cluster sums of a sweep: the improved estimators.  With
 * M = sum_C s_C M_C, M_C = sum_{i in C} |phi_i| and independent cluster signs
 * s_C = +-1, the average over the signs is known in closed form:
 *   <(sum phi)^2> = <sum_C M_C^2>,
 *   <(sum phi)^4> = <3 (sum_C M_C^2)^2 - 2 sum_C M_C^4>,
 *   <|sum_i phi_i e^{i p x_i}|^2> = <sum_C |sum_{i in C} |phi_i| e^{i p x_i}|^2>,
 * the susceptibility, the Binder cumulant and the second-moment correlation
 * length, with a variance well below the naive sums'.  The sweep's kernel
 * forms the sums while the labels are on chip.  ABI 6: symbols added, none
 * changed.  The three calls are named sq_phi4_ensemble_*: the family
 * sq_phi4_ens_* is a closed table of 72 entry points
 * (tests/test_phi4_ens_null_boundary.py counts them).
 *
 * One sweep with the sums, of replica r holding phi.  All arithmetic in double
 * from the float field, no contraction:
 *   1. Steps 1 - 6 of the sweep above, unchanged: fields, the sweep counter,
 *      cstat and every other state are bit for bit those of the plain call.
 *   2. Per-site weights, fixed-point integers, so that a cluster's sums are
 *      exact whatever the order of the lanes.  a = |phi_i| in double (of the
 *      field the sweep started from; a flip changes no magnitude).  A site is
 *      saturated when a is NaN, infinite or >= 2^15: q = 0 and all
 *      a_mu = b_mu = 0, and it is counted.  Otherwise q_i = floor(a 2^32) as
 *      int64 and, per axis mu = x, y, z with (c, s) =
 *      sq_phi4_ens_momentum_table(L_mu, 1) and k the site's coordinate on that
 *      axis, a_mu,i = rint((a c[k]) 2^32), ties to even, and b_mu,i the same
 *      with s[k]: the product is rounded once in double, the scaling by 2^32
 *      is exact.  Saturated sites take part in bonds and labels as ever.
 *   3. Per cluster C with label l, as int64: M_C = sum q_i, A_mu,C = sum a_mu,i,
 *      B_mu,C = sum b_mu,i.  At most 32,768 sites: |sum| < 2^62.
 *   4. Per replica and sweep a record of 8 doubles.  With m_C = (double)M_C
 *      2^-32, alpha, beta likewise of A, B:
 *        I2 = sum_C m_C^2, I4 = sum_C (m_C^2)^2,
 *        F_mu = sum_C alpha_mu,C^2 + sum_C beta_mu,C^2 for mu = x, y, z,
 *        Mmax = max_C m_C, Mtot = (double)(sum_C M_C) 2^-32,
 *        nsat = the number of saturated sites.
 *      An unconverged sweep writes eight zeros except nsat = -1 (and no sums).
 *      Every sum over clusters runs over the roots in the kernel's fixed order
 *      (lane, then the kernel's fold), the same bits from run to run; against
 *      another order it is within n_clusters 2^-52 relative.  Mmax, Mtot and
 *      nsat are exact.
 *
 * sq_phi4_ensemble_cluster_improved: sq_phi4_ens_cluster with series
 * [nsweeps][nrep][8] = I2, I4, F_x, F_y, F_z, Mmax, Mtot, nsat (required) and
 * weights, nullable: [nsweeps][nrep][sites][7] = M, A_x, B_x, A_y, B_y, A_z,
 * B_z at the root's index, 0 elsewhere.
 * sq_phi4_ensemble_step_hmc_cluster_improved: sq_phi4_ens_step_hmc_cluster with
 * cseries [nrounds][nrep][8] (required) and weights [nrounds][nrep][sites][7].
 * Checks and errors are the plain calls': a replica with sig == 0 is
 * SQ_E_STATE, and nothing is launched on a bad argument.
 * sq_phi4_ensemble_cluster_improved_shape_info: out = {K, T, LDS bytes, LDS limit,
 * park} of that launch; park = 1: the labels wait in device memory while the
 * LDS image serves as the accumulators (K = 8), 0: in registers.  Needs no
 * device. */
int sq_phi4_ensemble_cluster_improved(sq_phi4_ens *e, int nsweeps, double *series /*[nsweeps][R][8]*/,
                                 unsigned char *bonds /*[nsweeps][R][sites], nullable*/,
                                 int *labels /*[nsweeps][R][sites], nullable*/,
                                 long long *weights /*[nsweeps][R][sites][7] int64: M, A_x, B_x, A_y, B_y, A_z, B_z at
                                                      the root's index, 0 elsewhere; nullable*/);
int sq_phi4_ensemble_step_hmc_cluster_improved(sq_phi4_ens *e, int nrounds, int ntraj, int nleap, int randomize, int every,
                                          double *series /*[nrounds ntraj/every][R][4]*/,
                                          int measure /*bit 0: correlate*/,
                                          double *rec_hmc /*[nrounds ntraj][R][4], nullable*/,
                                          unsigned char *bonds /*[nrounds][R][sites], nullable*/,
                                          int *labels /*[nrounds][R][sites], nullable*/,
                                          double *cseries /*[nrounds][R][8]*/,
                                          long long *weights /*[nrounds][R][sites][7], nullable*/);
int sq_phi4_ensemble_cluster_improved_shape_info(const int dims[3], int out[5] /*K, T, LDS bytes, LDS limit, park*/);

/* Checkpoints of the phi^4 ensemble, and the field digest they rest on
 * (DESIGN.md §4.3).  ABI 6: symbols added, none changed; named
 * sq_phi4_ensemble_* as the cluster sums' calls are.  The contract: a run that
 * saves, ends and resumes in a new process returns the bits of the run that
 * never stopped.
 *
 * The field digest.  With
 *   mix(x):  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;
 *            x *= 0x94D049BB133111EB;  x ^= x >> 31          (uint64, wrapping)
 * replica r's digest is
 *   D_r = sum over sites i = 0 .. sites-1 of mix((uint64(i) << 32) | bits32(phi_r[i]))   mod 2^64,
 * i the site's index in the replica's row (z slowest, sq_phi4_ens_download's
 * order) and bits32 the float's IEEE pattern: -0.0, every NaN payload and the
 * infinities are told apart.  A wrapping integer sum is exact in any order, so
 * the kernel (sq_phi4_ens_digest.hip: one work-group per replica, 16-byte
 * loads, a wave reduction, LDS across waves, one 8-byte store) and the host
 * agree bit for bit.  digest(bytes), used below, is the same sum over a byte
 * string read as little-endian 32-bit words, the last one zero-padded.
 * sq_phi4_ensemble_digest: out[r] = D of replica first + r, r < count; it
 * reads the fields and changes nothing.
 *
 * A checkpoint named <path> is three little-endian files:
 *   <path>        NumPy .npy v1.0: the magic "\x93NUMPY", bytes 1 and 0, the
 *                 header's length as uint16, the header
 *                 "{'descr': '<f4', 'fortran_order': False, 'shape': (R, Lz, Ly, Lx), }"
 *                 padded with spaces so that the data starts on a multiple of
 *                 64 bytes, its last byte '\n'; then R Lz Ly Lx float32 in C
 *                 order.  np.load(path) is sq_phi4_ens_download's array.  A
 *                 reader accepts exactly this header.
 *   <path>.state  the per-replica tables ("sections"), raw, each starting on
 *                 an 8-byte boundary, zero bytes between them and up to the
 *                 file's end, which is a multiple of 8.
 *   <path>.json   one JSON object with exactly these keys, no byte behind its
 *                 closing brace:
 *     "format": "stochquant-phi4-ensemble", "version": 1,
 *     "dims": [Lx, Ly, Lz], "R", "loops", "adapt_dtau" (0 or 1),
 *     "clamp_bits": the double's IEEE pattern as an unsigned decimal,
 *     "exchange_round", "cluster_sweep": unsigned 64-bit decimals,
 *     "ladder": slots per ladder, 0 none,
 *     "momenta": [[nx, ny], ...], "flow_levels": [n_1, ...],
 *     "flow_eps_bits", "flow_m2_bits", "flow_lambda_bits": patterns (a NaN m2
 *       or lambda means "the replica's own"),
 *     "clamp", "flow_eps", "flow_m2", "flow_lambda": decimal copies, null
 *       when not finite; informative only, never read,
 *     "field_digest": [D_0, ..., D_{R-1}],
 *     "field_bytes", "state_bytes": the sizes of the other two files,
 *     "state_digest": digest(<path>.state),
 *     "meta_digest": digest of the little-endian bytes of the uint64 words
 *       version, Lx, Ly, Lz, R, loops, clamp_bits, adapt_dtau, exchange_round,
 *       cluster_sweep, ladder, M, nx_1, ny_1, ..., F, n_1, ..., flow_eps_bits,
 *       flow_m2_bits, flow_lambda_bits, field_bytes, state_bytes, state_digest,
 *       D_0 .. D_{R-1}, the number of sections, every section's offset in the
 *       table's order (negative values as two's complement),
 *     "sections": [{"name", "dtype", "shape", "offset"}, ...].
 *   Integers are JSON integers (no fraction, no exponent); strings are plain
 *   ASCII without escapes; a key appears once.
 *
 * The sections, with nt = Lz / 2 + 1, M momenta, F flow levels (dtype, shape):
 *   seed, step                      <u8 [R]
 *   dtau, m2, lambda, C             <f8 [R]
 *   flags                           <i4 [R]       the guard flags
 *   frame_dtau, frame_C             <f8 [R]       the frame state ...
 *   frame_T, frame_V                <f4 [R]
 *   frame_init, frame_cnt, frame_fired, frame_flag, frame_exec   <i4 [R]
 *   frame_records                   <f4 [R][3][loops]   M | D | A of the last frame; optional: there
 *                                                 once a frames call has run
 *   corr_G <f8 [R][nt], corr_S1 <f8 [R], corr_nmeas <i8 [R]
 *   pcorr_G <f8 [R][M][nt]          exactly when M > 0
 *   pcorr_nmeas                     <i8 [R]
 *   flow_G <f8 [R][F][nt], flow_S1 <f8 [R][F], flow_nmeas <i8 [R][F]   exactly when F > 0
 *   mala_stats <i8 [R][3], hmc_stats <i8 [R][4]   optional: there once the sampler has run
 *   exchange_stats <i8 [R][2], walkers <i4 [R], cluster_stats <i8 [R][5]
 * A table that was never allocated reads as zeros; it is written as an absent
 * section and reads as zeros after the load.  Any other name is refused.
 *
 * Not saved, by decision: the records of the last call that the handle merely
 * holds for its caller (series, MALA / HMC / exchange / cluster records, bond
 * and label dumps, cluster weights); scratch and derived tables (twiddles,
 * parked labels, the *_tmp buffers, the device records, which are rebuilt from
 * the parameters); and sq_phi4_ens_perf, which restarts at zero.
 *
 * sq_phi4_ensemble_save synchronises the stream, reads and writes; the handle
 * goes on bit for bit as one that never saved.  Each file is written under a
 * temporary name in the same directory (<file>.tmp.<pid>.<count>, never shared
 * by two calls), flushed to the disk and renamed into place, and the directory
 * is flushed; the .json last; no temporary is left behind.  A torn set (files
 * of two saves, as two handles saving to one path at one time can leave) is
 * detected by the sizes and digests and refused, not repaired.
 *
 * sq_phi4_ensemble_load, fields_only == 0: dims, R, loops, clamp and
 * adapt_dtau must be the handle's (SQ_E_ARG naming the first that is not).
 * Everything is validated before the handle is touched: the JSON complete and
 * strict, the version, the section table (names, dtypes, shapes, offsets
 * inside the file and not overlapping), the sizes, the .npy header, the
 * host-recomputed digests, every replica's parameters by
 * sq_phi4_ens_create's bound, momenta, flow levels and ladder by the setters'
 * own rules.  A refused load (SQ_E_ARG) changes nothing.  After the upload the
 * digest kernel runs on the device copy; a mismatch is SQ_E_HIP.  Seeds come
 * from the file.  fields_only != 0: only dims and R must match; only the field
 * rows are uploaded (and digest-checked), nothing else changes.
 *
 * sq_phi4_ensemble_checkpoint_info needs no device and no handle: info =
 * {version, Lx, Ly, Lz, R, loops, adapt_dtau, number of sections}, *clamp
 * (nullable) the clamp.  verify != 0 also opens the other two files and runs
 * every check of the load that needs no handle. */
int sq_phi4_ensemble_digest(sq_phi4_ens *e, int first, int count, unsigned long long *out /*[count]*/);
int sq_phi4_ensemble_save(sq_phi4_ens *e, const char *path);
int sq_phi4_ensemble_load(sq_phi4_ens *e, const char *path, int fields_only);
int sq_phi4_ensemble_checkpoint_info(const char *path, int verify, long long info[8], double *clamp /*nullable*/);

/* Gradient-flow measurements of the phi^4 ensemble: the sums and the
 * time-slice correlator taken of a smoothed copy of a replica's field, inside
 * the resident kernel.  ABI 6: symbols added, none changed.
 *
 * Flow parameters, set once per handle (sq_phi4_ens_set_flow): a step eps > 0,
 * 1 .. SQ_PHI4_ENS_MAX_FLOW_LEVELS strictly ascending levels 0 <= n_1 < ... <
 * n_F <= SQ_PHI4_ENS_MAX_FLOW_STEPS (flow steps), and optionally a flow mass
 * m2 and coupling lambda shared by all replicas (NULL: replica r flows with
 * its own m2 / lambda; m2 = lambda = 0 is the lattice heat equation).
 *
 * Flow coefficients of replica r, derived on the host with the expressions of
 * a context's step coefficients: h = (float)eps, m2 = (float)m2, lam6 =
 * (float)((double)(float)lambda / 6.0), sig = 0.  They are re-derived whenever
 * sq_phi4_ens_set_params changes what they depend on and are held to the
 * parameter bound of sq_phi4_ens_create with (clamp, eps, m2, lambda, C = 0):
 * a sq_phi4_ens_set_flow or sq_phi4_ens_set_params call that would break it
 * for one replica returns SQ_E_ARG and changes nothing.
 *
 * Flowed field at level j: the noise-off site update of sq_phi4_ens_step (the
 * full guard, the handle's clamp) applied n_j times to a copy of the replica's
 * current field with those coefficients; no noise is drawn and no counter
 * advances.  Bit for bit what an ensemble with C = 0, dtau = eps and those m2,
 * lambda holds after sq_phi4_ens_upload of the field and sq_phi4_ens_step(n_j).
 * Level 0 is the field itself; the levels are reached in one pass of n_F steps.
 * A measurement at a level is the existing one of the flowed field: the four
 * sums of sq_phi4_ens_step's series, and S(z), g(t), s1 of the correlator
 * above, in their stated orders.
 *
 * The flow does not touch the simulation: after any call with it the fields,
 * the step counters, the guard flags (a clamp hit DURING THE FLOW sets none),
 * dtau, T and V, and the plain correlator and momentum accumulators are bit
 * for bit those of the same call without it.
 *
 * sq_phi4_ens_set_flow: nlevels = 0 turns the flow off (levels may be NULL).
 * Every successful call zeroes the flow accumulators of every replica.
 * sq_phi4_ens_get_flow: *nlevels (required) and, where given, eps, the levels
 * (room for SQ_PHI4_ENS_MAX_FLOW_LEVELS) and m2 / lambda, NaN for "each
 * replica's own".
 * sq_phi4_ens_step_flow: as sq_phi4_ens_step for fields, counters and flags
 * (Euler steps).  every >= 1 (else SQ_E_ARG); after each every-th step one
 * measurement per level: the four sums to series[rec][level][replica][4]
 * (nullable; an incomplete tail measures nothing) and, correlate != 0, one
 * correlator measurement per level added to the flow accumulators, per replica
 * and level G[nt] += g, S1 += s1, nmeas += 1, one addition each.  They persist
 * across calls and are cleared by sq_phi4_ens_fcorr_reset and
 * sq_phi4_ens_set_flow only.  The plain accumulators of sq_phi4_ens_corr_sums
 * do NOT advance: level 0 is the unflowed measurement.  No flow set:
 * SQ_E_STATE.
 * sq_phi4_ens_flowed: one measurement per level of the STORED fields of the
 * range, accumulating nothing and leaving the fields alone: sums[count][F][4],
 * S[count][F][Lz], g[count][F][nt], each nullable.
 * sq_phi4_ens_flow_field: the stored fields after nsteps flow steps, 0 <=
 * nsteps <= SQ_PHI4_ENS_MAX_FLOW_STEPS, to phi[count][sites]; eps, m2 and
 * lambda of sq_phi4_ens_set_flow are used, the levels are not; the stored
 * fields are untouched.
 * sq_phi4_ens_fcorr_sums: the raw flow accumulators, G[count][F][nt],
 * S1[count][F], nmeas[count] (the levels of a replica share their count), each
 * nullable.  sq_phi4_ens_fcorr_reset zeroes the range's.
 * sq_phi4_ens_fcorrelator: the rule of sq_phi4_ens_correlator level by level
 * through the same host code, mean[F][n], err[F][n] (nullable), n <= nt.
 * sq_phi4_ens_flowed, _flow_field, _fcorr_sums and _fcorrelator without a flow
 * set: SQ_E_STATE.
 * sq_phi4_ens_flow_shape_info (no device, no handle; SQ_E_ARG as
 * sq_phi4_ens_shape_info): out = {LDS images and dynamic LDS bytes of
 * sq_phi4_ens_step_flow without the correlator (the plain step launch's),
 * the same two with it (the correlator step launch's), the LDS bytes of the
 * sq_phi4_ens_flowed launch, where the un-flowed field waits during a flow
 * inside the step kernel (0 = registers, 1 = the replica's row in device
 * memory)}.
 *
 * sq_phi4_ens_step_flow_heun: sq_phi4_ens_step_flow with every step the Heun
 * step of sq_phi4_ens_step_heun: one measurement per level after each every-th
 * Heun step, series[nsteps / every][F][R][4], the same argument rules and early
 * returns (every < 1: SQ_E_ARG; no flow set: SQ_E_STATE; neither series nor
 * correlate: the plain Heun call; an incomplete tail measures nothing).
 * sq_phi4_ens_run_frames_flow: the frames call of `scheme` (SQ_SCHEME_EULER:
 * sq_phi4_ens_run_frames, SQ_SCHEME_HEUN: sq_phi4_ens_run_frames_heun; another
 * value: SQ_E_ARG) with the flow measurement behind every frame's verdict.
 * series (nullable, [nframes][F][R][4]): after EVERY frame the F levels' sums
 * of the field the replica then holds, the adopted field after a stable frame,
 * the frame's start field again after a rollback; with level 0 among the
 * levels that row is bit for bit the series of the frames call itself.
 * correlate != 0: after every STABLE frame one correlator measurement per
 * level added to the flow accumulators; a rolled-back frame adds nothing, and
 * with series == NULL it runs no flow step.  The plain correlator and momentum
 * accumulators stay at rest.  series == NULL and correlate == 0: the plain
 * frames call of that scheme.  No flow set: SQ_E_STATE; the other argument
 * rules are those of sq_phi4_ens_run_frames (loops >= 1, nframes == 0 does
 * nothing); a refused call changes nothing.  The paragraph "The flow does not
 * touch the simulation" covers both calls, for frames also stable[], dtau[],
 * the controller's count and the step records of sq_phi4_ens_stability.
 * sq_phi4_ens_frames_flow_shape_info (no device, no handle; SQ_E_ARG as
 * sq_phi4_ens_shape_info): out[0], out[1] = LDS images and dynamic LDS bytes
 * of sq_phi4_ens_run_frames_flow without the correlator (either scheme: the
 * frames launch's layout), out[2], out[3] = the same with it (the correlator
 * frames launch's), out[4] = the images of sq_phi4_ens_step_flow_heun without
 * the correlator (the plain step launch's layout) | with it << 8, out[5] = its
 * LDS bytes with the correlator (the correlator step launch's), out[6] = where
 * the un-flowed field waits (0 = registers, 1 = the replica's row in device
 * memory): bit 0 Euler frames, bit 1 Heun frames, bit 2 Heun steps, out[7] = a
 * mask, bit 2 scheme + (correlate != 0) set when sq_phi4_ens_run_frames_flow
 * runs that combination on the shape (a lacking one is SQ_E_ARG there; every
 * legal shape has all four).
 *
 * Out of scope for now: a flow together with the momentum measurements.  There
 * is no entry point for it (the Python binding refuses it before any library
 * call); sq_phi4_ens_flowed between calls serves those users. */
#define SQ_PHI4_ENS_MAX_FLOW_LEVELS 4
#define SQ_PHI4_ENS_MAX_FLOW_STEPS 4096
int sq_phi4_ens_set_flow(sq_phi4_ens *e, double eps, int nlevels, const int *levels,
                         const double *m2 /*NULL: each replica's own*/, const double *lambda /*likewise*/);
int sq_phi4_ens_get_flow(sq_phi4_ens *e, double *eps, int *nlevels, int *levels, double *m2, double *lambda);
int sq_phi4_ens_step_flow(sq_phi4_ens *e, int nsteps, int every, double *series /*[nsteps/every][F][R][4]*/,
                          int correlate);
int sq_phi4_ens_flowed(sq_phi4_ens *e, int first, int count, double *sums /*[count][F][4]*/,
                       double *S /*[count][F][Lz]*/, double *g /*[count][F][nt]*/);
int sq_phi4_ens_flow_field(sq_phi4_ens *e, int first, int count, int nsteps, float *phi /*[count][sites]*/);
int sq_phi4_ens_fcorr_sums(sq_phi4_ens *e, int first, int count, double *G /*[count][F][nt]*/,
                           double *S1 /*[count][F]*/, long long *nmeas /*[count]*/);
int sq_phi4_ens_fcorr_reset(sq_phi4_ens *e, int first, int count);
int sq_phi4_ens_fcorrelator(sq_phi4_ens *e, int connected, double *mean /*[F][n]*/, double *err, int n, int *used);
int sq_phi4_ens_flow_shape_info(const int dims[3], int out[6]);
int sq_phi4_ens_step_flow_heun(sq_phi4_ens *e, int nsteps, int every, double *series /*[nsteps/every][F][R][4]*/,
                               int correlate);
int sq_phi4_ens_run_frames_flow(sq_phi4_ens *e, int nframes, int *stable /*[nframes][R]*/,
                                double *dtau /*[nframes][R]*/, double *series /*[nframes][F][R][4], nullable*/,
                                int correlate, int scheme /*SQ_SCHEME_EULER or SQ_SCHEME_HEUN*/);
int sq_phi4_ens_frames_flow_shape_info(const int dims[3], int out[8]);

/* RCCL bootstrap: rank 0 creates the id, the caller distributes it (e.g. via
 * torch.distributed) into sq_params.comm_id of every rank. */
int sq_comm_unique_id(unsigned char out[128]);

/* SQ_COMM_P2P bootstrap: every rank exports one handle blob (IPC handles of
 * its staging buffer, mailbox and collective slots, plus its rank and the
 * lattice it was created for); the caller all-gathers the blobs in rank order
 * (e.g. torch.distributed.all_gather_object) and passes all of them to
 * sq_p2p_connect, which validates and maps them.  Steps, frames and the
 * correlator of a P2P context fail with SQ_E_STATE until connected.  Every
 * rank must run the same sequence of steps (the exchanges pair up by count). */
#define SQ_P2P_HANDLE_BYTES 512
int sq_p2p_handle(sq_ctx *ctx, unsigned char out[SQ_P2P_HANDLE_BYTES]);
int sq_p2p_connect(sq_ctx *ctx, const unsigned char *handles, int nranks); /* nranks * SQ_P2P_HANDLE_BYTES */

/* Device queries / self-tests used by tests and bench (no reference analogue). */
int sq_device_count(int *n);
int sq_selftest_normals(int device, unsigned long long seed, unsigned int stream,
                        unsigned long long quad0, unsigned long long step, float *out, size_t nquads);
int sq_selftest_dpp(int device, float *out64x2);
/* DPP cross-wave stress: mode 0 every wave rotates (wave_ror/rol:1), 1 even waves
 * run the records' row_shr/row_bcast wave-max scan while odd waves rotate, 2 every
 * wave does both, 3 as 1 without row_bcast; errs64[lane] = wrong rotated values. */
int sq_selftest_dpp_mix(int device, int mode, int blocks, int iters, unsigned int *errs64);
int sq_selftest_philox(int device, const unsigned int ctr[4], const unsigned int key[2], unsigned int out[4]);
int sq_copy_bandwidth(int device, size_t bytes, int iters, double *gbps);
/* The serial order's draws of one full launch from `seed` on the device:
 * words t1>>16, t2>>16, the seed after each call, xi ((N+1)*loops each).
 * generator 1 = the grid-wide generator the frames use, 0 = the one-block
 * generator it falls back to from the first exceptional call. */
int sq_selftest_lcg(int device, unsigned long long seed, int N, int loops, unsigned int *w1,
                    unsigned int *w2, unsigned long long *seeds, double *xi, int generator);
/* y[i] = f(x[i]) on the device with the serial order's float transcendentals
 * (glibc's algorithms, csrc/sq_glibcf.h): fn 0 logf, 1 cosf, 2 tanhf. */
int sq_selftest_libm(int device, int fn, const float *x, float *y, long long n);
/* The device's Box-Muller factors for every 23-bit argument m (4 x 2^23 floats,
 * csrc/sq_rng.h): out[m] = sqrt(-2 ln u), out[2^23 + m] = sqrt(-log2 u),
 * out[2*2^23 + m] = cos(t), out[3*2^23 + m] = sin(t), u = 2 - [1.m], t = [1.m]
 * revolutions.  A device normal is one fp32 product of two entries. */
int sq_selftest_bm_tables(int device, float *out);

#ifdef __cplusplus
}
#endif
#endif /* STOCHQUANT_H */
