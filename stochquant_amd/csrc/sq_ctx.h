// sq_ctx.h -- the context behind the C ABI (include/stochquant.h) and the
// helpers its source files share: sq_core.cpp, sq_comm.cpp, sq_phi4_*.cpp,
// sq_qm1d_host.cpp, sq_ens.cpp, sq_diag.cpp.  Not installed.
//
// sq_ctx is composed of one state struct per subsystem; each struct names the
// file that allocates and releases its members (release_* next to the
// allocation, called by sq_destroy).
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/stochquant.h"
#include "sq_internal.h"

namespace sq {

inline int fail(int code, const std::string &msg) { return set_error(code, msg); }

}  // namespace sq

#define SQ_HIP(expr)                                                                             \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return sq::fail(SQ_E_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));        \
    } while (0)

#define SQ_NCCL(expr)                                                                            \
    do {                                                                                         \
        ncclResult_t r_ = (expr);                                                                \
        if (r_ != ncclSuccess)                                                                   \
            return sq::fail(SQ_E_COMM, std::string(#expr) + ": " + ncclGetErrorString(r_));      \
    } while (0)

#define SQ_NCCLW(c, expr)                                                                        \
    do {                                                                                         \
        int rc_ = sq::nccl_settle((c), (expr), #expr);                                           \
        if (rc_ != SQ_OK) return rc_;                                                            \
    } while (0)

namespace sq {

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
    }
};

struct Slab {
    float *buf[2] = {nullptr, nullptr};  // padded ping-pong
    float *snap = nullptr;               // frame-start snapshot (interior planes) = snap_pad + gpad planes
    float *snap_pad = nullptr;           // its allocation, padded like buf[]: three-buffer device frames
                                         // rotate the three (phi4_frames_dev)
    int nz = 0;
    long long z0 = 0;
    hipStream_t sA = nullptr, sB = nullptr;
    hipEvent_t evC = nullptr;                 // C: the block's halo exchange done
    hipEvent_t evE = nullptr;                 // E: the block's output edge planes (what the next exchange sends) done
    float *stage = nullptr;                   // 2 G planes (x stage_slots): the staged copy of the edge planes an exchange sends
    hipEvent_t evS = nullptr;                 // S: the staged copy is complete (the field's edges may change)
    std::vector<hipEvent_t> evk;              // the block plan's SIGNAL / WAIT slots (kPlanSlots)
};

struct EvPair {
    hipEvent_t a, b;
};

// SQ_COMM_P2P: the words of a rank's mailbox its neighbours
// and peers write with stream-ordered flag writes; every value is a sequence
// number that only grows, so a wait is ">= this exchange / collective".
constexpr int kMbStagedFromDn = 0;  // the lower neighbour's staged edge planes of exchange e are complete
constexpr int kMbStagedFromUp = 1;  // ... the upper neighbour's
constexpr int kMbAckFromDn = 2;     // the lower neighbour has finished reading our staged copies (teardown)
constexpr int kMbAckFromUp = 3;     // ... the upper neighbour
constexpr int kMbColl = 16;         // + q: rank q's contribution to collective k is in our slot q
// staged copies per slab: P2P double-buffers them by exchange parity
inline size_t stage_slots(int comm) { return comm == SQ_COMM_P2P ? 2 : 1; }
// polls of the P2P hand-shake wave before it gives up (s_sleep 2 between: ~1-2 s)
constexpr unsigned int kHandshakePolls = 1u << 24;
constexpr int kMbWords = 1024;
constexpr int kP2pMaxRanks = kMbWords - kMbColl;
constexpr unsigned int kP2pMagic = 0x53513250u;  // "SQ2P"
// RCCL halo communicator: blocks per send/recv kernel (ncclConfig_t.maxCTAs)
constexpr int kRcclMaxCtas = 0;

struct Peer {  // a rank's buffers as this process addresses them
    float *stage = nullptr;
    unsigned int *mbox = nullptr;
    unsigned char *coll = nullptr;
    bool mapped = false;  // opened through IPC (closed by sq_destroy)
};

constexpr int kPlanSlots = 16;            // events per slab the plan's SIGNAL / WAIT ops name
constexpr int kRimSlot = kPlanSlots - 1;  // the rims of the block are done
constexpr int kA = 0, kB = 1;

// ---- sq_qm1d_host.cpp ----
struct Qm1dHost {
    int N = 0;
    double *qf[2] = {nullptr, nullptr}, *qx[2] = {nullptr, nullptr}, *qxx0[2] = {nullptr, nullptr};
    int qcur = 0;
    sq::Qm1dState *qst = nullptr;
    double *qscr[3] = {nullptr, nullptr, nullptr};  // N > kQm1dRegMaxN: fs, xs, ds of Qm1dArgs
    // N <= kQm1dRegMaxN, Jacobi frames: the precomputed tables of Qm1dArgs (om, xi, tcl, dd)
    double *qom = nullptr, *qdd = nullptr;
    float *qxi = nullptr, *qtcl = nullptr;
    double omega = 0;
    long runs = 0;
    int lrgEl = 0;
    double lrgVl = 0;
    hipStream_t qstream = nullptr;
};

// ---- sq_qm1d_host.cpp: the serial order (SQ_ORDER_SERIAL), LCG state and per-frame buffers ----
struct Qm1dSerialHost {
    int order = SQ_ORDER_JACOBI;
    unsigned long long lcg_seed = 0;  // rand1 (tauhost.c:185), advanced by the calls each frame makes
    bool inject_pending = false;       // g_xi holds a caller-supplied stream for the next frame
    unsigned long long consumed = 0;   // random() calls of the last serial frame
    long long g_calls = 0, g_hist = 0, g_loops = 0; // capacities
    double *g_xc = nullptr;  // potID 3: x_cl and ddPot(x_cl) of every (step, site), 2 (N+2) loops
    void *g_cand = nullptr;  // serial scan candidates per step
    int *g_flags = nullptr;  // per-step "candidates ready" flags, compared with gs_tag
    int gs_tag = 0;
    double *g_xi = nullptr, *g_om = nullptr, *g_hist_buf = nullptr, *g_nfp = nullptr;
    uint32_t *g_w1 = nullptr, *g_w2 = nullptr;
    unsigned long long *g_seeds = nullptr;
    unsigned long long *g_lcg_scr = nullptr;  // grid-wide LCG generator scratch (sq::kLcgScratch words)
    sq::Qm1dGsState *g_st = nullptr;
};

// ---- sq_phi4_create.cpp: the lattice, its slabs and launch shapes ----
struct Phi4Lattice {
    int Lx = 0, Ly = 0;
    long long Lz = 0;
    sq::Phi4Geom geom{};
    int zc = 8;
    int gz = 1;    // active ghost-zone depth (planes) of slab decompositions = steps per halo exchange
    int gpad = 1;  // allocated ghost planes on either side of each slab (gz <= gpad)
    double *dtune = nullptr;
    std::vector<Slab> slabs;
    int cur = 0;
    bool field_finite = true;  // every plane of the current field has been through the guard (or
                               // came from sq_init_field); false after a caller's upload / load
    bool fin_sync = false;     // multi-rank: field_finite changed locally; the next step call
                               // agrees on it across ranks first (ghost planes come from neighbours)
    double *dacc = nullptr;
    double *dpart = nullptr;       // moments: per-block partials (sq::kMomBlocks x 4)
    double *dslice = nullptr;      // correlator: slice sums of the global lattice (Lz), allocated once
    unsigned int *dmax = nullptr;  // [0] max |phi| bits, [1] ordered max phi
    int tbz = 0;                    // two-step fused launches: > 0 on; planes per block when pinned
    bool tbz_pin = false;           // SQ_FUSE2_Z pinned the planes per block
    int tb_minz = 4;                // fewest planes per block of a fused launch (SQ_TB2_MINZ, an experiment)
    int tb_blocks = 512;            // otherwise: blocks per launch aimed at (two per CU)
    // slab paths: the fused launches that run beside an exchange (the core
    // pairs, the middle pair after EDGES_DONE) aim at fewer blocks: the
    // exchange's kernels hold a few CUs, and a full one-round grid then leaves
    // its last blocks for a second round (core pair 43-45 us vs 33)
    int tb_blocks_xchg = 416;
};

// ---- sq_phi4_steps.cpp: the deep-halo block schedule and its variants ----
struct Phi4Schedule {
    bool g_auto = false, g_tuned = false;  // ghost depth chosen by timed trial blocks (phi4_autotune)
    bool k_auto = true;                    // ... and the core pairs (unless SQ_CORE_PAIRS pins them)
    bool edge_first = true; // deep-halo blocks: last step's edge planes first (SQ_EDGE_FIRST=0|1 pins it)
    bool diag_no_xwait = false;  // SQ_DIAG_NO_XWAIT: timing diagnostics only (results wrong)
    bool diag_no_ewait = false;  // SQ_DIAG_NO_EWAIT: no EDGES_DONE event at all (timing only, results wrong)
    bool p2p_kernel_handshake = true;  // P2P: the hand-shake as one wave (SQ_P2P_STREAMOPS=1: stream flag ops)
    bool ef_auto = true;    // the timed pick also tries the other edge_first (unless SQ_EDGE_FIRST pins it)
    int core_pairs = 1;     // deep-halo blocks: fused pairs of the core run ahead of the exchange (0: none)
    bool rims_b = false;    // ... and their rims run on the exchange stream (block_plan)
                            // (SQ_CORE_PAIRS pins; multi-rank runs time 1, 2, 4 on the real link)
    // EDGES_DONE as the stop event of the pair before it (SQ_EDGES_STOPEV=1):
    // hipExtLaunchKernel binds the event to the dispatch itself instead of a
    // marker packet behind it on stream A (each marker leaves a 5-7 us bubble)
    bool edges_stopev = false;
    // gated pair 0 (SQ_SLAB_GATE=1; default off, slower: DESIGN.md §8.0): K = 1 blocks run the core pair and
    // the rim pair as ONE launch whose thin rim chunks wait in-kernel for the
    // exchange (Phi4StepArgs::gate), no WAIT_EXCHANGE hop and no small rim grid
    bool slab_gate = false;
    unsigned int *gate_word = nullptr;  // fine-grained: stream B writes ++gate_seq behind each exchange
    unsigned int gate_seq = 0;
    int *gate_err = nullptr;
    // sticky: a gated rim chunk timed out, so the field's rim planes are stale;
    // every call that would use the field fails until a new field is uploaded
    // or initialised (gate_check / gate_reset)
    bool gate_failed = false;
    // single slab (SQ_TB2_RUN=1): a call's pairs as ONE resident launch
    // (sq_phi4_run.hip); run_flags: one epoch word per block, run_base the
    // epoch every block has reached (gate_err bit 2: a march wait gave up)
    bool tb_run = false;
    unsigned int *run_flags = nullptr;
    int run_nflags = 0;
    unsigned int run_base = 0;
    // P2P, SQ_P2P_KSTAGE=1: the last pair of a deep-halo block writes the next
    // exchange's staging slot itself and counts its blocks into kstage_ctr
    // (phi4_tb2_stage_kernel); the exchange's hand-shake waits for kstage_n
    // instead of the EDGES_DONE event plus a staging copy.  kstage_pending:
    // the slot holds the current field's edges (dropped when anything else
    // writes the field); evE_stale: EDGES_DONE was not recorded behind that
    // pair, so an exchange of the old form records it first
    // P2P, SQ_XCHG_ON_A=1: the exchange (staging, hand-shake, pull) runs on the
    // interior stream in order, between a block's last pair and the next
    // block's first (no core / rim split, no cross-stream event or spin)
    bool xchg_on_a = false;
    bool a_auto = true;   // multi-rank timed pick also tries it (unless SQ_XCHG_ON_A pins it)
    int kstage_env = -1;  // SQ_P2P_KSTAGE if set; else kstage follows xchg_on_a
    unsigned int *kstage_ctr = nullptr;
    unsigned int kstage_n = 0;
    bool kstage_pending = false, evE_stale = false;
    unsigned long long *stamps_next = nullptr;  // sq_phi4_block_stamps: the next fused launch's block stamps
    unsigned long long *dstamps = nullptr;
    int stamps_cap = 0, stamps_blocks = 0;
};

// ---- sq_phi4_frames.cpp ----
struct Phi4Frames {
    int *flag = nullptr;
    bool in_frame = false;  // phi4_frame: the step kernels raise the guard flag
    float *snap_next = nullptr;  // phi4_frame: the next fused launch writes its input here (Phi4StepArgs::snap)
    // stability heuristic of phi4 frames (tau_kernel.cl:135-143):
    // per-step device records of the current frame, kStabSlots words per step
    unsigned long long *st_md = nullptr;
    unsigned int *st_a = nullptr;
    // phi^4 frames: st_md | st_a | flag in ONE device block (one memset, one
    // read-back per frame) and its pinned host mirror
    void *frame_rec = nullptr;  // two record sets of frame_bytes (device frames alternate them)
    void *frame_cur = nullptr;  // the active set (st_md, st_a, flag point into it)
    int rec_set = 0;
    void *frame_host = nullptr;
    size_t frame_bytes = 0;
    bool frame_rec_zero = true;  // frame_rec is (or is queued to be) all zero: the next frame skips its memset
    unsigned long long frame_step0 = 0;  // Philox step of the frame's first step
    bool stab_init = false;              // T, V set from the field at the first frame
    float stab_T = 0, stab_V = 0;        // carried across frames, never rolled back (as lrgEl / lrgVl)
    int stab_fired = -1;                 // step of the last frame at which the rule fired, -1 none
    std::vector<float> rec_M, rec_D, rec_A;  // the last frame's per-step records
    // device frame control (phi4_frames_dev): controller state and its pinned
    // mirror, the last frame's folded records (M | D | A, loops floats each) and
    // per-frame verdicts / Δτ of a batch (fr_cap entries, device and pinned)
    sq::FrameCtl *ctl = nullptr, *ctl_host = nullptr;  // ctl: two states (frame f reads ctl[f&1], writes the other)
    float *rec_dev = nullptr;
    int *fr_stable = nullptr, *fr_stable_h = nullptr;
    double *fr_dtau = nullptr, *fr_dtau_h = nullptr;
    int fr_cap = 0;
    bool dev_frames = false;  // the current frame's launches read {h, sig, sigq} from ctl_cur->coef
    sq::FrameFoldArgs fold_next{};  // the next fused launch takes the previous frame's end (phi4_frames_dev)
    sq::RecClear clr_next{};        // ... and the launch after it clears that frame's record set
    bool clr_armed = false;
    // three-buffer device frames (phi4_frames_dev): buffers of the batch, the
    // frame's launch index, the controller state the launches read
    bool tri = false;
    float *tri_bufs[3] = {nullptr, nullptr, nullptr};
    int frame_tk = 0;
    // the host's guess of the current frame's buffer roles (FrameCtl::bs / bw0 /
    // bw1 if every earlier frame of the batch was stable); SQ_FRAME_SPEC=0: off
    int spec_bs = 0, spec_bw0 = 1, spec_bw1 = 2;
    bool tri_spec = true;
    bool clr_first = false;         // ... armed by the next launch even without a fold (a batch's frame 0)
    sq::FrameCtl *ctl_cur = nullptr;
};

// ---- sq_comm.cpp ----
struct P2pHost {
    ncclComm_t comm = nullptr;
    // SQ_COMM_P2P: mailbox, collective slots (2 parities x nranks x coll_cap
    // bytes) and every rank's buffers as mapped here (own ones at [rank])
    unsigned int *mbox = nullptr;
    unsigned char *coll = nullptr;
    size_t coll_cap = 0;
    std::vector<Peer> peers;
    bool p2p_ready = false;
    unsigned int xchg_seq = 0, coll_seq = 0;  // exchanges / collectives issued so far
};

// ---- sq_core.cpp: profiling ----
struct ProfHost {
    long long ev_extra_steps = 0;   // profiling mode 1: steps beyond the first in timed launches
    // profiling: 0 off, 1 per launch (hipExtLaunchKernel dispatch timestamps),
    // 2 one event pair around every sq_step call on the step-kernel stream
    int profiling = 0;
    std::vector<EvPair> evpool;
    size_t ev_used = 0;
    long long region_steps = 0;
    sq_perf_t perf{};
    // step-kernel launches since the last sq_perf_reset by kernel id (template
    // instance + grid, sq::phi4_kernel_id_name): sq_phi4_launch_info names the
    // dominant one, which bench.py matches against its committed PMC record
    std::map<uint64_t, long long> kstat;
};

}  // namespace sq

struct sq_ctx : sq::Qm1dHost, sq::Qm1dSerialHost, sq::Phi4Lattice, sq::Phi4Schedule, sq::Phi4Frames, sq::P2pHost,
                sq::ProfHost {
    sq_params p{};
    int dev = 0;
    double dtau = 0;
    int stab_cnt = 0;
    unsigned long long step = 0;  // Philox step counter (attempted steps)
};

namespace sq {

inline bool is_phi4(const sq_ctx *c) { return c->p.model == SQ_MODEL_PHI4; }

// one slab per process, ranks of a job (RCCL or peer pointers)
inline bool per_rank(int comm) { return comm == SQ_COMM_RCCL || comm == SQ_COMM_P2P; }

inline hipError_t wait_seq(hipStream_t s, unsigned int *word, unsigned int seq) {
    return hipStreamWaitValue32(s, word, seq, hipStreamWaitValueGte, 0xFFFFFFFFu);
}

inline size_t plane_floats(const sq_ctx *c) { return (size_t)c->Lx * (size_t)c->Ly; }

// Local plane 0 of buffer k (the ghost zone is the c->gpad planes on either side).
inline float *plane0(const sq_ctx *c, const Slab &s, int k) { return s.buf[k] + (size_t)c->gpad * plane_floats(c); }

// sq_core.cpp
int flush_events(sq_ctx *c);
int ev_take(sq_ctx *c, EvPair **out);
int ev_begin(sq_ctx *c, hipStream_t s, EvPair **out);
void release_events(sq_ctx *c);

// sq_comm.cpp
int nccl_settle(sq_ctx *c, ncclResult_t r, const char *what);
int rank_allreduce(sq_ctx *c, void *d, size_t n, P2pRed red, hipStream_t st);
int rccl_init(sq_ctx *c);
int p2p_alloc(sq_ctx *c);
bool p2p_drain(sq_ctx *c);
void p2p_close_peers(sq_ctx *c);
void release_p2p(sq_ctx *c);
void release_rccl(sq_ctx *c);

// sq_phi4_create.cpp
int create_phi4(sq_ctx *c);
void release_gate(sq_ctx *c);
void release_slabs(sq_ctx *c);
void release_lattice(sq_ctx *c);

// sq_phi4_plan.cpp
std::vector<sq_block_op> block_plan(int nz, int G, int g, bool fuse2, bool edge_first, int kc, bool rims_b);
int gate_pattern(const std::vector<sq_block_op> &ops);

// sq_phi4_steps.cpp
bool kstage_on(const sq_ctx *c);
int gate_check(sq_ctx *c, bool read_device);
int gate_reset(sq_ctx *c);
int fin_agree(sq_ctx *c);
int phi4_steps(sq_ctx *c, int n);
int phi4_join(sq_ctx *c);

// sq_phi4_frames.cpp
int alloc_frame_records(sq_ctx *c);
void release_frames(sq_ctx *c);

// sq_qm1d_host.cpp
double host_intconst(int pot);
int create_qm1d(sq_ctx *c);
int qm1d_frame(sq_ctx *c, int *stable);
void release_qm1d(sq_ctx *c);
void release_qm1d_serial(sq_ctx *c);

}  // namespace sq
