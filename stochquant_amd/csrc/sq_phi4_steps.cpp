// sq_phi4_steps.cpp -- PHI4 step launches: the single-slab paths (one step,
// a fused pair, a resident march) and the deep-halo block of slab
// decompositions (exchange on stream B or in order on stream A, core / rim
// split, gated rims, staged last pair), the timed schedule pick, sq_step.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "sq_ctx.h"

using namespace sq;

namespace {

sq::Phi4StepArgs phi4_base_args(sq_ctx *c, const Slab &s, int in_buf) {
    sq::Phi4StepArgs a{};
    a.in = s.buf[in_buf];
    a.out = s.buf[in_buf ^ 1];
    a.Lx = c->Lx;
    a.Ly = c->Ly;
    a.nz = s.nz;
    a.gz = c->gpad;
    a.zg0 = s.z0;
    a.Lzg = c->Lz;
    const float h = (float)c->dtau;
    a.h = h;
    a.m2 = (float)c->p.m2;
    a.lam6 = (float)((double)(float)c->p.lambda / 6.0);
    a.sig = (float)(sqrt(2.0 * (double)h) * c->p.C);  // sigma = C*sqrt(2 dtau) (tau_kernel.cl:112, a = 1)
    a.sigq = (float)(sqrt(2.0 * (double)h) * c->p.C * sq::kSqrt2Ln2);  // for the kernels' box_muller_q normals
    a.fin = c->field_finite ? 1 : 0;
    a.clampv = (float)c->p.clamp;
    a.k0 = (uint32_t)c->p.seed;
    a.k1 = (uint32_t)(c->p.seed >> 32);
    a.s_lo = (uint32_t)c->step;
    a.s_hi = (uint32_t)(c->step >> 32);
    a.nw0 = sq::phi4_noise_consts(a.k0, a.k1, c->step);
    a.nw1 = sq::phi4_noise_consts(a.k0, a.k1, c->step + 1);
    a.flag = c->in_frame ? c->flag : nullptr;  // the guard flag only feeds a frame's rollback
    a.st_md = nullptr;
    a.st_a = nullptr;
    a.dcoef = (c->in_frame && c->dev_frames) ? c->ctl_cur->coef : nullptr;
    if (c->in_frame && c->st_md != nullptr) {
        const size_t k = (size_t)(c->step - c->frame_step0) * sq::kStabSlots;
        a.st_md = c->st_md + k;
        a.st_a = c->st_a + k;
    }
    if (c->tri && c->in_frame) {  // the kernel picks in / out from the controller (FrameCtl::bs/bw0/bw1)
        a.buf0 = c->tri_bufs[0];
        a.buf1 = c->tri_bufs[1];
        a.buf2 = c->tri_bufs[2];
        a.tctl = c->ctl_cur;
        a.tk = c->frame_tk++;
        // the guess: the roles every earlier frame of the batch being stable
        // gives (phi4_frames_dev keeps them); kernels that can start on it
        // check it against the controller once their first loads are out
        const int bi = a.tk == 0 ? c->spec_bs : ((a.tk & 1) ? c->spec_bw0 : c->spec_bw1);
        const int bo = a.tk == 0 ? c->spec_bw0 : ((a.tk & 1) ? c->spec_bw1 : c->spec_bw0);
        a.in = c->tri_bufs[bi];
        a.out = c->tri_bufs[bo];
        a.tspec = c->tri_spec ? 1 : 0;
    }
    return a;
}

// Update local planes of the given chunks: chunk k = [zlo + k*zstep, +zc) clipped to zhi.
int phi4_launch_range(sq_ctx *c, const Slab &s, int in_buf, hipStream_t st, int zlo, int zhi,
                      int zstep, int zc, int nzc, int periodic, bool timed) {
    if (nzc <= 0 || zhi <= zlo) return SQ_OK;
    sq::Phi4StepArgs a = phi4_base_args(c, s, in_buf);
    a.zlo = zlo;
    a.zhi = zhi;
    a.zstep = zstep;
    a.zc = zc;
    a.nzc = nzc;
    a.periodic = periodic;
    sq::phi4_fill_units(a, c->geom);
    EvPair *e = nullptr;
    if (timed && c->profiling == 1) {
        int rc = ev_take(c, &e);
        if (rc) return rc;
    }
    uint64_t kid = 0;
    SQ_HIP(sq::phi4_step_launch(a, c->geom, st, e ? e->a : nullptr, e ? e->b : nullptr, &kid));
    c->perf.kernel_launches += 1;
    c->kstat[kid] += 1;
    return SQ_OK;
}

// Planes [lo, hi) in chunks of c->zc.
int phi4_launch_span(sq_ctx *c, const Slab &s, int in_buf, hipStream_t st, int lo, int hi, bool timed) {
    if (hi <= lo) return SQ_OK;
    return phi4_launch_range(c, s, in_buf, st, lo, hi, c->zc, c->zc, (hi - lo + c->zc - 1) / c->zc, 0, timed);
}

void count_step(sq_ctx *c) {
    c->step += 1;
    c->perf.steps += 1;
    for (auto &s : c->slabs) c->perf.site_updates += (long long)s.nz * (long long)plane_floats(c);
}

constexpr int kRunUnsupported = -1000;  // phi4_tb2_range: a resident march does not apply (internal)

// What one phi4_tb2_range launch is asked to do besides its ranges (phi4_block
// fills it per op; the single-slab callers pass the defaults), and what it did.
struct Tb2Opts {
    bool beside_xchg = false;    // the launch runs beside an exchange (it aims at tb_blocks_xchg blocks)
    hipEvent_t stop = nullptr;   // the launch's stop event (SQ_EDGES_STOPEV: EDGES_DONE bound to the dispatch)
    struct {
        bool on;
        int tlo0, thi0, tlen;
    } gate{false, 0, 0, 0};      // gated pair 0: the rim ranges as thin gated chunks of this launch
    float *stage_slot = nullptr; // P2P kstage: the staging slot the pair also writes (nullptr: no staged last pair)
    int run_pairs = 0;           // > 0: one resident launch of this many pairs
    bool stop_used = false;      // out: `stop` was bound to the launch, so EDGES_DONE need not record it
    bool staged = false;         // out: the launch wrote stage_slot and counted its blocks into kstage_ctr
};

// Steps s and s+1 in one launch (sq_phi4.hip, phi4_tb2_kernel) on the planes
// [lo, hi) of slab s and, when lo2 < hi2, also [lo2, hi2) (a range of the same
// length): reads buffer in_buf, writes in_buf ^ 1.
int phi4_tb2_range(sq_ctx *c, const Slab &s, int in_buf, hipStream_t st, int lo, int hi, int lo2, int hi2,
                   int periodic, bool timed, Tb2Opts &o) {
    if (hi <= lo) return SQ_OK;
    const int nr = lo2 < hi2 ? 2 : 1, len = hi - lo;
    if (nr == 2 && hi2 - lo2 != len) return fail(SQ_E_STATE, "two-step launch: ranges of different lengths");
    sq::Phi4StepArgs a = phi4_base_args(c, s, in_buf);
    a.snap = c->snap_next;  // only a one-stream frame's first launch (phi4_frame)
    c->snap_next = nullptr;
    a.stamps = c->stamps_next;  // sq_phi4_block_stamps
    c->stamps_next = nullptr;
    // device frames: a folding first launch (it computes its own coefficients,
    // so it must not read the ones its block 0 writes) arms the clear of the
    // folded record set for the launch after it
    if (c->clr_armed) {
        a.clr = c->clr_next;
        c->clr_armed = false;
    }
    if (c->fold_next.cin != nullptr) {
        a.fold = c->fold_next;
        a.dcoef = nullptr;
        a.tctl = nullptr;  // it derives its buffers itself (frame_fold)
        c->fold_next = sq::FrameFoldArgs{};
        c->clr_armed = true;
    } else if (c->clr_first) {  // a batch's first frame clears the set its second frame uses
        c->clr_armed = true;
    }
    c->clr_first = false;
    // planes per block: pinned, or as many as make one round of tb_blocks
    // blocks (a ragged second round costs more than the deeper chunks), but
    // not fewer than 4 (a chunk recomputes 2 planes of the first step)
    const int nyg = c->Ly / 8, nxseg = c->Lx / 256;
    // (the slabs of a loopback decomposition run concurrently on their own streams)
    const int target = o.beside_xchg ? c->tb_blocks_xchg : c->tb_blocks;
    const int nzc_t = std::max(1, target / (nyg * nxseg * (int)c->slabs.size() * nr));
    const int zb = c->tbz_pin ? c->tbz : std::min(len, std::max(c->tb_minz, (len + nzc_t - 1) / nzc_t));
    a.zlo = lo;
    a.zhi = nr == 2 ? hi2 : hi;
    a.zstep = nr == 2 ? lo2 - lo : 0;
    a.zc = zb;
    a.zlen = len;
    a.nzr = (len + zb - 1) / zb;
    a.nzc = nr * a.nzr;
    a.periodic = periodic;
    a.nxseg = nxseg;
    a.nyg = nyg;
    a.nunits = a.nxseg * a.nyg * a.nzc;
    if (o.gate.on) {  // the rim ranges as thin gated chunks of this launch
        a.gate = c->gate_word;
        a.gate_seq = c->gate_seq;
        a.gate_err = c->gate_err;
        a.n_reg = a.nunits;
        a.tzc = 4;
        a.tlen = o.gate.tlen;
        a.tlo0 = o.gate.tlo0;
        a.thi0 = o.gate.thi0;
        a.ntz = (a.tlen + a.tzc - 1) / a.tzc;
    }
    if (o.run_pairs > 0) {  // one resident launch of run_pairs pairs (the caller left no frame / stamp / stop state)
        const int pairs = o.run_pairs;
        if (c->profiling == 1 || c->run_flags == nullptr || c->gate_err == nullptr || !sq::phi4_tb2_run_ok(a, c->dev))
            return kRunUnsupported;  // nothing consumed: the caller falls back to one launch per pair
        sq::Tb2RunArgs r{c->run_flags, c->gate_err, c->run_base, pairs, nullptr};
        // diagnostics: SQ_DIAG_RUN_STAMPS=<file> appends each launch's per-pair
        // block stamps (Tb2RunArgs::stamps) as {npairs, nblocks, words...} u64
        const char *dpath = getenv("SQ_DIAG_RUN_STAMPS");
        const size_t nst = 2 * (size_t)pairs * a.nunits + a.nunits;
        if (dpath) SQ_HIP(hipMalloc(&r.stamps, nst * sizeof(unsigned long long)));
        uint64_t kid = 0;
        SQ_HIP(sq::phi4_tb2_run_launch(a, r, st, nullptr, nullptr, &kid));
        if (dpath) {
            std::vector<unsigned long long> h(nst + 2);
            h[0] = (unsigned long long)pairs;
            h[1] = (unsigned long long)a.nunits;
            SQ_HIP(hipStreamSynchronize(st));
            SQ_HIP(hipMemcpy(h.data() + 2, r.stamps, nst * sizeof(unsigned long long), hipMemcpyDeviceToHost));
            SQ_HIP(hipFree(r.stamps));
            if (FILE *f = fopen(dpath, "ab")) {
                fwrite(h.data(), sizeof(unsigned long long), h.size(), f);
                fclose(f);
            }
        }
        c->run_base += (unsigned int)pairs;
        c->perf.kernel_launches += 1;
        c->kstat[kid] += 1;
        c->perf.fused_steps += 2 * pairs;
        return SQ_OK;
    }
    EvPair *e = nullptr;
    if (timed && c->profiling == 1) {
        int rc = ev_take(c, &e);
        if (rc) return rc;
        c->ev_extra_steps += 1;
    }
    if (a.stamps != nullptr) {  // every block of the grid stamps (a gated launch adds its rim chunks)
        const int grid_n = a.nunits + (a.gate != nullptr ? a.nxseg * a.nyg * 2 * a.ntz : 0);
        if (grid_n > c->stamps_cap) return fail(SQ_E_STATE, "block stamps: more blocks than stamp slots");
        c->stamps_blocks = grid_n;
    }
    hipEvent_t stop = o.stop;
    uint64_t kid = 0;
    if (o.stage_slot != nullptr && stop == nullptr && sq::phi4_tb2_stage_ok(a, c->gz)) {
        const sq::Tb2StageArgs g{o.stage_slot, c->gz, c->kstage_ctr};
        SQ_HIP(sq::phi4_tb2_stage_launch(a, g, st, e ? e->a : nullptr, e ? e->b : nullptr, &kid));
        c->kstage_n += (unsigned int)a.nunits;
        o.staged = true;
    } else if (e == nullptr && stop != nullptr) {
        SQ_HIP(sq::phi4_tb2_launch(a, st, nullptr, stop, &kid));
        o.stop_used = true;
    } else {
        SQ_HIP(sq::phi4_tb2_launch(a, st, e ? e->a : nullptr, e ? e->b : nullptr, &kid));
    }
    c->perf.kernel_launches += 1;
    c->kstat[kid] += 1;
    c->perf.fused_steps += 2;
    return SQ_OK;
}

// Single slab covering the lattice: steps s and s+1 in one launch; the
// output lands in the other buffer.
int phi4_tb2_pair(sq_ctx *c) {
    Slab &s = c->slabs[0];
    Tb2Opts o;
    int rc = phi4_tb2_range(c, s, c->cur, s.sA, 0, s.nz, 0, 0, 1, true, o);
    if (rc) return rc;
    c->cur ^= 1;
    count_step(c);
    count_step(c);
    return SQ_OK;
}

// Single slab, SQ_TB2_RUN=1: `pairs` pairs as one resident launch
// (sq_phi4_run.hip); the output lands in buffer cur ^ (pairs & 1).
int phi4_tb2_run_pairs(sq_ctx *c, int pairs) {
    Slab &s = c->slabs[0];
    Tb2Opts o;
    o.run_pairs = pairs;
    int rc = phi4_tb2_range(c, s, c->cur, s.sA, 0, s.nz, 0, 0, 1, true, o);
    if (rc) return rc;
    c->cur ^= pairs & 1;
    for (int i = 0; i < 2 * pairs; ++i) count_step(c);
    return SQ_OK;
}

// Single slab covering the lattice: one launch per step, z wraps in-kernel.
int phi4_periodic_step(sq_ctx *c) {
    Slab &s = c->slabs[0];
    const int nzc = (s.nz + c->zc - 1) / c->zc;
    int rc = phi4_launch_range(c, s, c->cur, s.sA, 0, s.nz, c->zc, c->zc, nzc, 1, true);
    if (rc) return rc;
    c->cur ^= 1;
    count_step(c);
    return SQ_OK;
}

// Deep-halo block of g <= gz steps on every slab: executes block_plan.
int phi4_block(sq_ctx *c, int g) {
    const size_t plane = plane_floats(c);
    const int ns = (int)c->slabs.size(), G = c->gz;
    const size_t gbytes = (size_t)G * plane * sizeof(float);
    const int cur = c->cur;
    const unsigned long long step0 = c->step;
    std::vector<std::vector<sq_block_op>> plans;
    for (const Slab &s : c->slabs) plans.push_back(block_plan(s.nz, G, g, c->tbz > 0, c->edge_first, c->core_pairs, c->rims_b));
    // 1. exchange (stream B), for every slab before any slab waits for one;
    //    staged (EXCHANGE op lo = 1): the edge planes are copied aside first and
    //    sent from the copy, so the block's core pairs may overwrite them early
    std::vector<const float *> src_lo(ns), src_hi(ns);
    for (int i = 0; i < ns; ++i) {
        Slab &s = c->slabs[i];
        const float *p0 = plane0(c, s, cur);
        src_lo[i] = p0;
        src_hi[i] = p0 + (size_t)(s.nz - G) * plane;
    }
    // P2P with the staging slot already written by the previous block's last
    // pair (kstage): no EDGES_DONE wait and no staging copy on stream B, the
    // hand-shake waits for that pair's block count instead
    // SQ_XCHG_ON_A: the whole exchange on stream A, in order (no events)
    const bool on_a = c->xchg_on_a && ns == 1 &&
                      ((c->p.comm == SQ_COMM_P2P && c->p2p_kernel_handshake) || c->p.comm == SQ_COMM_RCCL);
    // the staged slot is used on stream A (stream order) or, when pinned
    // (SQ_P2P_KSTAGE=1), on stream B behind a wait for the pair's block count
    const bool kst = c->p.comm == SQ_COMM_P2P && c->kstage_pending && ns == 1 && c->p2p_kernel_handshake &&
                     (on_a || c->kstage_env == 1);
    c->kstage_pending = false;
    for (int i = 0; i < ns; ++i) {
        Slab &s = c->slabs[i];
        if (kst || on_a) continue;
        if (c->evE_stale) {  // the last pair before is complete in stream-A order: record it now
            SQ_HIP(hipEventRecord(s.evE, s.sA));
            c->evE_stale = false;
        }
        if (!c->diag_no_ewait) SQ_HIP(hipStreamWaitEvent(s.sB, s.evE, 0));
        if (c->p.comm == SQ_COMM_LOOPBACK) {  // we write the neighbours' ghosts: wait for them too
            SQ_HIP(hipStreamWaitEvent(s.sB, c->slabs[(i + ns - 1) % ns].evE, 0));
            SQ_HIP(hipStreamWaitEvent(s.sB, c->slabs[(i + 1) % ns].evE, 0));
        }
    }
    const bool p2p = c->p.comm == SQ_COMM_P2P;
    if (p2p && !c->p2p_ready) return fail(SQ_E_STATE, "SQ_COMM_P2P context not connected (sq_p2p_connect)");
    // P2P: this exchange's staged slot (two, by parity).  Reusing slot e & 1 at
    // exchange e needs both neighbours to have pulled our exchange e - 2; each
    // wrote its staged flag of exchange e - 1 behind that pull (stream order on
    // its exchange stream), and our exchange e - 1 waited for both flags before
    // anything of exchange e is issued behind it -- no acknowledgement words
    // and no waits on them per exchange (sq_destroy still drains with them).
    const size_t slot_stride = 2 * (size_t)c->gpad * plane;
    const size_t slot = p2p ? (size_t)((c->xchg_seq + 1) & 1u) * slot_stride : 0;
    for (int i = 0; i < ns; ++i) {
        Slab &s = c->slabs[i];
        const bool staged_wait = plans[i][0].lo == 1;  // core pair 1 waits for the copy (WAIT_STAGED)
        if (kst) continue;                              // the slot is written already
        if (!staged_wait && !p2p) continue;            // P2P: the neighbours always read the staged copy
        if (!s.stage) return fail(SQ_E_STATE, "staged exchange without a staging buffer");
        float *stg = s.stage + slot;
        // both ranges in one two-range copy launch (a 2-D hipMemcpy ran as a
        // rect-copy kernel of 23 us against 2 x 6 for two linear copies,
        // profiles/r06/c6/tr_p2p)
        SQ_HIP(sq::p2p_copy2_launch(stg, src_lo[i], stg + (size_t)G * plane, src_hi[i], (size_t)G * plane,
                                    on_a ? s.sA : s.sB));
        if (staged_wait && !on_a) SQ_HIP(hipEventRecord(s.evS, s.sB));
        src_lo[i] = stg;
        src_hi[i] = stg + (size_t)G * plane;
    }
    if (c->p.comm == SQ_COMM_LOOPBACK) {
        for (int i = 0; i < ns; ++i) {
            Slab &s = c->slabs[i];
            Slab &dn = c->slabs[(i + ns - 1) % ns];
            Slab &up = c->slabs[(i + 1) % ns];
            // my bottom G planes -> lower neighbour's upper ghosts [nz_dn, nz_dn+G)
            SQ_HIP(hipMemcpyAsync(plane0(c, dn, cur) + (size_t)dn.nz * plane, src_lo[i], gbytes,
                                  hipMemcpyDeviceToDevice, s.sB));
            // my top G planes -> upper neighbour's lower ghosts [-G, 0)
            SQ_HIP(hipMemcpyAsync(plane0(c, up, cur) - (size_t)G * plane, src_hi[i], gbytes,
                                  hipMemcpyDeviceToDevice, s.sB));
            SQ_HIP(hipEventRecord(s.evC, s.sB));
            c->perf.halo_bytes += 2.0 * (double)gbytes;
        }
    } else if (p2p) {
        // peer pointers: tell both neighbours our staged copy is complete, pull
        // theirs into our ghosts (lower ghosts <- the lower neighbour's top G
        // planes, upper ghosts <- the upper neighbour's bottom G planes), tell
        // them we are done reading.  Flag writes run after everything before
        // them on the stream; P = 2 (both neighbours one peer) and P = 1 (our
        // own copy) need no special case.
        Slab &s = c->slabs[0];
        float *p0 = plane0(c, s, cur);
        const int P = c->p.nranks, r = c->p.rank;
        const int up = (r + 1) % P, dn = (r + P - 1) % P;
        const unsigned int e = ++c->xchg_seq;
        const size_t n = (size_t)G * plane;
        hipStream_t xs = on_a ? s.sA : s.sB;
        if (c->p2p_kernel_handshake) {
            // one wave: "staged e" to both neighbours, then wait for both of theirs
            // (kstage on stream B: first for the last pair's block count; on
            // stream A that pair is complete in stream order)
            SQ_HIP(sq::p2p_handshake_launch(c->peers[up].mbox + kMbStagedFromDn, c->peers[dn].mbox + kMbStagedFromUp,
                                            c->mbox + kMbStagedFromDn, c->mbox + kMbStagedFromUp, e,
                                            kHandshakePolls, c->gate_err, xs,
                                            (kst && !on_a) ? c->kstage_ctr : nullptr, c->kstage_n));
        } else {  // stream-ordered flag writes and waits (SQ_P2P_STREAMOPS=1)
            SQ_HIP(hipStreamWriteValue32(s.sB, c->peers[up].mbox + kMbStagedFromDn, e, 0));
            SQ_HIP(hipStreamWriteValue32(s.sB, c->peers[dn].mbox + kMbStagedFromUp, e, 0));
            SQ_HIP(wait_seq(s.sB, c->mbox + kMbStagedFromDn, e));
            SQ_HIP(wait_seq(s.sB, c->mbox + kMbStagedFromUp, e));
        }
        // both neighbours' staged copies, pulled by one launch
        SQ_HIP(sq::p2p_copy2_launch(p0 - n, c->peers[dn].stage + slot + n, p0 + (size_t)s.nz * plane,
                                    c->peers[up].stage + slot, n, xs));
        if (!on_a) SQ_HIP(hipEventRecord(s.evC, s.sB));
        c->perf.halo_bytes += 2.0 * (double)gbytes;
    } else {  // RCCL: one slab per process; this send/recv order pairs correctly for P = 2 too
        Slab &s = c->slabs[0];
        float *p0 = plane0(c, s, cur);
        const int P = c->p.nranks, r = c->p.rank;
        const int up = (r + 1) % P, dn = (r + P - 1) % P;
        const size_t n = (size_t)G * plane;
        hipStream_t xs = on_a ? s.sA : s.sB;
        SQ_NCCLW(c, ncclGroupStart());
        SQ_NCCLW(c, ncclSend(src_hi[0], n, ncclFloat32, up, c->comm, xs));
        SQ_NCCLW(c, ncclSend(src_lo[0], n, ncclFloat32, dn, c->comm, xs));
        SQ_NCCLW(c, ncclRecv(p0 - n, n, ncclFloat32, dn, c->comm, xs));
        SQ_NCCLW(c, ncclRecv(p0 + (size_t)s.nz * plane, n, ncclFloat32, up, c->comm, xs));
        SQ_NCCLW(c, ncclGroupEnd());
        if (!on_a) SQ_HIP(hipEventRecord(s.evC, s.sB));
        c->perf.halo_bytes += 2.0 * (double)gbytes;
    }
    // gated pair 0: the exchange's completion as a device word the rim chunks poll
    const bool gated = c->slab_gate && c->gate_word != nullptr && ns == 1 && per_rank(c->p.comm) &&
                       gate_pattern(plans[0]) >= 0;
    if (gated) SQ_HIP(hipStreamWriteValue32(c->slabs[0].sB, c->gate_word, ++c->gate_seq, 0));
    // 2. the rest of the schedule, slab by slab (each slab has its own streams;
    //    slabs of a loopback decomposition may differ in nz, hence in schedule)
    int out_buf = cur;
    bool stop_used = false;  // EDGES_DONE is bound to the pair before it as its stop event
    bool staged = false;     // the pair before EDGES_DONE wrote the next exchange's staging slot
    for (int i = 0; i < ns; ++i) {
        Slab &s = c->slabs[i];
        const std::vector<sq_block_op> &ops = plans[i];
        // launch groups: the ops of one first step read the buffer written by
        // the group before (every group flips the parity once)
        std::vector<int> starts;
        for (const sq_block_op &op : ops)
            if (op.kind == SQ_OP_STEP || op.kind == SQ_OP_PAIR) starts.push_back(op.step);
        std::sort(starts.begin(), starts.end());
        starts.erase(std::unique(starts.begin(), starts.end()), starts.end());
        std::vector<char> timed(starts.size(), 0);
        // stream-A launches issued while an exchange may run: from the block's
        // exchange to its WAIT_EXCHANGE (the core pairs), and after EDGES_DONE
        // (the middle pair, beside the next block's exchange)
        bool xchg_live = true;
        for (size_t oi = 0; oi < ops.size(); ++oi) {
            const sq_block_op &op = ops[oi];
            int rc = SQ_OK;
            hipStream_t st = op.stream == kB ? s.sB : s.sA;
            Tb2Opts o;
            o.beside_xchg = xchg_live && op.stream != kB && c->p.comm != SQ_COMM_NONE;
            // gated pair 0: [PAIR core (A), WAIT_EXCHANGE (A), PAIR rim (A, two ranges)] of the
            // same step as one launch whose rim chunks wait in-kernel for the exchange
            if (gated && (int)oi == gate_pattern(ops)) {
                const sq_block_op &rim = ops[oi + 2];
                const size_t gi = (size_t)(std::lower_bound(starts.begin(), starts.end(), op.step) - starts.begin());
                const int in = cur ^ (int)(gi & 1);
                const bool first = !timed[gi];
                timed[gi] = 1;
                c->step = step0 + (unsigned long long)op.step;
                o.gate = {true, rim.lo, rim.lo2, rim.hi - rim.lo};
                rc = phi4_tb2_range(c, s, in, st, op.lo, op.hi, 0, 0, 0, first, o);
                if (rc) return rc;
                xchg_live = false;
                oi += 2;
                continue;
            }
            if (op.kind == SQ_OP_STEP || op.kind == SQ_OP_PAIR) {
                const size_t gi = (size_t)(std::lower_bound(starts.begin(), starts.end(), op.step) - starts.begin());
                const int in = cur ^ (int)(gi & 1);
                const bool first = !timed[gi];  // it carries the group's timing
                timed[gi] = 1;
                c->step = step0 + (unsigned long long)op.step;
                stop_used = false;
                if (c->edges_stopev && op.kind == SQ_OP_PAIR && oi + 1 < ops.size() &&
                    ops[oi + 1].kind == SQ_OP_EDGES_DONE && ops[oi + 1].stream == op.stream)
                    o.stop = s.evE;  // phi4_tb2_range binds it to the launch (stop_used)
                // P2P kstage: the block's last pair (the whole slab, right before
                // EDGES_DONE) also writes the next exchange's staging slot
                staged = false;
                const bool kstage = p2p && kstage_on(c) && ns == 1 && c->p2p_kernel_handshake && !c->in_frame &&
                                     s.stage != nullptr && op.kind == SQ_OP_PAIR && op.stream == kA && op.lo == 0 &&
                                     op.hi == s.nz && op.lo2 >= op.hi2 && oi + 1 < ops.size() &&
                                     ops[oi + 1].kind == SQ_OP_EDGES_DONE && ops[oi + 1].stream == kA;
                if (kstage) o.stage_slot = s.stage + (size_t)((c->xchg_seq + 1) & 1u) * slot_stride;
                if (op.kind == SQ_OP_PAIR) {
                    rc = phi4_tb2_range(c, s, in, st, op.lo, op.hi, op.lo2, op.hi2, 0, first, o);
                    stop_used = o.stop_used;  // an empty range launched nothing: EDGES_DONE records
                    staged = o.staged;
                } else if (op.lo2 < op.hi2)  // two equal ranges in one launch: two chunks zstep apart
                    rc = phi4_launch_range(c, s, in, st, op.lo, op.hi2, op.lo2 - op.lo, op.hi - op.lo, 2, 0, first);
                else
                    rc = phi4_launch_span(c, s, in, st, op.lo, op.hi, first);
            } else if (op.kind == SQ_OP_WAIT_EXCHANGE) {
                if (op.stream != kB) xchg_live = false;
                // (SQ_DIAG_NO_XWAIT=1, timing diagnostics only: no wait, the rims race the exchange)
                if (op.stream != kB && !c->diag_no_xwait && !on_a) SQ_HIP(hipStreamWaitEvent(st, s.evC, 0));
                if (c->p.comm == SQ_COMM_LOOPBACK) {
                    SQ_HIP(hipStreamWaitEvent(st, c->slabs[(i + ns - 1) % ns].evC, 0));
                    SQ_HIP(hipStreamWaitEvent(st, c->slabs[(i + 1) % ns].evC, 0));
                }
            } else if (op.kind == SQ_OP_WAIT_STAGED) {
                if (!kst) SQ_HIP(hipStreamWaitEvent(st, s.evS, 0));  // kstage: no copy reads the field
            } else if (op.kind == SQ_OP_EDGES_DONE) {
                xchg_live = true;
                if (staged) {  // the next exchange waits for the pair's block count instead
                    c->kstage_pending = true;
                    c->evE_stale = true;
                    staged = false;
                } else if (on_a) {  // the next exchange follows on stream A in order
                    c->evE_stale = true;
                } else if (!stop_used && !c->diag_no_ewait) {
                    SQ_HIP(hipEventRecord(s.evE, st));  // else bound to the pair before
                    c->evE_stale = false;
                }
                stop_used = false;
            } else if (op.kind == SQ_OP_SIGNAL || op.kind == SQ_OP_WAIT) {
                if (op.lo < 0 || op.lo >= kPlanSlots) return fail(SQ_E_STATE, "block op event slot out of range");
                if (op.kind == SQ_OP_SIGNAL)
                    SQ_HIP(hipEventRecord(s.evk[op.lo], st));
                else
                    SQ_HIP(hipStreamWaitEvent(st, s.evk[op.lo], 0));
            } else if (op.kind != SQ_OP_EXCHANGE) {  // the exchange was issued above for every slab
                return fail(SQ_E_STATE, "unknown block op");
            }
            if (rc) return rc;
        }
        out_buf = cur ^ (int)(starts.size() & 1);
    }
    c->step = step0;
    for (int k = 0; k < g; ++k) count_step(c);
    c->cur = out_buf;
    return SQ_OK;
}

// Ghost depth by measurement (slab paths): G in {4, 8, 16} (<= the allocated
// depth), each timed over two blocks after one warm-up block on the interior
// stream; across ranks the per-candidate times are max-reduced (RCCL or peer
// memory) so every rank picks the same G (exchange sizes must match).  With
// fused pairs the deepest zone is also tried without a core/rim split (K = 0)
// and with K = 2, 4 core pairs, rims on A or on the exchange stream.  The
// trial steps are ordinary steps: the field is the same for any schedule
// (DESIGN.md §8).
int phi4_autotune(sq_ctx *c, int &n) {
    struct Cand {
        int g, k;
        bool rb, ef, a;
    };
    std::vector<Cand> cand;
    const bool ef = c->edge_first, a0 = c->xchg_on_a;
    for (int g : {4, 8, 16})
        if (g <= c->gpad) cand.push_back({g, c->core_pairs, c->rims_b, ef, a0});
    if (cand.empty()) cand.push_back({c->gpad, c->core_pairs, c->rims_b, ef, a0});
    const int gd = cand.back().g;
    if (c->tbz > 0 && c->k_auto && !a0) {
        cand.push_back({gd, 0, false, ef, false});
        for (bool rb : {false, true})
            for (int k : {2, 4})
                if (k <= gd / 2) cand.push_back({gd, k, rb, ef, false});
    }
    // the exchange in order on stream A (no overlap, no cross-stream hop):
    // cheaper when the transfer is short, so timed like the rest
    if (c->a_auto && !a0) cand.push_back({gd, 0, false, ef, true});
    // the edges-first split of the block's last pair buys the next exchange a
    // longer window at the price of a split launch and an event bubble: worth
    // it when the exchange is long (a real link), not on one GPU (19.3 vs 19.9
    // us/step at 256^3, profiles/r03/s2/slab_ef/), so both are timed
    if (c->ef_auto) cand.push_back({gd, c->core_pairs, c->rims_b, !ef, a0});
    if (cand.size() > 16) cand.resize(16);  // dtune holds 16 times
    int need = 0;
    for (const Cand &k : cand) need += 3 * k.g;
    if (n < need) return SQ_OK;  // too few steps requested: try again on a later call
    hipEvent_t t0, t1;
    SQ_HIP(hipEventCreate(&t0));
    SQ_HIP(hipEventCreate(&t1));
    std::vector<double> ms(cand.size());
    for (size_t k = 0; k < cand.size(); ++k) {
        const int g = cand[k].g;
        c->gz = g;
        c->core_pairs = cand[k].k;
        c->rims_b = cand[k].rb;
        c->edge_first = cand[k].ef;
        c->xchg_on_a = cand[k].a;
        int rc = phi4_block(c, g);
        if (!rc) rc = phi4_join(c);
        if (rc) return rc;
        SQ_HIP(hipEventRecord(t0, c->slabs[0].sA));
        for (int b = 0; b < 2 && !rc; ++b) rc = phi4_block(c, g);
        if (rc) return rc;
        SQ_HIP(hipEventRecord(t1, c->slabs[0].sA));
        SQ_HIP(hipEventSynchronize(t1));
        rc = phi4_join(c);
        if (rc) return rc;
        float e = 0;
        SQ_HIP(hipEventElapsedTime(&e, t0, t1));
        ms[k] = (double)e / (2.0 * g);
        n -= 3 * g;
    }
    (void)hipEventDestroy(t0);
    (void)hipEventDestroy(t1);
    if (per_rank(c->p.comm) && c->p.nranks > 1) {
        hipStream_t st = c->slabs[0].sA;
        SQ_HIP(hipMemcpyAsync(c->dtune, ms.data(), sizeof(double) * ms.size(), hipMemcpyHostToDevice, st));
        int rc = rank_allreduce(c, c->dtune, ms.size(), sq::P2pRed::kMaxF64, st);
        if (rc) return rc;
        SQ_HIP(hipMemcpyAsync(ms.data(), c->dtune, sizeof(double) * ms.size(), hipMemcpyDeviceToHost, st));
        SQ_HIP(hipStreamSynchronize(st));
    }
    const Cand best = cand[(size_t)sq_phi4_pick_ghost(ms.data(), (int)ms.size())];
    c->gz = best.g;
    c->core_pairs = best.k;
    c->rims_b = best.rb;
    c->edge_first = best.ef;
    c->xchg_on_a = best.a;
    c->g_tuned = true;
    return SQ_OK;
}

int phi4_steps_impl(sq_ctx *c, int n) {
    if (c->p.comm == SQ_COMM_NONE) {
        if (c->tb_run && c->tbz > 0 && n >= 4 && !c->in_frame && c->snap_next == nullptr &&
            c->stamps_next == nullptr && c->fold_next.cin == nullptr && !c->clr_armed && !c->clr_first) {
            int rc = gate_check(c, false);  // no march on a field a timed-out launch left corrupt
            if (rc) return rc;
            // SQ_TB2_RUN_MAXP (experiments): at most this many pairs per launch
            const char *mp = getenv("SQ_TB2_RUN_MAXP");
            const int maxp = mp ? std::max(1, atoi(mp)) : INT_MAX;
            while (n >= 2) {
                const int np = std::min(n / 2, maxp);
                rc = phi4_tb2_run_pairs(c, np);
                if (rc == kRunUnsupported) {
                    c->tb_run = false;  // this context's shape: one launch per pair from now on
                    break;
                }
                if (rc) return rc;
                n -= 2 * np;
            }
        }
        for (; c->tbz > 0 && n >= 2; n -= 2) {
            int rc = phi4_tb2_pair(c);
            if (rc) return rc;
        }
        for (int i = 0; i < n; ++i) {
            int rc = phi4_periodic_step(c);
            if (rc) return rc;
        }
        return SQ_OK;
    }
    if (c->p.comm == SQ_COMM_P2P && !c->p2p_ready)
        return fail(SQ_E_STATE, "SQ_COMM_P2P context not connected (sq_p2p_connect)");
    {
        int rc = fin_agree(c);
        if (rc) return rc;
    }
    if (c->g_auto && !c->g_tuned) {
        int rc = phi4_autotune(c, n);
        if (rc) return rc;
    }
    // balanced blocks: the fewest blocks of <= gz steps, of near-equal length
    // (even where fused pairs can use it), so a call of n steps pays
    // ceil(n / gz) exchanges and the least redundant ghost-zone work: 20 steps
    // at gz = 16 run as 10 + 10, not 16 + 4
    while (n > 0) {
        const int nb = (n + c->gz - 1) / c->gz;
        int g = (n + nb - 1) / nb;
        if (c->tbz > 0 && (g & 1) && g < c->gz) ++g;
        g = std::min(g, n);
        int rc = phi4_block(c, g);
        if (rc) return rc;
        n -= g;
    }
    return SQ_OK;
}

}  // namespace

namespace sq {

// P2P: does the block's last pair write the next exchange's staging slot
// (SQ_P2P_KSTAGE pins it; by default with the exchange on stream A, whose
// stream order replaces the count wait on stream B)
bool kstage_on(const sq_ctx *c) { return c->kstage_env >= 0 ? c->kstage_env != 0 : c->xchg_on_a; }

// Gated rim chunks that gave up waiting for their exchange (tb_gate_wait) store
// nothing, so the field is corrupt from then on: the error is sticky on the
// context.  read_device: the caller has joined the streams, read the device
// word (otherwise only the sticky flag, no synchronisation).
int gate_check(sq_ctx *c, bool read_device) {
    if (!c->gate_failed && read_device && c->gate_err) {
        int e = 0;
        SQ_HIP(hipMemcpy(&e, c->gate_err, sizeof e, hipMemcpyDeviceToHost));
        if (e) c->gate_failed = true;
    }
    if (c->gate_failed)
        return fail(SQ_E_COMM, "slab exchange: gated rim chunks timed out waiting for the exchange, a P2P "
                               "hand-shake gave up waiting for a neighbour, or a resident march's block gave up "
                               "waiting for its neighbours (planes are stale; the field is corrupt until it is "
                               "uploaded or initialised again)");
    return SQ_OK;
}

// a new field replaces every plane: the timed-out chunks no longer matter
// (a resident march's epochs start over too: a timed-out launch left them uneven)
int gate_reset(sq_ctx *c) {
    if (c->gate_err) SQ_HIP(hipMemset(c->gate_err, 0, sizeof(int)));
    if (c->run_flags) SQ_HIP(hipMemset(c->run_flags, 0, (size_t)c->run_nflags * sizeof(unsigned int)));
    c->kstage_pending = false;  // the staged edges are the old field's
    c->run_base = 0;
    c->gate_failed = false;
    return SQ_OK;
}

// Multi-rank: one rank's unguarded upload makes the others' ghost planes
// unguarded too, so after a local change of field_finite the ranks agree on it
// (max-reduce of "not finite") before the next step call or frame uses it.
int fin_agree(sq_ctx *c) {
    if (!c->fin_sync) return SQ_OK;
    c->fin_sync = false;
    if (!per_rank(c->p.comm) || c->p.nranks <= 1) return SQ_OK;
    hipStream_t st = c->slabs[0].sA;
    double v = c->field_finite ? 0.0 : 1.0;
    SQ_HIP(hipMemcpyAsync(c->dtune, &v, sizeof v, hipMemcpyHostToDevice, st));
    int rc = rank_allreduce(c, c->dtune, 1, sq::P2pRed::kMaxF64, st);
    if (rc) return rc;
    SQ_HIP(hipMemcpyAsync(&v, c->dtune, sizeof v, hipMemcpyDeviceToHost, st));
    SQ_HIP(hipStreamSynchronize(st));
    c->field_finite = v == 0.0;
    return SQ_OK;
}

// Every launch of the call reads c->field_finite as its `fin`; once one step
// has run, every plane (ghost zones included: they are exchanged copies) has
// been through the guard.
int phi4_steps(sq_ctx *c, int n) {
    const int rc = phi4_steps_impl(c, n);
    if (rc == SQ_OK && n > 0) c->field_finite = true;
    return rc;
}

int phi4_join(sq_ctx *c) {
    for (auto &s : c->slabs) {
        SQ_HIP(hipStreamSynchronize(s.sA));
        SQ_HIP(hipStreamSynchronize(s.sB));
    }
    return SQ_OK;
}

}  // namespace sq

extern "C" {

int sq_step(sq_ctx *c, int nsteps) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "sq_step is for PHI4 contexts (QM1D uses sq_run_frame)");
    if (nsteps < 0) return fail(SQ_E_ARG, "nsteps < 0");
    DeviceGuard g(c->dev);
    {
        int rc = gate_check(c, false);  // a known timeout: no more steps on the corrupt field
        if (rc) return rc;
    }
    const auto t0 = std::chrono::steady_clock::now();
    EvPair *region = nullptr;
    if (c->profiling == 2 && nsteps > 0) {
        int rc = ev_take(c, &region);
        if (rc) return rc;
        SQ_HIP(hipEventRecord(region->a, c->slabs[0].sA));
    }
    {
        int rc = phi4_steps(c, nsteps);
        if (rc) return rc;
    }
    if (c->gate_err) {  // tests: SQ_DIAG_GATE_ERR=1 flags a gate timeout as tb_gate_wait would
        const char *ge = getenv("SQ_DIAG_GATE_ERR");
        if (ge && atoi(ge) != 0) SQ_HIP(hipMemsetAsync(c->gate_err, 1, 1, c->slabs[0].sA));
    }
    if (region) {
        SQ_HIP(hipEventRecord(region->b, c->slabs[0].sA));
        c->region_steps += nsteps;
    }
    c->perf.frame_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SQ_OK;
}

int sq_phi4_block_stamps(sq_ctx *c, unsigned long long *out, int cap, int *nblocks) {
    if (!c || !out || !nblocks || cap < 1) return fail(SQ_E_ARG, "null argument");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "PHI4 only");
    if (c->slabs.size() != 1 || c->p.comm != SQ_COMM_NONE || c->tbz <= 0)
        return fail(SQ_E_STATE, "block stamps: one slab without an exchange, fused launches");
    DeviceGuard g(c->dev);
    const int need = std::max(cap, 4096);
    if (c->stamps_cap < need) {
        (void)hipFree(c->dstamps);
        c->stamps_cap = 0;
        SQ_HIP(hipMalloc(&c->dstamps, 4 * sizeof(unsigned long long) * (size_t)need));  // + the shader clock
        c->stamps_cap = need;
    }
    c->stamps_next = c->dstamps;
    c->stamps_blocks = 0;
    int rc = phi4_steps(c, 2);
    c->stamps_next = nullptr;
    if (rc) return rc;
    if (c->stamps_blocks > cap) return fail(SQ_E_ARG, "cap smaller than the launch's blocks");
    SQ_HIP(hipMemcpyAsync(out, c->dstamps, 2 * sizeof(unsigned long long) * (size_t)c->stamps_blocks,
                          hipMemcpyDeviceToHost, c->slabs[0].sA));
    SQ_HIP(hipStreamSynchronize(c->slabs[0].sA));
    *nblocks = c->stamps_blocks;
    return SQ_OK;
}

int sq_phi4_block_clocks(sq_ctx *c, unsigned long long *out, int cap, int *nblocks) {
    if (!c || !out || !nblocks || cap < 1) return fail(SQ_E_ARG, "null argument");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "PHI4 only");
    if (c->dstamps == nullptr || c->stamps_blocks < 1) return fail(SQ_E_STATE, "no sq_phi4_block_stamps launch yet");
    if (c->stamps_blocks > cap) return fail(SQ_E_ARG, "cap smaller than the launch's blocks");
    DeviceGuard g(c->dev);
    const size_t n = 2 * (size_t)c->stamps_blocks;  // written behind the 2 x blocks constant-clock stamps
    SQ_HIP(hipMemcpyAsync(out, c->dstamps + n, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost,
                          c->slabs[0].sA));
    SQ_HIP(hipStreamSynchronize(c->slabs[0].sA));
    *nblocks = c->stamps_blocks;
    return SQ_OK;
}

}  // extern "C"
