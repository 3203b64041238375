// sq_phi4_create.cpp -- PHI4 context set-up: lattice geometry, the slab
// decomposition with its buffers, streams and events, the launch shapes and
// every SQ_* tuning override read at creation; the getters that report them.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "sq_ctx.h"

using namespace sq;

namespace sq {

int create_phi4(sq_ctx *c) {
    const sq_params &p = c->p;
    if (p.dims[0] <= 0 || p.dims[1] <= 0 || p.dims[2] <= 0 || p.dims[0] > (1 << 20) ||
        p.dims[1] > (1 << 20))
        return fail(SQ_E_ARG, "PHI4 dims must be positive");
    c->Lx = (int)p.dims[0];
    c->Ly = (int)p.dims[1];
    c->Lz = p.dims[2];
    if (!sq::phi4_geometry(c->Lx, c->Ly, &c->geom))
        return fail(SQ_E_ARG, "PHI4 needs Lx in {8,16,32,64,128,256} or a multiple of 256, and Ly a "
                              "multiple of the wave's row count");
    // Philox counter word 0 holds the global site quad (sites/4): < 2^32 quads,
    // i.e. up to 1.7e10 sites (68 GB of fp32 field, a quarter of one MI355X).
    if ((long long)c->Lx * c->Ly * c->Lz / 4 >= (1ll << 32))
        return fail(SQ_E_ARG, "lattice exceeds 2^34 sites (Philox counter layout)");
    if ((long long)c->Lx * c->Ly * 4 >= (1ll << 31))
        return fail(SQ_E_ARG, "plane exceeds 2 GiB (32-bit buffer offsets)");
    if (c->Lz >= (1ll << 31)) return fail(SQ_E_ARG, "Lz must be < 2^31 (32-bit plane indices)");
    {   // the guard's fast path (Phi4StepArgs::fin) needs every update of a field
        // inside [-clamp, clamp] to be finite or +-inf, never NaN: bound the drift
        const double cl = p.clamp, h = p.deltatau;
        const double drift = 12.0 * cl + std::fabs(p.m2) * cl + std::fabs(p.lambda) / 6.0 * cl * cl * cl;
        // (float)clamp squared finite too: with lambda = 0, clamp^2 = inf would make
        // fma(lam/6, phi^2, m2) = 0 * inf = NaN at |phi| = clamp
        const float clf = (float)cl;
        if (!std::isfinite(cl) || !(cl > 0) || !std::isfinite(p.m2) || !std::isfinite(p.lambda) ||
            !std::isfinite(p.C) || !std::isfinite(clf * clf) ||
            !(h * drift + cl + 16.0 * sqrt(2.0 * h) * std::fabs(p.C) < 1e30))
            return fail(SQ_E_ARG, "PHI4 parameters must be finite with clamp^2 finite in fp32 and "
                                  "dtau * drift(clamp) < 1e30");
    }
    if (const char *e = getenv("SQ_ROWS")) {  // tuning override of the rows per lane
        const int r = atoi(e), rs = 64 / c->geom.qx;
        if ((r == 1 || r == 2 || r == 4) && c->Ly % r == 0)
            c->geom = sq::Phi4Geom{c->geom.qx, r, rs * r, c->geom.pf, c->geom.v};
    }
    if (const char *e = getenv("SQ_VSEG"))  // tuning override: float4 segments per lane
        if (atoi(e) == 1 || (atoi(e) == 2 && c->geom.qx == 64 && c->Lx % 512 == 0)) c->geom.v = atoi(e);
    {   // very large per-device fields: non-temporal output stores (mode 4) beat the
        // sc0 sc1 stores of mode 7 at 1024^3 (1575 vs 1598 us per step), not at
        // 512^3 (193.5 vs 190.8 us), profiles/r01/sweep*_sc1.log
        const long long nz_dev = per_rank(p.comm) ? (c->Lz + p.nranks - 1) / std::max(1, p.nranks) : c->Lz;
        const double field_bytes = 4.0 * c->Lx * c->Ly * (double)nz_dev;  // this device's share
        if (c->geom.pf == 7 && 2.0 * field_bytes > 2.0 * (1 << 30)) c->geom.pf = 4;
    }
    if (const char *e = getenv("SQ_PREFETCH")) {  // tuning override of the store / arithmetic mode
        const int m = atoi(e);
        c->geom.pf = (m == 3 || m == 4 || m == 7) && c->geom.qx == 64 ? m : 1;
    }
    int nslab = 1;
    long long zfirst = 0;
    std::vector<long long> zs;
    if (p.comm == SQ_COMM_NONE) {
        zs = {0, c->Lz};
    } else if (p.comm == SQ_COMM_LOOPBACK) {
        nslab = p.nslabs;
        if (nslab < 1 || nslab > c->Lz) return fail(SQ_E_ARG, "nslabs must be in [1, Lz]");
        for (int i = 0; i <= nslab; ++i) zs.push_back(c->Lz * i / nslab);
    } else if (per_rank(p.comm)) {
        if (p.nranks < 1 || p.rank < 0 || p.rank >= p.nranks || p.nranks > c->Lz)
            return fail(SQ_E_ARG, "bad rank/nranks for the slab decomposition");
        if (p.comm == SQ_COMM_P2P && p.nranks > kP2pMaxRanks) return fail(SQ_E_ARG, "SQ_COMM_P2P: too many ranks");
        zfirst = c->Lz * p.rank / p.nranks;
        zs = {zfirst, c->Lz * (p.rank + 1) / p.nranks};
    } else {
        return fail(SQ_E_ARG, "unknown comm");
    }
    // ghost-zone depth: one exchange of gz planes per gz steps;
    // bounded by the thinnest slab so a ghost zone never spans two neighbours
    if (p.comm != SQ_COMM_NONE) {
        long long nz_min = c->Lz;
        for (int i = 0; i < nslab; ++i) nz_min = std::min(nz_min, zs[i + 1] - zs[i]);
        if (per_rank(p.comm)) nz_min = c->Lz / p.nranks;  // identical on every rank
        // measured (profiles/r01/ghost_sweep.log, 256^3 slab, RCCL): 51.8 / 37.0 /
        // 30.4 / 26.9 / 25.6 us per step at G = 1 / 2 / 4 / 8 / 16: a fixed
        // ~28 us per exchange amortised over G steps against (G-1)/nz of
        // redundant ghost-zone planes.  G = nz/16 keeps the redundancy <= ~6 %.
        int g = (int)std::min(16ll, std::max(1ll, nz_min / 16));
        // multi-rank RCCL runs measure G in {4, 8, 16} on the real link (the
        // fixed cost and bandwidth of an xGMI exchange are not those of the
        // one-GPU self-exchange these defaults were measured on); SQ_GHOST
        // pins G, SQ_GHOST_AUTO=1 forces the trials on any slab path
        c->g_auto = per_rank(p.comm) && p.nranks > 1 && nz_min >= 64;
        if (const char *e = getenv("SQ_GHOST_AUTO")) c->g_auto = atoi(e) != 0;
        if (c->g_auto) g = (int)std::min(16ll, nz_min / 2);
        if (const char *e = getenv("SQ_GHOST")) {
            g = std::max(1, atoi(e));
            c->g_auto = false;
        }
        c->gz = (int)std::max(1ll, std::min((long long)g, nz_min));
        c->gpad = c->gz;
        SQ_HIP(hipMalloc(&c->dtune, 16 * sizeof(double)));
    }
    const size_t plane = plane_floats(c);
    for (int i = 0; i < nslab; ++i) {
        c->slabs.emplace_back();  // owned by the context from here on: sq_destroy frees a partial set-up
        Slab &s = c->slabs.back();
        s.z0 = zs[i];
        s.nz = (int)(zs[i + 1] - zs[i]);
        if (s.nz < 1) return fail(SQ_E_ARG, "empty slab");
        const size_t bytes = (size_t)(s.nz + 2 * c->gpad) * plane * sizeof(float);
        for (int k = 0; k < 2; ++k) {
            SQ_HIP(hipMalloc(&s.buf[k], bytes));
            SQ_HIP(hipMemset(s.buf[k], 0, bytes));
        }
        SQ_HIP(hipStreamCreateWithFlags(&s.sA, hipStreamNonBlocking));
        // halo stream at the highest priority: its RCCL and boundary-plane
        // kernels must not queue behind the interior kernel's waves
        // (SQ_XCHG_PRIO=0: the default priority, an experiment)
        int prio_lo = 0, prio_hi = 0;
        SQ_HIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        const char *xp = getenv("SQ_XCHG_PRIO");
        SQ_HIP(hipStreamCreateWithPriority(&s.sB, hipStreamNonBlocking, (xp && atoi(xp) == 0) ? prio_lo : prio_hi));
        SQ_HIP(hipEventCreateWithFlags(&s.evC, hipEventDisableTiming));
        SQ_HIP(hipEventCreateWithFlags(&s.evE, hipEventDisableTiming));
        SQ_HIP(hipEventCreateWithFlags(&s.evS, hipEventDisableTiming));
        s.evk.assign(kPlanSlots, nullptr);
        for (hipEvent_t &e : s.evk) SQ_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        // the staged copy of the 2 G edge planes; P2P keeps two, by exchange parity
        // (phi4_block: a neighbour's staged flag of exchange e-1 then implies it
        // has read our copy of exchange e-2, so no per-exchange acknowledgement)
        if (p.comm != SQ_COMM_NONE)
            SQ_HIP(hipMalloc(&s.stage, stage_slots(p.comm) * 2 * (size_t)c->gpad * plane * sizeof(float)));
        SQ_HIP(hipEventRecord(s.evC, s.sB));
        SQ_HIP(hipEventRecord(s.evE, s.sA));
    }
    {
        int rc = alloc_frame_records(c);
        if (rc) return rc;
    }
    SQ_HIP(hipMalloc(&c->dacc, 2 * sizeof(double)));
    SQ_HIP(hipMalloc(&c->dpart, 4 * sizeof(double) * sq::kMomBlocks));
    SQ_HIP(hipMalloc(&c->dmax, 2 * sizeof(unsigned int)));
    if (p.comm == SQ_COMM_RCCL) {
        int rc = rccl_init(c);
        if (rc) return rc;
    }
    if (per_rank(p.comm)) {  // the gated pair 0's word (fine-grained: written by stream B, polled by kernels)
        SQ_HIP(hipExtMallocWithFlags(reinterpret_cast<void **>(&c->gate_word), 64, hipDeviceMallocFinegrained));
        SQ_HIP(hipMemset(c->gate_word, 0, 64));
        SQ_HIP(hipMalloc(&c->gate_err, sizeof(int)));
        SQ_HIP(hipMemset(c->gate_err, 0, sizeof(int)));
        const char *e = getenv("SQ_SLAB_GATE");
        c->slab_gate = e ? atoi(e) != 0 : false;  // off: its spinning rim blocks hold the CU slots the exchange needs
    }
    if (p.comm == SQ_COMM_P2P) {
        // the last pair's block count (phi4_tb2_stage_kernel; monotonic, never reset)
        SQ_HIP(hipMalloc(&c->kstage_ctr, 64));
        SQ_HIP(hipMemset(c->kstage_ctr, 0, 64));
        const char *ks = getenv("SQ_P2P_KSTAGE");
        if (ks) c->kstage_env = atoi(ks) != 0 ? 1 : 0;
    }
    if (p.comm == SQ_COMM_P2P || p.comm == SQ_COMM_RCCL) {
        // one rank's self-exchange moves no bytes over a link: in order on the
        // interior stream it costs less than the two cross-stream hops that
        // overlap it (RCCL 1.117 vs 1.148, P2P with the staged last pair 1.078
        // vs 1.142 x the single slab, profiles/r06/c25); ranks on a link get
        // it as one more candidate of the timed pick (phi4_autotune)
        if (const char *xa = getenv("SQ_XCHG_ON_A")) {
            c->xchg_on_a = atoi(xa) != 0;
            c->a_auto = false;
        }
    }
    if (p.comm == SQ_COMM_P2P) {
        int rc = p2p_alloc(c);
        if (rc) return rc;
    }
    // z chunk per wave: long enough to amortise the chunk-edge planes, short
    // enough to give >= ~8 waves per CU.
    const long long rows = (long long)(c->Lx / (4 * c->geom.qx * c->geom.v)) * (c->Ly / c->geom.wy);
    const int nz_max = c->slabs[0].nz;
    // measured optima (profiles/r01/sweep*): zc = 4 for one-segment rows (256^3),
    // zc = 8 when rows span several 256-site segments (512^3); big lattices
    // lengthen the chunk while >= 32 waves per SIMD remain, which cuts the
    // chunk-edge plane re-reads (1024^3: zc 32, 1760 -> 1711 us,
    // profiles/r01/sweep1024_zc.log)
    int zc = c->Lx > 256 ? 8 : 4;
    while (zc > 1 && rows * ((nz_max + zc - 1) / zc) < 2048) zc /= 2;
    while (zc < 32 && rows * ((nz_max + 2 * zc - 1) / (2 * zc)) >= 32768) zc *= 2;
    if (const char *e = getenv("SQ_ZCHUNK")) zc = std::max(1, atoi(e));
    // edges-first by default except for one rank's self-exchange, which is short
    // enough to fit beside the next core pair: RCCL (off 19.2-19.4 vs 19.9
    // us/step, round 3) and, since round 6's shorter P2P chain, P2P (off 1.180
    // vs 1.201 x the single slab, profiles/r06/c7/slab_ab.log); the timed pick
    // of multi-rank contexts tries both
    c->edge_first = !((c->p.comm == SQ_COMM_RCCL || c->p.comm == SQ_COMM_P2P) && c->p.nranks == 1);
    if (const char *e = getenv("SQ_EDGE_FIRST")) {
        c->edge_first = atoi(e) != 0;
        c->ef_auto = false;
    }
    if (const char *e = getenv("SQ_CORE_PAIRS")) {
        c->core_pairs = std::max(0, atoi(e));
        c->k_auto = false;
    }
    if (const char *e = getenv("SQ_RIMS_B")) {
        c->rims_b = atoi(e) != 0;
        c->k_auto = false;
    }
    // one rank's self-exchange: in order on stream A unless pinned otherwise
    // (SQ_XCHG_ON_A, or a pinned core / rim split)
    if ((p.comm == SQ_COMM_P2P || p.comm == SQ_COMM_RCCL) && p.nranks == 1 && c->a_auto && c->k_auto)
        c->xchg_on_a = true;
    if (c->xchg_on_a) {  // the exchange runs between two pairs on stream A: nothing to split around it
        c->core_pairs = 0;
        c->rims_b = false;
        c->k_auto = false;
    }
    c->zc = zc;
    // Two steps per launch on 256-wide lattices (SQ_FUSE2=0: off; SQ_FUSE2_Z:
    // pin the output planes per block), single slab and deep-halo slabs alike.
    // 256^3: 19.5 vs 22.0 us per step on the same box; one round of two
    // blocks per CU (z = 16 at 256^3) measured best of z = 8/11/12/16/22/32
    // (profiles/r01/fuse2_sweep.log), so every launch picks the depth that
    // makes one such round.
    // Loopback decompositions (several slabs on one GPU, a rehearsal mode)
    // keep one step per launch unless SQ_FUSE2=1: there the concurrent slab
    // launches ran slower fused (29.1 vs 25.4 us per step, 2 slabs of 128
    // planes), while one RCCL slab of 256 planes gains (24.2 vs 26.0,
    // profiles/r01/fuse2_slabs.log).
    // Rows of several 256-site segments fuse through the x-halo wave: measured
    // (profiles/r02/sweep_tb2_*.log, us per step, fused vs one step per launch)
    // 512^3 153 vs 200 (with the guard's fast path; 197 before it), 1024 x
    // 1024 x 128 194 vs 225, 1024^3 1537 vs 1678.
    const char *fe = getenv("SQ_FUSE2");
    const bool fuse = fe ? atoi(fe) != 0 : p.comm != SQ_COMM_LOOPBACK;
    if (fuse && sq::phi4_tb2_supported(c->Lx, c->Ly) && (p.comm != SQ_COMM_NONE || c->slabs[0].nz >= 2)) {
        c->tbz = 16;
        if (const char *z = getenv("SQ_TB2_MINZ")) c->tb_minz = std::max(1, atoi(z));
        if (const char *z = getenv("SQ_FUSE2_Z")) {
            c->tbz = std::max(1, atoi(z));
            c->tbz_pin = true;
        }
        int ncu = 0;
        SQ_HIP(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->dev));
        // two blocks per CU (256-wide rows: 65 VGPRs, 10 waves; wider rows: 11 waves at <= 80)
        c->tb_blocks = 2 * std::max(1, ncu);
        if (const char *e = getenv("SQ_TB2_BLOCKS_PER_CU")) c->tb_blocks = std::max(1, atoi(e)) * std::max(1, ncu);
        // 96 slots left to the exchange's kernels: RCCL self-exchange, 256^3, G = 16
        // (profiles/r04/slab/): 512 blocks 19.36 / 19.54 us/step, 480 19.49 / 19.47,
        // 448 19.02 / 19.32, 416 18.89 / 19.24; SQ_XCHG_BLOCKS pins the target
        c->tb_blocks_xchg = std::max(1, c->tb_blocks - 96);
        if (const char *e = getenv("SQ_XCHG_BLOCKS")) c->tb_blocks_xchg = std::max(1, atoi(e));
        if (const char *e = getenv("SQ_EDGES_STOPEV")) c->edges_stopev = atoi(e) != 0;
        if (const char *e = getenv("SQ_DIAG_NO_XWAIT")) c->diag_no_xwait = atoi(e) != 0;
        if (const char *e = getenv("SQ_DIAG_NO_EWAIT")) c->diag_no_ewait = atoi(e) != 0;
        if (const char *e = getenv("SQ_P2P_STREAMOPS")) c->p2p_kernel_handshake = atoi(e) == 0;
        const char *rn = getenv("SQ_TB2_RUN");
        if (rn && atoi(rn) != 0 && p.comm == SQ_COMM_NONE && c->slabs.size() == 1) {
            // one epoch word per block: at most Ly / 8 y-bands x nz / 2 chunks (>= 2 planes each)
            c->run_nflags = (c->Ly / 8) * std::max(1, c->slabs[0].nz / 2);
            SQ_HIP(hipMalloc(&c->run_flags, (size_t)c->run_nflags * sizeof(unsigned int)));
            SQ_HIP(hipMemset(c->run_flags, 0, (size_t)c->run_nflags * sizeof(unsigned int)));
            if (c->gate_err == nullptr) {
                SQ_HIP(hipMalloc(&c->gate_err, sizeof(int)));
                SQ_HIP(hipMemset(c->gate_err, 0, sizeof(int)));
            }
            c->tb_run = true;
        }
    }
    SQ_HIP(hipDeviceSynchronize());  // the set-up memsets ran on the null stream
    return SQ_OK;
}

// the gate word, the error word, the resident march's epochs and the staged pair's count
void release_gate(sq_ctx *c) {
    (void)hipFree(c->gate_word);
    (void)hipFree(c->gate_err);
    (void)hipFree(c->run_flags);
    (void)hipFree(c->kstage_ctr);
    c->gate_word = nullptr;
    c->gate_err = nullptr;
    c->run_flags = nullptr;
    c->kstage_ctr = nullptr;
}

void release_slabs(sq_ctx *c) {
    for (auto &s : c->slabs) {
        (void)hipFree(s.buf[0]);
        (void)hipFree(s.buf[1]);
        (void)hipFree(s.snap_pad);
        if (s.sA) (void)hipStreamDestroy(s.sA);
        if (s.sB) (void)hipStreamDestroy(s.sB);
        if (s.evC) (void)hipEventDestroy(s.evC);
        if (s.evE) (void)hipEventDestroy(s.evE);
        if (s.evS) (void)hipEventDestroy(s.evS);
        for (hipEvent_t e : s.evk)
            if (e) (void)hipEventDestroy(e);
        (void)hipFree(s.stage);
    }
    c->slabs.clear();
}

// the observables' and the timed pick's scratch (dslice: sq_correlator; dstamps: sq_phi4_block_stamps)
void release_lattice(sq_ctx *c) {
    (void)hipFree(c->dstamps);
    (void)hipFree(c->dacc);
    (void)hipFree(c->dpart);
    (void)hipFree(c->dslice);
    (void)hipFree(c->dtune);
    (void)hipFree(c->dmax);
    c->dstamps = nullptr;
    c->dacc = c->dpart = c->dslice = c->dtune = nullptr;
    c->dmax = nullptr;
    c->stamps_cap = 0;
}

}  // namespace sq

extern "C" {

int sq_slab(sq_ctx *c, long long *nz_local, long long *z0) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "PHI4 only");
    long long n = 0;
    for (auto &s : c->slabs) n += s.nz;
    if (nz_local) *nz_local = n;
    if (z0) *z0 = c->slabs[0].z0;
    return SQ_OK;
}

int sq_phi4_tile(sq_ctx *c, int out[4]) {
    if (!c || !out) return fail(SQ_E_ARG, "null argument");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "PHI4 only");
    out[0] = c->geom.qx;
    out[1] = c->geom.r;
    out[2] = c->zc;
    out[3] = c->geom.v;
    return SQ_OK;
}

int sq_phi4_kernel(sq_ctx *c, char *name, size_t cap) {
    if (!c || !name || cap == 0) return fail(SQ_E_ARG, "bad argument");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "PHI4 only");
    // the template arguments phi4_step_launch picks for the interior launch
    // (rocprofv3 prints the kernel under exactly this name)
    const bool ms = c->Lx / (4 * c->geom.qx * c->geom.v) > 1;
    const bool nz = (float)(sqrt(2.0 * (double)(float)c->dtau) * c->p.C) != 0.0f;
    const int pf = c->geom.pf;
    if (c->tbz > 0 && c->tbz_pin)
        snprintf(name, cap, "phi4_tb2_kernel<%s> (2 steps per launch) z=%d", nz ? "true" : "false", c->tbz);
    else if (c->tbz > 0)
        snprintf(name, cap, "phi4_tb2_kernel<%s> (2 steps per launch) one round of %d blocks", nz ? "true" : "false",
                 c->tb_blocks);
    else
        snprintf(name, cap, "phi4_step_kernel<%d, %d, %d, %s, %s, %d> zc=%d", c->geom.qx, c->geom.r, c->geom.v,
                 ms ? "true" : "false", nz ? "true" : "false", pf, c->zc);
    return SQ_OK;
}

int sq_phi4_ghost(sq_ctx *c, int *active, int *allocated) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "PHI4 only");
    if (active) *active = c->p.comm == SQ_COMM_NONE ? 0 : c->gz;
    if (allocated) *allocated = c->p.comm == SQ_COMM_NONE ? 0 : c->gpad;
    return SQ_OK;
}

int sq_phi4_schedule(sq_ctx *c, int *core_pairs, int *rims_b, int *tuned) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "PHI4 only");
    const bool slab = c->p.comm != SQ_COMM_NONE;
    if (core_pairs) *core_pairs = slab ? c->core_pairs : 0;
    if (rims_b) *rims_b = slab && c->rims_b ? 1 : 0;
    if (tuned) *tuned = c->g_tuned ? 1 : 0;
    return SQ_OK;
}

int sq_phi4_edge_first(sq_ctx *c, int *edge_first) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "PHI4 only");
    if (edge_first) *edge_first = c->p.comm != SQ_COMM_NONE && c->edge_first ? 1 : 0;
    return SQ_OK;
}

int sq_phi4_exchange_stream(sq_ctx *c, int *in_order, int *kstaged) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "PHI4 only");
    const bool slab = c->p.comm == SQ_COMM_P2P || c->p.comm == SQ_COMM_RCCL;
    if (in_order) *in_order = slab && c->xchg_on_a ? 1 : 0;
    if (kstaged) *kstaged = c->p.comm == SQ_COMM_P2P && kstage_on(c) ? 1 : 0;
    return SQ_OK;
}

int sq_phi4_launch_info(sq_ctx *c, char *name, size_t cap, long long *grid_threads, long long *launches) {
    if (!c || !name || cap == 0) return fail(SQ_E_ARG, "bad argument");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "PHI4 only");
    name[0] = 0;
    uint64_t best = 0;
    long long n = 0;
    for (const auto &kv : c->kstat)  // most launches; ties: the larger grid (the map is ordered by id)
        if (kv.second > n || (kv.second == n && sq::phi4_kernel_id_grid(kv.first) > sq::phi4_kernel_id_grid(best))) {
            best = kv.first;
            n = kv.second;
        }
    if (n > 0) {
        if ((best & 3) == 3)
            sq::phi4_run_kernel_id_name(best, name, cap);
        else
            sq::phi4_kernel_id_name(best, name, cap);
    }
    if (grid_threads) *grid_threads = n > 0 ? (long long)sq::phi4_kernel_id_grid(best) : 0;
    if (launches) *launches = n;
    return SQ_OK;
}

}  // extern "C"
