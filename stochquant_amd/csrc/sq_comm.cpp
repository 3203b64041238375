// sq_comm.cpp -- the two transports of per-rank slab contexts: RCCL
// (bounded bring-up and calls, nccl_settle) and peer pointers over IPC
// (SQ_COMM_P2P, DESIGN.md §8: mailbox, collective slots, hand-shake,
// teardown drain); the all-reduce the frames and observables use on either.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <thread>

#include "sq_ctx.h"

using namespace sq;

namespace {

struct P2pBlob {  // sq_p2p_handle's output
    unsigned int magic, version;
    int rank, nranks, Lx, Ly, gpad, loops, gz, gauto;  // gz / gauto: active ghost depth, timed pick
    // the block schedule: pinned settings and which of them the timed pick may
    // change (the pick's candidate list and every exchange depend on them)
    int ef_auto, k_auto, edge_first, core_pairs, rims_b;
    int a_auto, on_a, kstage;  // the exchange's stream and the staged last pair (SQ_XCHG_ON_A, SQ_P2P_KSTAGE)
    long long Lz, coll_cap;
    unsigned long long seed;
    hipIpcMemHandle_t stage, mbox, coll;
};
static_assert(sizeof(P2pBlob) <= SQ_P2P_HANDLE_BYTES, "P2P handle blob");

// RCCL communicators are created non-blocking (ncclConfig_t.blocking = 0) so
// that no call can hang the host: a call that returns ncclInProgress (the
// init, a group end launching in the background) is polled with
// ncclCommGetAsyncError up to a deadline (SQ_COMM_TIMEOUT_S, default 300 s);
// past it the communicator is aborted (ncclCommAbort) and the call fails
// with SQ_E_COMM instead of waiting forever on a peer that never comes.
double comm_timeout_s() {
    const char *e = getenv("SQ_COMM_TIMEOUT_S");
    const double v = e ? atof(e) : 300.0;
    return v > 0 ? v : 300.0;
}

// Collective over peer memory: our contribution into slot `rank` of every
// rank's gather buffer (parity seq & 1), a flag to each, wait for every rank's
// flag, then fold our buffer's slots in rank order (sq_p2p.hip).  Round k + 2
// reuses round k's slots: a rank issues it only after every rank's flag of
// round k + 1, which each rank writes after its fold of round k.
int p2p_allreduce(sq_ctx *c, void *d, size_t n, sq::P2pRed red, hipStream_t st) {
    const int P = c->p.nranks, r = c->p.rank;
    if (!c->p2p_ready) return fail(SQ_E_STATE, "SQ_COMM_P2P context not connected (sq_p2p_connect)");
    const size_t esz = (red == sq::P2pRed::kMaxU32 || red == sq::P2pRed::kMaxI32) ? 4 : 8;
    if (n * esz > c->coll_cap) return fail(SQ_E_ARG, "collective larger than the P2P slot");
    const unsigned int seq = ++c->coll_seq;
    const size_t base = (size_t)(seq & 1u) * (size_t)P * c->coll_cap;
    for (int q = 0; q < P; ++q)
        SQ_HIP(hipMemcpyAsync(c->peers[q].coll + base + (size_t)r * c->coll_cap, d, n * esz, hipMemcpyDeviceToDevice, st));
    for (int q = 0; q < P; ++q) SQ_HIP(hipStreamWriteValue32(st, c->peers[q].mbox + kMbColl + r, seq, 0));
    for (int q = 0; q < P; ++q) SQ_HIP(wait_seq(st, c->mbox + kMbColl + q, seq));
    SQ_HIP(sq::p2p_fold_launch(c->coll + base, P, c->coll_cap, d, n, red, st));
    return SQ_OK;
}

}  // namespace

namespace sq {

// All-reduce of n elements at d across the ranks of a one-slab-per-process
// context (no-op for one rank and for single-process contexts).
int rank_allreduce(sq_ctx *c, void *d, size_t n, sq::P2pRed red, hipStream_t st) {
    if (c->p.nranks <= 1 || !per_rank(c->p.comm)) return SQ_OK;
    if (c->p.comm == SQ_COMM_P2P) return p2p_allreduce(c, d, n, red, st);
    if (!c->comm) return fail(SQ_E_STATE, "no RCCL communicator");
    ncclDataType_t t = ncclFloat64;
    ncclRedOp_t op = ncclMax;
    switch (red) {
    case sq::P2pRed::kMaxU32: t = ncclUint32; break;
    case sq::P2pRed::kMaxI32: t = ncclInt32; break;
    case sq::P2pRed::kMaxU64: t = ncclUint64; break;
    case sq::P2pRed::kMaxF64: t = ncclFloat64; break;
    case sq::P2pRed::kSumF64: t = ncclFloat64; op = ncclSum; break;
    }
    SQ_NCCLW(c, ncclAllReduce(d, d, n, t, op, c->comm, st));
    return SQ_OK;
}

int nccl_settle(sq_ctx *c, ncclResult_t r, const char *what) {
    if (r == ncclInProgress && c->comm != nullptr) {
        const auto t0 = std::chrono::steady_clock::now();
        const double lim = comm_timeout_s();
        long spins = 0;
        for (;;) {
            ncclResult_t st = ncclSuccess;
            const ncclResult_t q = ncclCommGetAsyncError(c->comm, &st);
            if (q != ncclSuccess) {
                r = q;
                break;
            }
            if (st != ncclInProgress) {
                r = st;
                break;
            }
            const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
            if (el > lim) {
                (void)ncclCommAbort(c->comm);
                c->comm = nullptr;
                return fail(SQ_E_COMM, std::string(what) + ": no completion within " + std::to_string((int)lim) +
                                           " s (SQ_COMM_TIMEOUT_S); communicator aborted");
            }
            if (++spins > 2000) std::this_thread::sleep_for(std::chrono::microseconds(50));
            else std::this_thread::yield();
        }
    }
    if (r != ncclSuccess) return fail(SQ_E_COMM, std::string(what) + ": " + ncclGetErrorString(r));
    return SQ_OK;
}

// create_phi4, SQ_COMM_RCCL: the halo communicator.
int rccl_init(sq_ctx *c) {
    const sq_params &p = c->p;
    ncclUniqueId id;
    static_assert(sizeof(id.internal) <= 128, "ncclUniqueId size");
    memcpy(id.internal, p.comm_id, sizeof(id.internal));
    // non-blocking (bounded bring-up, nccl_settle) with the halo kernels'
    // CU footprint capped: the exchange's send/recv kernel shares the CUs
    // with the core pair it overlaps, so it gets
    // SQ_RCCL_MAX_CTAS blocks (default kRcclMaxCtas; 0 = RCCL's choice)
    ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
    const char *nb = getenv("SQ_RCCL_BLOCKING");
    cfg.blocking = (nb && atoi(nb) != 0) ? 1 : 0;
    const char *mc = getenv("SQ_RCCL_MAX_CTAS");
    const int max_ctas = mc ? atoi(mc) : kRcclMaxCtas;
    if (max_ctas > 0) {
        cfg.maxCTAs = max_ctas;
        cfg.minCTAs = 1;
    }
    ncclResult_t r = ncclCommInitRankConfig(&c->comm, p.nranks, id, p.rank, &cfg);
    if (r != ncclSuccess && r != ncclInProgress) {
        c->comm = nullptr;
        return fail(SQ_E_COMM, std::string("ncclCommInitRankConfig: ") + ncclGetErrorString(r));
    }
    return nccl_settle(c, r, "ncclCommInitRankConfig");
}

// create_phi4, SQ_COMM_P2P: mailbox and collective slots; peers mapped by sq_p2p_connect.
int p2p_alloc(sq_ctx *c) {
    const sq_params &p = c->p;
    // fine-grained device memory: the words are written by the peers'
    // command processors (hipStreamWriteValue32) and copy engines from
    // other devices over xGMI and polled here by hipStreamWaitValue32 /
    // read by the fold kernel -- in coarse-grained memory a reader may keep
    // serving a stale cached line (round 3 recorded such a hang on a flag)
    SQ_HIP(hipExtMallocWithFlags(reinterpret_cast<void **>(&c->mbox), kMbWords * sizeof(unsigned int),
                                 hipDeviceMallocFinegrained));
    SQ_HIP(hipMemset(c->mbox, 0, kMbWords * sizeof(unsigned int)));
    const size_t need = std::max({(size_t)8 * (size_t)c->Lz, (size_t)8 * sq::kStabSlots * (size_t)std::max(1, p.loops),
                                  (size_t)256});
    c->coll_cap = (need + 255) / 256 * 256;
    SQ_HIP(hipExtMallocWithFlags(reinterpret_cast<void **>(&c->coll), 2 * (size_t)p.nranks * c->coll_cap,
                                 hipDeviceMallocFinegrained));
    c->peers.assign(p.nranks, Peer{});
    c->peers[p.rank] = Peer{c->slabs[0].stage, c->mbox, c->coll, false};
    c->p2p_ready = p.nranks == 1;  // one rank: its own buffers, nothing to map
    return SQ_OK;
}

// sq_destroy: false when the drain failed (the caller then leaks rather than
// free memory a peer may still read).
bool p2p_drain(sq_ctx *c) {
    bool p2p_drained = true;
    if (c->p2p_ready && c->xchg_seq > 0 && !c->slabs.empty() && c->slabs[0].sB) {
        // P2P: our staged copy may still be read by a neighbour that is behind;
        // free it only after both have acknowledged the last exchange (bounded
        // wait: a peer that died leaves the buffers mapped, not a hang)
        // (exchanges do not acknowledge one by one, phi4_block: the last one is
        // acknowledged here, behind our own pulls of it on the exchange stream)
        hipStream_t sB = c->slabs[0].sB;
        const int P = c->p.nranks, r = c->p.rank;
        const int up = (r + 1) % P, dn = (r + P - 1) % P;
        // with the exchange in order on stream A (SQ_XCHG_ON_A) our last pulls
        // ran there: the acknowledgements on stream B must follow them (the
        // hand-shake's bounded poll ends stream A's work even if a peer died)
        (void)hipStreamSynchronize(c->slabs[0].sA);
        if (hipStreamWriteValue32(sB, c->peers[dn].mbox + kMbAckFromUp, c->xchg_seq, 0) != hipSuccess ||
            hipStreamWriteValue32(sB, c->peers[up].mbox + kMbAckFromDn, c->xchg_seq, 0) != hipSuccess ||
            wait_seq(sB, c->mbox + kMbAckFromDn, c->xchg_seq) != hipSuccess ||
            wait_seq(sB, c->mbox + kMbAckFromUp, c->xchg_seq) != hipSuccess)
            p2p_drained = false;
        const auto t0 = std::chrono::steady_clock::now();
        while (p2p_drained && hipStreamQuery(sB) == hipErrorNotReady) {
            if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60)) p2p_drained = false;
            std::this_thread::sleep_for(std::chrono::microseconds(200));
        }
    }
    return p2p_drained;
}

void p2p_close_peers(sq_ctx *c) {
    for (Peer &o : c->peers)
        if (o.mapped) {
            (void)hipIpcCloseMemHandle(o.stage);
            (void)hipIpcCloseMemHandle(o.mbox);
            (void)hipIpcCloseMemHandle(o.coll);
            o = Peer{};
        }
}

void release_p2p(sq_ctx *c) {
    (void)hipFree(c->mbox);
    (void)hipFree(c->coll);
    c->mbox = nullptr;
    c->coll = nullptr;
    c->peers.clear();
    c->p2p_ready = false;
}

void release_rccl(sq_ctx *c) {
    if (c->comm) (void)ncclCommDestroy(c->comm);
    c->comm = nullptr;
}

}  // namespace sq

extern "C" {

int sq_comm_unique_id(unsigned char out[128]) {
    if (!out) return fail(SQ_E_ARG, "null argument");
    ncclUniqueId id;
    SQ_NCCL(ncclGetUniqueId(&id));
    memset(out, 0, 128);
    memcpy(out, id.internal, sizeof(id.internal));
    return SQ_OK;
}

int sq_p2p_handle(sq_ctx *c, unsigned char out[SQ_P2P_HANDLE_BYTES]) {
    if (!c || !out) return fail(SQ_E_ARG, "null argument");
    if (!is_phi4(c) || c->p.comm != SQ_COMM_P2P) return fail(SQ_E_STATE, "not an SQ_COMM_P2P context");
    DeviceGuard g(c->dev);
    P2pBlob b{};
    b.magic = kP2pMagic;
    b.version = SQ_ABI_VERSION;
    b.rank = c->p.rank;
    b.nranks = c->p.nranks;
    b.Lx = c->Lx;
    b.Ly = c->Ly;
    b.gpad = c->gpad;
    b.loops = c->p.loops;
    b.gz = c->gz;
    b.gauto = c->g_auto ? 1 : 0;
    b.ef_auto = c->ef_auto ? 1 : 0;
    b.k_auto = c->k_auto ? 1 : 0;
    b.edge_first = c->edge_first ? 1 : 0;
    b.core_pairs = c->core_pairs;
    b.rims_b = c->rims_b ? 1 : 0;
    b.a_auto = c->a_auto ? 1 : 0;
    b.on_a = c->xchg_on_a ? 1 : 0;
    b.kstage = c->kstage_env;
    b.Lz = c->Lz;
    b.coll_cap = (long long)c->coll_cap;
    b.seed = c->p.seed;
    SQ_HIP(hipIpcGetMemHandle(&b.stage, c->slabs[0].stage));
    SQ_HIP(hipIpcGetMemHandle(&b.mbox, c->mbox));
    SQ_HIP(hipIpcGetMemHandle(&b.coll, c->coll));
    memset(out, 0, SQ_P2P_HANDLE_BYTES);
    memcpy(out, &b, sizeof b);
    return SQ_OK;
}

int sq_p2p_connect(sq_ctx *c, const unsigned char *handles, int nranks) {
    if (!c || !handles) return fail(SQ_E_ARG, "null argument");
    if (!is_phi4(c) || c->p.comm != SQ_COMM_P2P) return fail(SQ_E_STATE, "not an SQ_COMM_P2P context");
    if (nranks != c->p.nranks) return fail(SQ_E_ARG, "handle count != nranks");
    if (c->p2p_ready && nranks > 1) return fail(SQ_E_STATE, "already connected");
    if (nranks == 1) return SQ_OK;
    std::vector<P2pBlob> bl(nranks);
    for (int q = 0; q < nranks; ++q) {  // validate every blob before mapping anything
        memcpy(&bl[q], handles + (size_t)q * SQ_P2P_HANDLE_BYTES, sizeof(P2pBlob));
        const P2pBlob &b = bl[q];
        if (b.magic != kP2pMagic || b.version != SQ_ABI_VERSION) return fail(SQ_E_ARG, "not a P2P handle blob");
        if (b.rank != q || b.nranks != nranks)
            return fail(SQ_E_ARG, "handle " + std::to_string(q) + " belongs to rank " + std::to_string(b.rank) +
                                      " of " + std::to_string(b.nranks) + " (blobs must be in rank order)");
        if (b.Lx != c->Lx || b.Ly != c->Ly || b.Lz != c->Lz || b.gpad != c->gpad ||
            b.coll_cap != (long long)c->coll_cap || b.seed != c->p.seed)
            return fail(SQ_E_ARG, "rank " + std::to_string(q) + " was created for a different lattice, ghost depth or seed");
        // the exchanges move gz planes and the frame collectives loops records:
        // ranks that disagree would hang in a wait or fold mismatched records
        if (b.loops != c->p.loops || b.gz != c->gz || b.gauto != (c->g_auto ? 1 : 0))
            return fail(SQ_E_ARG, "rank " + std::to_string(q) + " has different loops (" + std::to_string(b.loops) +
                                      "), active ghost depth (" + std::to_string(b.gz) + ") or ghost tuning (SQ_GHOST)");
        if (b.ef_auto != (c->ef_auto ? 1 : 0) || b.k_auto != (c->k_auto ? 1 : 0) ||
            b.edge_first != (c->edge_first ? 1 : 0) || b.core_pairs != c->core_pairs || b.rims_b != (c->rims_b ? 1 : 0) ||
            b.a_auto != (c->a_auto ? 1 : 0) || b.on_a != (c->xchg_on_a ? 1 : 0) || b.kstage != c->kstage_env)
            return fail(SQ_E_ARG, "rank " + std::to_string(q) + " has a different block schedule (SQ_EDGE_FIRST, "
                                      "SQ_CORE_PAIRS, SQ_RIMS_B, SQ_XCHG_ON_A, SQ_P2P_KSTAGE must be set alike on every rank)");
    }
    DeviceGuard g(c->dev);
    for (int q = 0; q < nranks; ++q) {
        if (q == c->p.rank) continue;
        Peer pr{};
        void *a = nullptr, *m = nullptr, *k = nullptr;
        hipError_t e = hipIpcOpenMemHandle(&a, bl[q].stage, hipIpcMemLazyEnablePeerAccess);
        if (e == hipSuccess) e = hipIpcOpenMemHandle(&m, bl[q].mbox, hipIpcMemLazyEnablePeerAccess);
        if (e == hipSuccess) e = hipIpcOpenMemHandle(&k, bl[q].coll, hipIpcMemLazyEnablePeerAccess);
        if (e != hipSuccess) {
            for (void *v : {a, m, k})
                if (v) (void)hipIpcCloseMemHandle(v);
            p2p_close_peers(c);
            return fail(SQ_E_COMM, std::string("hipIpcOpenMemHandle (rank ") + std::to_string(q) + "): " +
                                       hipGetErrorString(e));
        }
        pr.stage = static_cast<float *>(a);
        pr.mbox = static_cast<unsigned int *>(m);
        pr.coll = static_cast<unsigned char *>(k);
        pr.mapped = true;
        c->peers[q] = pr;
    }
    c->p2p_ready = true;
    return SQ_OK;
}

}  // extern "C"
