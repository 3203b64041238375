// sq_phi4_plan.cpp -- the schedule of a deep-halo block as a list of ops
// (pure host code: sq_phi4_block_plan exports it, phi4_block in
// sq_phi4_steps.cpp executes it) and the timed pick's choice.
#include <algorithm>

#include "sq_ctx.h"

using namespace sq;

namespace sq {

// The schedule of a deep-halo block of g <= G steps on a slab of nz planes
// with a ghost zone of G planes.  Each op names its stream:
// A (interior) or B (exchange, and the rims when rims_b).
//   EXCHANGE     stream B, after the previous block's EDGES_DONE: G edge planes
//                of the block's input field to both z-neighbours, their ghosts in.
//   Step k updates the shrinking extended range [-(g-1-k), nz+g-1-k),
//   recomputing ghost-zone sites.  With fuse2 (two steps per launch) and g >= 3
//   every step runs in pairs, and the first K pairs (kc = core pairs) are split:
//     PAIR 2j core  stream A, step 2j+1 on [2j+2, nz-2j-2), j < K: reads no ghost
//                   (step s is valid without ghosts on [s+1, nz-s-1)), so the
//                   core pairs overlap the exchange;
//     PAIR 2j rim   step 2j+1 on [-(g-2-2j), 2j+2) u [nz-2j-2, nz+g-2-2j) (two
//                   ranges, one launch), either on stream A after WAIT_EXCHANGE
//                   (short exchanges: no cross-stream hop before the next pair),
//                   or, rims_b, on stream B right behind the exchange, rim j > 0
//                   after core j-1 (SIGNAL A / WAIT B on slot j-1), stream A
//                   continuing once they are in (SIGNAL B / WAIT A on kRimSlot):
//                   long exchanges then overlap the cores with the rims too;
//     K = 0: no split -- stream A waits for the exchange and the first pair
//                   covers the whole range (an exchange shorter than the
//                   previous block's last middle pair is then hidden for free);
//     PAIR s        stream A, the remaining pairs on step s+1's whole range;
//     the last pair (or single step) computes its edge planes [0, G) u
//     [nz-G, nz) first and marks EDGES_DONE, so the NEXT block's exchange
//     overlaps this step's middle as well as the next cores (when the core
//     pairs reach the last step, EDGES_DONE follows the rims);
//   without fuse2 (or g < 3) step 0 is a single-step core [1, nz-1) and rim
//   [-(g-1), 1) u [nz-1, nz+g-1) (K = 0: one span), the later steps single
//   launches on A.
// Ghost-zone sites are recomputed redundantly; the counter-based noise makes
// them bit-identical to their owner's, so the result equals the monolithic run.
// Buffers: a launch group (the ops of one first step) reads the buffer of the
// step before it and writes the other (phi4_block counts the groups); a core
// pair running ahead of the rims only writes [2j+2, nz-2j-2), which no earlier
// rim pair reads ([.., 2i+4) u [nz-2i-4, ..) for i < j).
// (kPlanSlots, kRimSlot, kA, kB: sq_ctx.h)
std::vector<sq_block_op> block_plan(int nz, int G, int g, bool fuse2, bool edge_first, int kc, bool rims_b) {
    std::vector<sq_block_op> ops;
    auto add = [&](int kind, int step, int lo, int hi, int lo2, int hi2, int stream) {
        ops.push_back(sq_block_op{kind, step, lo, hi, lo2, hi2, stream});
    };
    const int rs = rims_b ? kB : kA;  // the rims' stream
    auto rims_done = [&]() {
        if (!rims_b) return;
        add(SQ_OP_SIGNAL, 0, kRimSlot, 0, 0, 0, kB);
        add(SQ_OP_WAIT, 0, kRimSlot, 0, 0, 0, kA);
    };
    const bool split_edges = edge_first && nz > 2 * G;
    add(SQ_OP_EXCHANGE, 0, 0, 0, 0, 0, kB);
    int st;
    bool edges = false;
    if (kc <= 0) {  // no core/rim split
        add(SQ_OP_WAIT_EXCHANGE, 0, 0, 0, 0, 0, kA);
        st = 0;
    } else if (fuse2 && g >= 3) {
        // core pairs: at least one, at most the pairs of the block, and only
        // while the core is not empty
        int K = std::max(1, std::min(std::min(kc, g / 2), kRimSlot));
        while (K > 1 && nz <= 4 * K) --K;
        // core pair 1 writes step 3 into the buffer the exchange sends its edge
        // planes from: with K >= 2 the exchange sends a staged copy of them, and
        // core pair 1 waits only for that copy
        if (K >= 2) ops[0].lo = 1;
        int nc = 0;
        for (int j = 0; j < K && nz > 4 * j + 4; ++j, ++nc) {
            if (j == 1) add(SQ_OP_WAIT_STAGED, 0, 0, 0, 0, 0, kA);
            add(SQ_OP_PAIR, 2 * j, 2 * j + 2, nz - 2 * j - 2, 0, 0, kA);
            if (rims_b && j + 1 < K) add(SQ_OP_SIGNAL, 2 * j, j, 0, 0, 0, kA);
        }
        add(SQ_OP_WAIT_EXCHANGE, 0, 0, 0, 0, 0, rs);
        for (int j = 0; j < K; ++j) {
            if (rims_b && j > 0 && j - 1 < nc) add(SQ_OP_WAIT, 2 * j, j - 1, 0, 0, 0, kB);
            const int lo_a = -(g - 2 - 2 * j), hi_a = 2 * j + 2, lo_b = nz - 2 * j - 2, hi_b = nz + g - 2 - 2 * j;
            if (hi_a >= lo_b)  // rims meet (no core): one span
                add(SQ_OP_PAIR, 2 * j, lo_a, hi_b, 0, 0, rs);
            else
                add(SQ_OP_PAIR, 2 * j, lo_a, hi_a, lo_b, hi_b, rs);
        }
        rims_done();
        st = 2 * K;
    } else {
        if (nz - 1 > 1) add(SQ_OP_STEP, 0, 1, nz - 1, 0, 0, kA);
        add(SQ_OP_WAIT_EXCHANGE, 0, 0, 0, 0, 0, rs);
        const int lo_a = -(g - 1), hi_a = 1, lo_b = nz - 1, hi_b = nz + g - 1;
        if (hi_a >= lo_b)  // rims meet (nz <= 2): one span
            add(SQ_OP_STEP, 0, lo_a, hi_b, 0, 0, rs);
        else
            add(SQ_OP_STEP, 0, lo_a, hi_a, lo_b, hi_b, rs);
        rims_done();
        st = 1;
    }
    while (st < g) {
        const bool pair = fuse2 && st + 1 <= g - 1;
        const int last = pair ? st + 1 : st;  // the step this op group completes
        const int kind = pair ? SQ_OP_PAIR : SQ_OP_STEP;
        if (last == g - 1 && split_edges) {
            add(kind, st, 0, G, nz - G, nz, kA);
            add(SQ_OP_EDGES_DONE, st, 0, 0, 0, 0, kA);
            add(kind, st, G, nz - G, 0, 0, kA);
            edges = true;
        } else {
            const int e = g - 1 - last;  // ghost planes the completed step still updates on either side
            add(kind, st, -e, nz + e, 0, 0, kA);
        }
        st = last + 1;
    }
    if (!edges) add(SQ_OP_EDGES_DONE, g - 1, 0, 0, 0, 0, kA);
    return ops;
}

// The index of a plan's [PAIR core (A), WAIT_EXCHANGE (A), PAIR rim (A, two
// equal ranges)] of one step -- the K = 1, rims-on-A block start -- or -1.
int gate_pattern(const std::vector<sq_block_op> &ops) {
    for (size_t i = 0; i + 2 < ops.size(); ++i) {
        const sq_block_op &a = ops[i], &w = ops[i + 1], &r = ops[i + 2];
        if (a.kind == SQ_OP_PAIR && a.stream == kA && a.lo2 >= a.hi2 && w.kind == SQ_OP_WAIT_EXCHANGE &&
            w.stream == kA && r.kind == SQ_OP_PAIR && r.stream == kA && r.step == a.step && r.lo2 < r.hi2 &&
            r.hi - r.lo == r.hi2 - r.lo2)
            return (int)i;
        if (a.kind == SQ_OP_WAIT_EXCHANGE) return -1;  // the pattern is the block's start or absent
    }
    return -1;
}

}  // namespace sq

extern "C" {

int sq_phi4_block_plan(int nz, int ghost, int g, int fuse2, int edge_first, int core_pairs, int rims_b,
                       sq_block_op *ops, int cap, int *nops) {
    if (!nops || (cap > 0 && !ops)) return fail(SQ_E_ARG, "null argument");
    if (nz < 1 || ghost < 1 || g < 1 || g > ghost || ghost > nz) return fail(SQ_E_ARG, "need 1 <= g <= ghost <= nz");
    if (core_pairs < 0) return fail(SQ_E_ARG, "core_pairs must be >= 0");
    const std::vector<sq_block_op> v = block_plan(nz, ghost, g, fuse2 != 0, edge_first != 0, core_pairs, rims_b != 0);
    *nops = (int)v.size();
    if ((int)v.size() > cap) return fail(SQ_E_ARG, "cap too small: need " + std::to_string(v.size()));
    std::copy(v.begin(), v.end(), ops);
    return SQ_OK;
}

int sq_phi4_pick_ghost(const double *ms, int n) {
    int best = 0;
    for (int k = 1; k < n; ++k)
        if (ms[k] < ms[best]) best = k;
    return best;
}

}  // extern "C"
