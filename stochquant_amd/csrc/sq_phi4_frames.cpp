// sq_phi4_frames.cpp -- frames: the stability heuristic and the dtau
// controller, the host-decided PHI4 frame and the batches under
// the device controller, their record buffers; sq_run_frame / sq_run_frames
// for both models.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "sq_ctx.h"

using namespace sq;

namespace {

// Inverse of the kernels' order-preserving float -> uint map (sq_phi4.hip ord_f32).
float unord_f32(unsigned int o) {
    const unsigned int u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
    float f;
    memcpy(&f, &u, sizeof f);
    return f;
}

// Point st_md / st_a / flag at record set k of frame_rec (st_md | st_a | flag).
void use_rec_set(sq_ctx *c, int k) {
    const size_t nrec = (size_t)sq::kStabSlots * (size_t)std::max(c->p.loops, 0);
    char *b = static_cast<char *>(c->frame_rec) + (size_t)k * c->frame_bytes;
    c->rec_set = k;
    c->frame_cur = b;
    c->st_md = nrec > 0 ? reinterpret_cast<unsigned long long *>(b) : nullptr;
    c->st_a = nrec > 0 ? reinterpret_cast<unsigned int *>(b + nrec * sizeof(unsigned long long)) : nullptr;
    c->flag = reinterpret_cast<int *>(b + nrec * (sizeof(unsigned long long) + sizeof(unsigned int)));
}

// the device controller's states, their pinned mirror and the folded records
void free_frame_ctl(sq_ctx *c) {
    (void)hipFree(c->ctl);
    (void)hipFree(c->rec_dev);
    if (c->ctl_host) (void)hipHostFree(c->ctl_host);
    c->ctl = nullptr;
    c->rec_dev = nullptr;
    c->ctl_host = nullptr;
}

// a batch's per-frame verdicts and dtau, device and pinned
void free_frame_batch(sq_ctx *c) {
    (void)hipFree(c->fr_stable);
    (void)hipFree(c->fr_dtau);
    if (c->fr_stable_h) (void)hipHostFree(c->fr_stable_h);
    if (c->fr_dtau_h) (void)hipHostFree(c->fr_dtau_h);
    c->fr_stable = nullptr;  // a failed allocation below must not leave freed pointers for sq_destroy
    c->fr_dtau = nullptr;
    c->fr_stable_h = nullptr;
    c->fr_dtau_h = nullptr;
    c->fr_cap = 0;
}

}  // namespace

namespace sq {

// create_phi4: the two record sets and their pinned mirror.
int alloc_frame_records(sq_ctx *c) {
    const sq_params &p = c->p;
    const size_t nrec = (size_t)sq::kStabSlots * (size_t)std::max(p.loops, 0);
    c->frame_bytes = nrec * (sizeof(unsigned long long) + sizeof(unsigned int)) + 2 * sizeof(int);
    SQ_HIP(hipMalloc(&c->frame_rec, 2 * c->frame_bytes));
    SQ_HIP(hipMemset(c->frame_rec, 0, 2 * c->frame_bytes));
    SQ_HIP(hipHostMalloc(&c->frame_host, c->frame_bytes, hipHostMallocDefault));
    use_rec_set(c, 0);
    return SQ_OK;
}

void release_frames(sq_ctx *c) {
    if (c->frame_rec) {  // flag, st_md, st_a live in it
        (void)hipFree(c->frame_rec);
    } else {
        (void)hipFree(c->flag);
        (void)hipFree(c->st_md);
        (void)hipFree(c->st_a);
    }
    if (c->frame_host) (void)hipHostFree(c->frame_host);
    c->frame_rec = c->frame_cur = c->frame_host = nullptr;
    c->flag = nullptr;
    c->st_md = nullptr;
    c->st_a = nullptr;
    free_frame_ctl(c);
    free_frame_batch(c);
}

}  // namespace sq

namespace {

void adapt(sq_ctx *c, int stable) {  // tauhost.c:523-529,537-541
    if (!c->p.adapt_dtau) return;
    if (stable == 1) {
        if (c->stab_cnt > 10) {
            c->stab_cnt = 0;
            c->dtau /= 0.950;
        }
        c->stab_cnt++;
    } else {
        c->dtau *= 0.950;
        c->stab_cnt = 0;
    }
}

// max phi and max |phi| over the whole lattice (all slabs, all ranks).
int phi4_field_max(sq_ctx *c, float *mx_phi, float *mx_abs) {
    unsigned int m[2] = {0, 0};
    for (auto &s : c->slabs) {
        unsigned int t[2];
        SQ_HIP(sq::phi4_moments_launch(plane0(c, s, c->cur), (long long)s.nz * (long long)plane_floats(c), c->dacc,
                                       c->dmax, c->dpart, s.sA));
        int rc = rank_allreduce(c, c->dmax, 2, sq::P2pRed::kMaxU32, s.sA);
        if (rc) return rc;
        SQ_HIP(hipMemcpyAsync(t, c->dmax, sizeof t, hipMemcpyDeviceToHost, s.sA));
        SQ_HIP(hipStreamSynchronize(s.sA));
        m[0] = std::max(m[0], t[0]);
        m[1] = std::max(m[1], t[1]);
    }
    memcpy(mx_abs, &m[0], sizeof(float));
    *mx_phi = unord_f32(m[1]);
    return SQ_OK;
}

// The stability heuristic of tau_kernel.cl:135-143, restated for the 3-D
// lattice from per-step records: step j has a new leader when
// its maximum M_j exceeds T (the maximum of the step before, carried across
// frames); the frame is unstable at the first leader whose drift increment
// D_j = |phi' - phi - sigma xi| at the maximum exceeds V, the running maximum
// of |phi| of the steps before.  T and V are updated through that step (the
// reference breaks after it) and never rolled back.
int stab_rule(float &T, float &V, const float *M, const float *D, const float *A, int n) {
    for (int j = 0; j < n; ++j) {
        const bool fired = M[j] > T && D[j] > V;
        T = M[j];
        V = std::max(V, A[j]);
        if (fired) return j;
    }
    return -1;
}

// The frame snapshot: allocated padded like the slab's buffers, so the three
// can swap roles (three-buffer device frames); snap = its interior.
int ensure_snap(sq_ctx *c, Slab &s) {
    if (s.snap_pad) return SQ_OK;
    const size_t bytes = (size_t)(s.nz + 2 * c->gpad) * plane_floats(c) * sizeof(float);
    SQ_HIP(hipMalloc(&s.snap_pad, bytes));
    s.snap = s.snap_pad + (size_t)c->gpad * plane_floats(c);
    return SQ_OK;
}

int phi4_frame(sq_ctx *c, int *stable) {
    const size_t plane = plane_floats(c);
    // one slab without an exchange: every launch of the frame is on stream A,
    // so stream order replaces the joins around the set-up
    const bool one_stream = c->slabs.size() == 1 && c->p.comm == SQ_COMM_NONE;
    int rc = one_stream ? SQ_OK : phi4_join(c);
    if (rc) return rc;
    if (!c->stab_init) {  // the first frame's leader value and running max: the field itself
        rc = phi4_field_max(c, &c->stab_T, &c->stab_V);
        if (rc) return rc;
        c->stab_init = true;
    }
    const size_t nrec = (size_t)sq::kStabSlots * (size_t)c->p.loops;
    if (!c->frame_rec_zero)  // records and guard flag (normally cleared behind the previous read-back)
        SQ_HIP(hipMemsetAsync(c->frame_cur, 0, c->frame_bytes, c->slabs[0].sA));
    c->frame_rec_zero = false;
    // frame-start snapshot, kept on device: a one-stream frame that starts
    // with a fused pair has that launch store its input's interior (every
    // site once, nontemporal), otherwise a device copy
    const bool snap_in_kernel = one_stream && c->tbz > 0 && c->p.loops >= 2;
    for (auto &s : c->slabs) {
        const size_t bytes = (size_t)s.nz * plane * sizeof(float);
        rc = ensure_snap(c, s);
        if (rc) return rc;
        if (snap_in_kernel)
            c->snap_next = s.snap;
        else
            SQ_HIP(hipMemcpyAsync(s.snap, plane0(c, s, c->cur), bytes, hipMemcpyDeviceToDevice, s.sA));
    }
    rc = one_stream ? SQ_OK : phi4_join(c);
    if (rc) return rc;
    c->in_frame = true;
    c->kstage_pending = false;  // frames stage their exchanges by copy
    c->frame_step0 = c->step;
    // the agreed value: a rollback restores it on every rank alike (an
    // unagreed local value would let a rank with fin = 1 take the guard's fast
    // path on a neighbour's unguarded ghost planes after the rollback)
    rc = fin_agree(c);
    if (rc) return rc;
    const bool fin0 = c->field_finite;
    rc = phi4_steps(c, c->p.loops);
    c->in_frame = false;
    c->snap_next = nullptr;
    if (rc) return rc;
    rc = one_stream ? SQ_OK : phi4_join(c);
    if (rc) return rc;
    Slab &s0 = c->slabs[0];
    if (per_rank(c->p.comm) && c->p.nranks > 1) {
        const bool grp = c->p.comm == SQ_COMM_RCCL;
        if (grp) SQ_NCCLW(c, ncclGroupStart());
        rc = rank_allreduce(c, c->flag, 1, sq::P2pRed::kMaxI32, s0.sA);
        if (!rc) rc = rank_allreduce(c, c->st_md, nrec, sq::P2pRed::kMaxU64, s0.sA);
        if (!rc) rc = rank_allreduce(c, c->st_a, nrec, sq::P2pRed::kMaxU32, s0.sA);
        if (grp) SQ_NCCLW(c, ncclGroupEnd());
        if (rc) return rc;
    }
    // one read-back of the records and the flag into pinned memory
    SQ_HIP(hipMemcpyAsync(c->frame_host, c->frame_cur, c->frame_bytes, hipMemcpyDeviceToHost, s0.sA));
    // clear the records for the next frame behind the read-back (stream order), off its start
    SQ_HIP(hipMemsetAsync(c->frame_cur, 0, c->frame_bytes, s0.sA));
    c->frame_rec_zero = true;
    SQ_HIP(hipStreamSynchronize(s0.sA));
    rc = gate_check(c, true);  // a timed-out rim chunk: no verdict from a corrupt field
    if (rc) return rc;
    const char *hb = static_cast<const char *>(c->frame_host);
    const unsigned long long *md = reinterpret_cast<const unsigned long long *>(hb);
    const unsigned int *am = reinterpret_cast<const unsigned int *>(hb + nrec * sizeof(unsigned long long));
    const int h = *reinterpret_cast<const int *>(hb + nrec * (sizeof(unsigned long long) + sizeof(unsigned int)));
    const int L = c->p.loops;
    c->rec_M.assign(L, 0.f);
    c->rec_D.assign(L, 0.f);
    c->rec_A.assign(L, 0.f);
    for (int j = 0; j < L; ++j) {
        unsigned long long k = 0;
        unsigned int a = 0;
        for (int i = 0; i < sq::kStabSlots; ++i) {
            k = std::max(k, md[(size_t)j * sq::kStabSlots + i]);
            a = std::max(a, am[(size_t)j * sq::kStabSlots + i]);
        }
        c->rec_M[j] = unord_f32((unsigned int)(k >> 32));
        const unsigned int db = (unsigned int)k;
        memcpy(&c->rec_D[j], &db, sizeof(float));
        memcpy(&c->rec_A[j], &a, sizeof(float));
    }
    c->stab_fired = stab_rule(c->stab_T, c->stab_V, c->rec_M.data(), c->rec_D.data(), c->rec_A.data(), L);
    *stable = (h == 0 && c->stab_fired < 0) ? 1 : 0;
    if (!*stable) {  // rollback from the device snapshot; the noise counter is NOT rewound,
                     // so a retried frame draws fresh noise (as the reference's LCG state)
        c->field_finite = fin0;
        for (auto &s : c->slabs)
            SQ_HIP(hipMemcpyAsync(plane0(c, s, c->cur), s.snap, (size_t)s.nz * plane * sizeof(float),
                                  hipMemcpyDeviceToDevice, s.sA));
        rc = phi4_join(c);
        if (rc) return rc;
    }
    return SQ_OK;
}

// Frames back to back under the device controller: per frame
// the launches of phi4_frame (snapshot from the first fused launch, the frame
// instances with the guard flag and the records), then phi4_frame_ctl_kernel
// (record fold, stab_rule, Δτ) and phi4_rollback_kernel (a no-op when
// stable); the launches of frame f+1 read the coefficients frame f's
// controller wrote.  One read-back at the end of the batch.  Bit-identical to
// the host path (phi4_frame + adapt) in field, verdicts, Δτ, T/V and records.
// One slab without an exchange; other decompositions (and loops < 1, a field
// not yet through the guard, SQ_FRAME_HOST=1) take the host path per frame.
int phi4_frames_dev(sq_ctx *c, int n, int *stable, double *dtau_out) {
    const int L = c->p.loops;
    const bool one_stream = c->slabs.size() == 1 && c->p.comm == SQ_COMM_NONE;
    const char *fh = getenv("SQ_FRAME_HOST");
    const bool host_only = !one_stream || L < 1 || c->st_md == nullptr || (fh && atoi(fh) != 0) ||
                           ((size_t)c->slabs[0].nz * plane_floats(c)) % 4 != 0;
    int f = 0;
    while (f < n && (host_only || !c->field_finite)) {  // host path (rollback restores fin0 = false)
        int rc = phi4_frame(c, &stable[f]);
        if (rc) return rc;
        adapt(c, stable[f]);
        if (dtau_out) dtau_out[f] = c->dtau;
        ++f;
    }
    if (f == n) return SQ_OK;
    Slab &s0 = c->slabs[0];
    const hipStream_t st = s0.sA;
    const size_t plane = plane_floats(c), nfl = (size_t)s0.nz * plane;
    if (!c->stab_init) {
        int rc = phi4_field_max(c, &c->stab_T, &c->stab_V);
        if (rc) return rc;
        c->stab_init = true;
    }
    if (!c->ctl || !c->ctl_host || !c->rec_dev) {  // all three, or none after a failure
        free_frame_ctl(c);
        SQ_HIP(hipMalloc(&c->ctl, 2 * sizeof(sq::FrameCtl)));
        SQ_HIP(hipHostMalloc(&c->ctl_host, sizeof(sq::FrameCtl), hipHostMallocDefault));
        SQ_HIP(hipMalloc(&c->rec_dev, 3 * sizeof(float) * (size_t)L));
    }
    {
        int rc = ensure_snap(c, s0);
        if (rc) return rc;
    }
    const int m = n - f;
    if (m > c->fr_cap) {
        free_frame_batch(c);
        SQ_HIP(hipMalloc(&c->fr_stable, sizeof(int) * (size_t)m));
        SQ_HIP(hipMalloc(&c->fr_dtau, sizeof(double) * (size_t)m));
        SQ_HIP(hipHostMalloc(&c->fr_stable_h, sizeof(int) * (size_t)m, hipHostMallocDefault));
        SQ_HIP(hipHostMalloc(&c->fr_dtau_h, sizeof(double) * (size_t)m, hipHostMallocDefault));
        c->fr_cap = m;
    }
    // the controller starts from the host's state (a caller may have set Δτ or T/V)
    sq::FrameCtl &h = *c->ctl_host;
    memset(&h, 0, sizeof h);
    h.dtau = c->dtau;
    h.C = c->p.C;
    const float hf = (float)c->dtau;  // as phi4_base_args
    h.coef[0] = hf;
    h.coef[1] = (float)(sqrt(2.0 * (double)hf) * c->p.C);
    h.coef[2] = (float)(sqrt(2.0 * (double)hf) * c->p.C * sq::kSqrt2Ln2);
    h.T = c->stab_T;
    h.V = c->stab_V;
    h.stab_cnt = c->stab_cnt;
    h.adapt = c->p.adapt_dtau ? 1 : 0;
    h.stable = 1;
    h.fired = -1;
    // three buffers (the slab's two and the padded snapshot allocation): a
    // frame never writes the buffer it starts from, so that buffer is its
    // rollback -- no snapshot store, no copy back (SQ_FRAME_TRI=0: off)
    const char *ft = getenv("SQ_FRAME_TRI");
    const bool tri = c->tbz > 0 && L >= 2 && !(ft && atoi(ft) == 0);
    if (tri) {
        c->tri_bufs[0] = s0.buf[c->cur];
        c->tri_bufs[1] = s0.buf[c->cur ^ 1];
        c->tri_bufs[2] = s0.snap_pad;
        h.tri = 1;
        h.bs = 0;
        h.bw0 = 1;
        h.bw1 = 2;
        h.nl_odd = ((L / 2) + (L & 1)) & 1;  // launches per frame: the pairs and an odd last step
    }
    c->spec_bs = 0;  // the guess starts from the roles the controller starts from
    c->spec_bw0 = 1;
    c->spec_bw1 = 2;
    {
        const char *fs = getenv("SQ_FRAME_SPEC");
        c->tri_spec = !(fs && atoi(fs) == 0);
    }
    SQ_HIP(hipMemcpyAsync(c->ctl, c->ctl_host, sizeof h, hipMemcpyHostToDevice, st));
    // the active record set must start zero; each frame-end launch clears the
    // other one, which the next frame then uses
    if (!c->frame_rec_zero) SQ_HIP(hipMemsetAsync(c->frame_cur, 0, c->frame_bytes, st));
    const bool snap_in_kernel = c->tbz > 0 && L >= 2;
    // frame i > 0's first fused launch takes frame i-1's end (FrameFoldArgs):
    // frames of 4..kFoldMaxL steps (the launch after the first, a fused pair
    // too, clears the folded set); SQ_FRAME_FOLD=0 keeps one end launch per frame
    const char *ff = getenv("SQ_FRAME_FOLD");
    const bool fold = snap_in_kernel && L >= 4 && L <= sq::kFoldMaxL && !(ff && atoi(ff) == 0);
    // diagnostic only (profiles/r04/frames/): no snapshot store, so a rolled-back
    // frame restores garbage -- prices the store on stable frames
    const char *dns = getenv("SQ_DIAG_NO_SNAP");
    const bool diag_no_snap = dns && atoi(dns) != 0;
    c->tri = tri;
    for (int i = 0; i < m; ++i) {
        if (tri)
            c->snap_next = nullptr;
        else if (snap_in_kernel)
            c->snap_next = diag_no_snap ? nullptr : s0.snap;
        else
            SQ_HIP(hipMemcpyAsync(s0.snap, plane0(c, s0, c->cur), nfl * sizeof(float), hipMemcpyDeviceToDevice, st));
        c->in_frame = true;
        c->kstage_pending = false;  // frames stage their exchanges by copy
        c->dev_frames = true;
        c->ctl_cur = c->ctl + (i & 1);
        c->frame_step0 = c->step;
        c->frame_tk = 0;
        c->clr_armed = false;
        if (fold && i == 0 && m > 1) {
            // the other record set still holds the previous batch's last frame:
            // frame 0's second launch clears it for frame 1
            const int cur_set = c->rec_set;
            use_rec_set(c, cur_set ^ 1);
            c->clr_next = sq::RecClear{c->st_md, c->st_a, c->flag, L * sq::kStabSlots};
            use_rec_set(c, cur_set);
            c->clr_first = true;
        }
        int rc = phi4_steps(c, L);
        if (tri) {  // the next frame's roles if this one is stable (frame_decide's rotation)
            const int fin = h.nl_odd ? c->spec_bw0 : c->spec_bw1;
            const int third = 3 - c->spec_bs - fin;
            c->spec_bw1 = c->spec_bs;
            c->spec_bs = fin;
            c->spec_bw0 = third;
        }
        c->in_frame = false;
        c->dev_frames = false;
        c->snap_next = nullptr;
        c->fold_next = sq::FrameFoldArgs{};
        c->clr_armed = false;
        c->clr_first = false;
        if (rc) {
            c->tri = false;
            return rc;
        }
        if (fold && i + 1 < m) {
            // frame i+1's first launch decides frame i: it folds this record
            // set and writes ctl[(i+1)&1]; frame i+1 accumulates into the other
            // set (cleared by frame i's second launch)
            sq::FrameFoldArgs fa{};
            fa.cin = c->ctl + (i & 1);
            fa.cout = c->ctl + ((i + 1) & 1);
            fa.md = c->st_md;
            fa.am = c->st_a;
            fa.flag = c->flag;
            fa.rec = c->rec_dev;
            fa.stable_out = c->fr_stable + i;
            fa.dtau_out = c->fr_dtau + i;
            fa.snap = s0.snap;
            fa.L = L;
            sq::RecClear cl{};
            cl.md = c->st_md;
            cl.am = c->st_a;
            cl.flag = c->flag;
            cl.n = L * sq::kStabSlots;
            use_rec_set(c, c->rec_set ^ 1);
            c->fold_next = fa;
            c->clr_next = cl;
            continue;
        }
        sq::FrameEndArgs e{};
        e.cin = c->ctl + (i & 1);
        e.cout = c->ctl + ((i + 1) & 1);
        e.md = c->st_md;
        e.am = c->st_a;
        e.flag = c->flag;
        const int cur_set = c->rec_set;
        use_rec_set(c, cur_set ^ 1);
        e.md_next = c->st_md;
        e.am_next = c->st_a;
        e.flag_next = c->flag;
        e.L = L;
        e.rec = c->rec_dev;
        e.stable_out = c->fr_stable + i;
        e.dtau_out = c->fr_dtau + i;
        e.dst = reinterpret_cast<float4 *>(plane0(c, s0, c->cur));
        e.snap = reinterpret_cast<const float4 *>(s0.snap);
        e.n4 = tri ? 0 : (long long)(nfl / 4);  // three buffers: the rollback is the next start buffer
        SQ_HIP(sq::phi4_frame_end_launch(e, st));
        c->perf.kernel_launches += 1;
    }
    c->tri = false;
    c->frame_rec_zero = true;  // the active set is the one the last frame-end launch cleared
    SQ_HIP(hipMemcpyAsync(c->ctl_host, c->ctl + (m & 1), sizeof h, hipMemcpyDeviceToHost, st));
    SQ_HIP(hipMemcpyAsync(c->fr_stable_h, c->fr_stable, sizeof(int) * (size_t)m, hipMemcpyDeviceToHost, st));
    SQ_HIP(hipMemcpyAsync(c->fr_dtau_h, c->fr_dtau, sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, st));
    SQ_HIP(hipMemcpyAsync(c->frame_host, c->rec_dev, 3 * sizeof(float) * (size_t)L, hipMemcpyDeviceToHost, st));
    SQ_HIP(hipStreamSynchronize(st));
    for (int i = 0; i < m; ++i) {
        stable[f + i] = c->fr_stable_h[i];
        if (dtau_out) dtau_out[f + i] = c->fr_dtau_h[i];
    }
    c->dtau = h.dtau;
    c->stab_cnt = h.stab_cnt;
    c->stab_T = h.T;
    c->stab_V = h.V;
    c->stab_fired = h.fired;
    if (tri) {  // the field is the start buffer of the frame after the batch: make it buf[0]
        if (h.bs < 0 || h.bs > 2) return fail(SQ_E_STATE, "device frames: corrupt buffer rotation");
        float *b[3] = {c->tri_bufs[h.bs], c->tri_bufs[(h.bs + 1) % 3], c->tri_bufs[(h.bs + 2) % 3]};
        s0.buf[0] = b[0];
        s0.buf[1] = b[1];
        s0.snap_pad = b[2];
        s0.snap = b[2] + (size_t)c->gpad * plane;
        c->cur = 0;
    }
    const float *r = static_cast<const float *>(c->frame_host);
    c->rec_M.assign(r, r + L);
    c->rec_D.assign(r + L, r + 2 * L);
    c->rec_A.assign(r + 2 * L, r + 3 * L);
    return SQ_OK;
}

}  // namespace

extern "C" {

int sq_run_frame(sq_ctx *c, int *stable) {
    if (!c || !stable) return fail(SQ_E_ARG, "null argument");
    DeviceGuard g(c->dev);
    const auto t0 = std::chrono::steady_clock::now();
    // one frame: the host-decided path (one read-back, 454 vs 478 us per 256^3
    // 20-step frame for the device controller's state upload and read-back);
    // sq_run_frames keeps the decisions on the device across frames
    int rc = is_phi4(c) ? gate_check(c, false) : SQ_OK;
    if (!rc) rc = is_phi4(c) ? phi4_frame(c, stable) : qm1d_frame(c, stable);
    if (rc) return rc;
    adapt(c, *stable);
    c->perf.frame_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SQ_OK;
}

int sq_run_frames(sq_ctx *c, int nframes, int *stable, double *dtau) {
    if (!c || (!stable && nframes > 0)) return fail(SQ_E_ARG, "null argument");
    if (nframes < 0) return fail(SQ_E_ARG, "nframes < 0");
    DeviceGuard g(c->dev);
    const auto t0 = std::chrono::steady_clock::now();
    if (is_phi4(c)) {
        int rc = gate_check(c, false);
        if (!rc) rc = phi4_frames_dev(c, nframes, stable, dtau);
        if (rc) return rc;
    } else {
        for (int f = 0; f < nframes; ++f) {
            int rc = qm1d_frame(c, &stable[f]);
            if (rc) return rc;
            adapt(c, stable[f]);
            if (dtau) dtau[f] = c->dtau;
        }
    }
    c->perf.frame_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SQ_OK;
}

int sq_phi4_stability(sq_ctx *c, double state[2], int *fired_step, float *M, float *D, float *A, int n) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "PHI4 only");
    if (n < 0 || (n > 0 && (!M || !D || !A))) return fail(SQ_E_ARG, "bad record arguments");
    if (n > (int)c->rec_M.size()) return fail(SQ_E_ARG, "n exceeds the last frame's steps");
    if (state) {
        state[0] = c->stab_T;
        state[1] = c->stab_V;
    }
    if (fired_step) *fired_step = c->stab_fired;
    for (int j = 0; j < n; ++j) {
        M[j] = c->rec_M[j];
        D[j] = c->rec_D[j];
        A[j] = c->rec_A[j];
    }
    return SQ_OK;
}

}  // extern "C"

namespace sq {
int frame_state_get(const sq_ctx *c, FrameState *fs) {
    if (!c || !fs) return fail(SQ_E_ARG, "null argument");
    fs->T = c->stab_T;
    fs->V = c->stab_V;
    fs->init = c->stab_init ? 1 : 0;
    fs->stab_cnt = c->stab_cnt;
    return SQ_OK;
}
int frame_state_set(sq_ctx *c, const FrameState &fs) {
    if (!c) return fail(SQ_E_ARG, "null argument");
    if (fs.stab_cnt < 0) return fail(SQ_E_ARG, "stab_cnt must be >= 0");
    c->stab_T = fs.T;
    c->stab_V = fs.V;
    c->stab_init = fs.init != 0;
    c->stab_cnt = fs.stab_cnt;
    return SQ_OK;
}
}  // namespace sq

extern "C" {

int sq_phi4_set_stability(sq_ctx *c, double T, double V) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "PHI4 only");
    c->stab_T = (float)T;
    c->stab_V = (float)V;
    c->stab_init = true;
    return SQ_OK;
}

int sq_set_noise(sq_ctx *c, double C) {
    if (!c) return fail(SQ_E_ARG, "null context");
    // the PHI4 guard fast path bounds |sigma xi| by 16 sqrt(2 dtau) |C| (create_phi4), dtau <= 1e20
    if (!std::isfinite(C) || std::fabs(C) > 1e12) return fail(SQ_E_ARG, "C must be finite, |C| <= 1e12");
    if (is_phi4(c)) {  // create_phi4's bound with the new C at the current dtau
        const double cl = c->p.clamp, h = c->dtau;
        const double drift = 12.0 * cl + std::fabs(c->p.m2) * cl + std::fabs(c->p.lambda) / 6.0 * cl * cl * cl;
        if (!(h * drift + cl + 16.0 * sqrt(2.0 * h) * std::fabs(C) < 1e30))
            return fail(SQ_E_ARG, "C too large for the guard's fast path at this dtau (dtau * drift + noise >= 1e30)");
    }
    c->p.C = C;
    return SQ_OK;
}

}  // extern "C"
