// sq_phi4_hmc.cpp -- HMC trajectories of the single phi^4 lattice: sq_phi4_step_hmc,
// sq_phi4_hmc_stats, sq_phi4_hmc_reset (include/stochquant.h; the kernels and the
// design are sq_phi4_hmc.hip's).  A call is one stream of launches on the slab's
// step stream; the host reads nothing back between trajectories.
#include <cmath>
#include <cstring>
#include <utility>

#include "sq_ctx.h"
#include "sq_phi4_hmc.h"

using namespace sq;

namespace {

// Philox4x32-10 (sq_rng.h's philox4x32_10, which is device code), for the
// trajectory length the host must know to enqueue L - 1 leap launches.
void philox_host(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += kPhiloxW0;
            k1 += kPhiloxW1;
        }
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c[0], p1 = (uint64_t)kPhiloxM1 * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = (uint32_t)p1;
        c[2] = n2;
        c[3] = (uint32_t)p0;
    }
}

int hmc_length(const sq_ctx *c, int nleap, int randomize) {
    if (!randomize) return nleap;
    uint32_t o[4] = {0u, kStreamAccept << 24, (uint32_t)c->step, (uint32_t)(c->step >> 32)};
    philox_host(o, (uint32_t)c->p.seed, (uint32_t)(c->p.seed >> 32));
    return 1 + (int)(((unsigned long long)o[1] * (unsigned long long)(uint32_t)nleap) >> 32);
}

float hmc_sigma(const sq_ctx *c) { return (float)(sqrt(2.0 * (double)(float)c->dtau) * c->p.C); }  // phi4_base_args' sig

// The checks every entry point shares: a PHI4 context of one periodic slab.
int hmc_ctx_check(sq_ctx *c) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "HMC trajectories are for PHI4 contexts");
    if (c->p.comm != SQ_COMM_NONE || c->slabs.size() != 1)
        return fail(SQ_E_STATE, "HMC trajectories run on one periodic slab (comm none)");
    return SQ_OK;
}

int hmc_alloc(sq_ctx *c, const Phi4StepArgs &a, size_t rows) {
    const Slab &s = c->slabs[0];
    if (c->hmc_st == nullptr) {
        SQ_HIP(hipMalloc(&c->hmc_st, sizeof(Phi4HmcState)));
        SQ_HIP(hipMemset(c->hmc_st, 0, sizeof(Phi4HmcState)));
    }
    if (c->hmc_q == nullptr)
        SQ_HIP(hipMalloc(&c->hmc_q, (size_t)(s.nz + 2 * c->gpad) * plane_floats(c) * sizeof(float)));
    const int nb = phi4_hmc_blocks(a);
    if (c->hmc_nblocks != nb) {
        (void)hipFree(c->hmc_part);
        c->hmc_part = nullptr;
        c->hmc_nblocks = 0;
        SQ_HIP(hipMalloc(&c->hmc_part, 2 * (size_t)nb * sizeof(double)));
        c->hmc_nblocks = nb;
    }
    if (rows > c->hmc_rec_cap) {
        (void)hipFree(c->hmc_rec);
        c->hmc_rec = nullptr;
        c->hmc_rec_cap = 0;
        SQ_HIP(hipMalloc(&c->hmc_rec, rows * 4 * sizeof(double)));
        c->hmc_rec_cap = rows;
    }
    return SQ_OK;
}

// One trajectory at the context's counter, enqueued on the step stream.
int hmc_trajectory(sq_ctx *c, int L, float sig, double *rec_row) {
    Slab &s = c->slabs[0];
    hipStream_t st = s.sA;
    float *F = s.buf[c->cur], *P = s.buf[c->cur ^ 1], *Q = c->hmc_q;
    const Phi4StepArgs base = phi4_periodic_args(c);
    double *part_sub = c->hmc_part, *part_add = c->hmc_part + c->hmc_nblocks;
    // phi_1 = E_s(phi_0): F -> P
    int rc = phi4_periodic_launch(c);
    if (rc) return rc;
    Phi4StepArgs t = base;  // the term passes: step size h, no noise drawn
    t.flag = &c->hmc_st->trip;
    t.in = F;
    t.out = P;
    SQ_HIP(phi4_hmc_term_launch(t, c->geom, true, part_sub, st));
    // the interior steps at 2h.  k = 1 reads phi_0 at the site from F and starts Q; from k = 2 on phi_{k+1}
    // goes in place over phi_{k-1}
    float *cur = P;
    const float *prev = F;
    if (L > 1) {
        Phi4StepArgs b = base;
        b.flag = &c->hmc_st->trip;
        b.h = base.h + base.h;
        b.sig = 0.f;
        b.sigq = 0.f;
        float *out = Q;
        for (int k = 1; k < L; ++k) {
            b.in = cur;
            b.out = out;
            SQ_HIP(phi4_hmc_leap_launch(b, c->geom, prev, st));
            float *was = cur;
            cur = out;
            prev = out = was;
        }
        c->perf.kernel_launches += L - 1;
    }
    // cur holds phi_L, prev phi_{L-1}
    t.in = cur;
    t.out = const_cast<float *>(prev);
    SQ_HIP(phi4_hmc_term_launch(t, c->geom, false, part_add, st));
    Phi4HmcVerdictArgs w{};
    w.part_sub = part_sub;
    w.part_add = part_add;
    w.nblocks = c->hmc_nblocks;
    w.L = L;
    w.sig = sig;
    w.k0 = base.k0;
    w.k1 = base.k1;
    w.s_lo = base.s_lo;
    w.s_hi = base.s_hi;
    w.st = c->hmc_st;
    w.rec = rec_row;
    SQ_HIP(phi4_hmc_verdict_launch(w, st));
    SQ_HIP(phi4_hmc_commit_launch(cur + (size_t)c->gpad * plane_floats(c), plane0(c, s, c->cur), (size_t)s.nz * plane_floats(c),
                                  c->hmc_st, st));
    c->perf.kernel_launches += 4;
    c->step += 1;
    c->perf.steps += 1;
    c->perf.site_updates += (long long)L * (long long)s.nz * (long long)plane_floats(c);
    return SQ_OK;
}

}  // namespace

namespace sq {

// sq_phi4_step_hmc in its parts, which sq_phi4_step_hmc_cluster (sq_phi4_cluster.cpp) puts a sweep between.
int phi4_hmc_check(sq_ctx *c, int ntraj, int nleap) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (ntraj < 0) return fail(SQ_E_ARG, "ntraj < 0");
    if (nleap < 1 || nleap > SQ_PHI4_ENS_MAX_LEAP) return fail(SQ_E_ARG, "nleap outside [1, SQ_PHI4_ENS_MAX_LEAP]");
    int rc = hmc_ctx_check(c);
    if (rc) return rc;
    if (hmc_sigma(c) == 0.0f) return fail(SQ_E_STATE, "HMC trajectories need noise: sigma = C sqrt(2 dtau) is 0");
    DeviceGuard g(c->dev);
    return gate_check(c, false);  // a pending sticky error: no trajectories on a corrupt field
}

int phi4_hmc_reserve(sq_ctx *c, size_t rows) { return hmc_alloc(c, phi4_periodic_args(c), rows); }

int phi4_hmc_enqueue(sq_ctx *c, int ntraj, int nleap, int randomize, size_t row0, bool rec) {
    const float sig = hmc_sigma(c);
    for (int t = 0; t < ntraj; ++t) {
        int rc = hmc_trajectory(c, hmc_length(c, nleap, randomize), sig,
                                rec ? c->hmc_rec + 4 * (row0 + (size_t)t) : nullptr);
        if (rc) return rc;
    }
    return SQ_OK;
}

int phi4_hmc_fetch(sq_ctx *c, double *rec, size_t rows) {
    SQ_HIP(hipMemcpyAsync(rec, c->hmc_rec, rows * 4 * sizeof(double), hipMemcpyDeviceToHost, c->slabs[0].sA));
    return SQ_OK;
}

void release_hmc(sq_ctx *c) {
    (void)hipFree(c->hmc_q);
    (void)hipFree(c->hmc_part);
    (void)hipFree(c->hmc_st);
    (void)hipFree(c->hmc_rec);
    c->hmc_q = nullptr;
    c->hmc_part = c->hmc_rec = nullptr;
    c->hmc_st = nullptr;
    c->hmc_nblocks = 0;
    c->hmc_rec_cap = 0;
}

}  // namespace sq

extern "C" {

int sq_phi4_step_hmc(sq_ctx *c, int ntraj, int nleap, int randomize, double *rec) {
    int rc = phi4_hmc_check(c, ntraj, nleap);
    if (rc || ntraj == 0) return rc;
    DeviceGuard g(c->dev);
    rc = phi4_hmc_reserve(c, rec ? (size_t)ntraj : 0);
    if (!rc) rc = phi4_hmc_enqueue(c, ntraj, nleap, randomize, 0, rec != nullptr);
    if (!rc && rec) rc = phi4_hmc_fetch(c, rec, (size_t)ntraj);
    if (rc) return rc;
    if (rec) SQ_HIP(hipStreamSynchronize(c->slabs[0].sA));
    return SQ_OK;
}

int sq_phi4_hmc_stats(sq_ctx *c, long long out[4]) {
    int rc = hmc_ctx_check(c);
    if (rc) return rc;
    if (!out) return fail(SQ_E_ARG, "null argument");
    memset(out, 0, 4 * sizeof(long long));
    if (c->hmc_st == nullptr) return SQ_OK;  // no trajectory yet
    DeviceGuard g(c->dev);
    hipStream_t st = c->slabs[0].sA;
    SQ_HIP(hipMemcpyAsync(out, c->hmc_st->stat, 4 * sizeof(long long), hipMemcpyDeviceToHost, st));
    SQ_HIP(hipStreamSynchronize(st));
    return SQ_OK;
}

int sq_phi4_hmc_reset(sq_ctx *c) {
    int rc = hmc_ctx_check(c);
    if (rc) return rc;
    if (c->hmc_st == nullptr) return SQ_OK;
    DeviceGuard g(c->dev);
    hipStream_t st = c->slabs[0].sA;
    // behind the trajectories in flight; the trip and accept words are cleared by their own kernels
    SQ_HIP(hipMemsetAsync(c->hmc_st, 0, sizeof(Phi4HmcState), st));
    return SQ_OK;
}

}  // extern "C"
