// sq_phi4_heun.cpp -- Heun steps of the single phi^4 lattice: sq_phi4_step_heun (include/stochquant.h; the
// kernel and the design are sq_phi4_heun.hip's; sq_phi4_step_heun_meas is with its twins in
// sq_phi4_measure.cpp).  A step is two launches on the slab's step stream; the host reads nothing back.
// sq_phi4_step_heun_fused: the same step as one launch on rows of 256 S sites (sq_phi4_heun_fused.hip), and
// sq_phi4_heun_fused_shape_info.
#include <algorithm>
#include <chrono>

#include "sq_ctx.h"
#include "sq_phi4_heun.h"
#include "sq_phi4_heun_fused.h"

using namespace sq;

namespace sq {

// sq_phi4_step_heun in its parts, which sq_phi4_step_heun_meas puts measurements between.
int phi4_heun_check(sq_ctx *c, int nsteps) {
    if (!c) return fail(SQ_E_ARG, "null context");
    if (nsteps < 0) return fail(SQ_E_ARG, "nsteps < 0");
    if (!is_phi4(c)) return fail(SQ_E_STATE, "Heun steps are for PHI4 contexts");
    if (c->p.comm != SQ_COMM_NONE || c->slabs.size() != 1)
        return fail(SQ_E_STATE, "Heun steps run on one periodic slab (comm none)");
    DeviceGuard g(c->dev);
    return gate_check(c, false);  // a pending sticky error: no steps on a corrupt field
}

int phi4_heun_enqueue(sq_ctx *c, int nsteps) {
    Slab &s = c->slabs[0];
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < nsteps; ++i) {
        // p = E_s(phi): F -> P, the plain one-step launch; cur stays
        int rc = phi4_periodic_launch(c);
        if (rc) return rc;
        // e = E_s(p) and phi' = guard(0.5f (phi + e)) over phi in F
        Phi4StepArgs a = phi4_periodic_args(c);
        a.in = s.buf[c->cur ^ 1];
        a.out = s.buf[c->cur];
        SQ_HIP(phi4_heun_launch(a, c->geom, s.sA));
        c->perf.kernel_launches += 1;
        c->step += 1;
        c->perf.steps += 1;
        c->perf.site_updates += (long long)s.nz * (long long)plane_floats(c);
        c->field_finite = true;  // every site of F has been through the guard
    }
    c->perf.frame_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SQ_OK;
}

// sq_phi4_step_heun_fused in the same parts.  The refusals name their cause and launch nothing.
int phi4_heun_fused_check(sq_ctx *c, int nsteps) {
    int rc = phi4_heun_check(c, nsteps);
    if (rc) return rc;
    if (!phi4_heun_tb_supported(c->Lx, c->Ly, c->slabs[0].nz))
        return fail(SQ_E_STATE, "fused Heun steps need Lx % 256 == 0, Ly % 8 == 0 and Lz >= 2");
    if (c->tbz <= 0) return fail(SQ_E_STATE, "fused Heun steps need the two-step path (the context was created with SQ_FUSE2=0)");
    return SQ_OK;
}

int phi4_heun_fused_enqueue(sq_ctx *c, int nsteps) {
    Slab &s = c->slabs[0];
    const auto t0 = std::chrono::steady_clock::now();
    for (int i = 0; i < nsteps; ++i) {
        // the whole step, F -> P, in the two-step launches' chunking of the periodic slab: planes per block
        // pinned (SQ_FUSE2_Z), or as many as make one round of tb_blocks blocks, not fewer than tb_minz
        Phi4StepArgs a = phi4_periodic_args(c);  // the counter, nw0 and fin of this step
        const int len = s.nz;
        a.nyg = c->Ly / 8;
        a.nxseg = c->Lx / 256;
        const int nzc_t = std::max(1, c->tb_blocks / (a.nyg * a.nxseg));
        const int zb = c->tbz_pin ? c->tbz : std::min(len, std::max(c->tb_minz, (len + nzc_t - 1) / nzc_t));
        a.zlo = 0;
        a.zhi = len;
        a.zstep = 0;
        a.zc = zb;
        a.zlen = len;
        a.nzr = (len + zb - 1) / zb;
        a.nzc = a.nzr;
        a.nunits = a.nxseg * a.nyg * a.nzc;
        SQ_HIP(phi4_heun_tb_launch(a, s.sA));
        c->cur ^= 1;
        c->perf.kernel_launches += 1;
        c->step += 1;
        c->perf.steps += 1;
        c->perf.site_updates += (long long)s.nz * (long long)plane_floats(c);
        c->field_finite = true;  // every site of the new F has been through the guard
    }
    c->perf.frame_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return SQ_OK;
}

}  // namespace sq

extern "C" {

int sq_phi4_step_heun_fused(sq_ctx *c, int nsteps) {
    int rc = phi4_heun_fused_check(c, nsteps);
    if (rc || nsteps == 0) return rc;
    DeviceGuard g(c->dev);
    return phi4_heun_fused_enqueue(c, nsteps);
}

int sq_phi4_heun_fused_shape_info(const int *dims, int *info) {
    if (!dims || !info) return fail(SQ_E_ARG, "null argument");
    if (dims[0] <= 0 || dims[1] <= 0 || dims[2] <= 0) return fail(SQ_E_ARG, "dims must be positive");
    const bool ok = phi4_heun_tb_supported(dims[0], dims[1], dims[2]);
    info[0] = ok ? 1 : 0;
    info[1] = ok && dims[0] > 256 ? 1 : 0;
    // a comm-none context pads its buffers by one plane on either side
    info[2] = ok && phi4_heun_tb_one_descriptor(dims[0], dims[1], dims[2], 1) ? 1 : 0;
    return SQ_OK;
}

int sq_phi4_step_heun(sq_ctx *c, int nsteps) {
    int rc = phi4_heun_check(c, nsteps);
    if (rc || nsteps == 0) return rc;
    DeviceGuard g(c->dev);
    return phi4_heun_enqueue(c, nsteps);
}

}  // extern "C"
