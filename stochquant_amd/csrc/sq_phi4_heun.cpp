// sq_phi4_heun.cpp -- Heun steps of the single phi^4 lattice: sq_phi4_step_heun (include/stochquant.h; the
// kernel and the design are sq_phi4_heun.hip's; sq_phi4_step_heun_meas is with its twins in
// sq_phi4_measure.cpp).  A step is two launches on the slab's step stream; the host reads nothing back.
#include <chrono>

#include "sq_ctx.h"
#include "sq_phi4_heun.h"

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

}  // namespace sq

extern "C" {

int sq_phi4_step_heun(sq_ctx *c, int nsteps) {
    int rc = phi4_heun_check(c, nsteps);
    if (rc || nsteps == 0) return rc;
    DeviceGuard g(c->dev);
    return phi4_heun_enqueue(c, nsteps);
}

}  // extern "C"
