// sq_phi4_heun.h -- the second launch of the single lattice's Heun step (sq_phi4_heun.hip) as its host code
// (sq_phi4_heun.cpp) enqueues it.  Not installed.
#pragma once
#include "sq_internal.h"

namespace sq {

// Stage 2 of one Heun step.  a: the periodic single-slab arguments of the Euler step at the step's counter
// (phi4_fill_units over chunks of zc planes), with a.in = p = E_s(phi) (stage 1's output) and a.out = the
// buffer that holds phi and receives phi' in place.  a.sig != 0 picks the instance that draws the normals.
hipError_t phi4_heun_launch(const Phi4StepArgs &a, const Phi4Geom &g, hipStream_t s);

}  // namespace sq
