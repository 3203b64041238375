// sq_phi4_heun_fused.h -- the one-launch Heun step of the single lattice (sq_phi4_heun_fused.hip) as its host
// code (sq_phi4_heun.cpp) enqueues it.  Not installed.
#pragma once
#include "sq_internal.h"

namespace sq {

// The shapes the fused step serves: rows of 256 S sites, Ly a multiple of 8, at least two planes.
bool phi4_heun_tb_supported(int Lx, int Ly, int Lz);
// The padded buffer (nz + 2 gz planes) fits one 32-bit buffer descriptor: the WH instances.
bool phi4_heun_tb_one_descriptor(long long Lx, long long Ly, long long nz, long long gz);

// One whole Heun step at the arguments' counter, a.in -> a.out.  a: the periodic single slab in tb2's chunking
// (zlo = 0, zlen = nz >= 2, nzc = nzr chunks of zc planes, nxseg = Lx / 256, nyg = Ly / 8, nunits blocks), nw0
// the noise words of the step, no gate or frame pointers.  a.sig != 0 picks the instance that draws the normals.
hipError_t phi4_heun_tb_launch(const Phi4StepArgs &a, hipStream_t s);

}  // namespace sq
