// sq_phi4_heun.hip -- the stochastic Heun step of the single phi^4 lattice (sq_phi4_step_heun; DESIGN.md
// §4.7): the ensemble's step (include/stochquant.h, the block above sq_phi4_ens_step_heun) for a field that
// lives in device memory instead of registers and LDS.
//
//   p    = E_s(phi)
//   e    = E_s(p), the same counter and so the same normals
//   phi' = guard(0.5f (phi + e)), one fp32 add and one fp32 multiply per site
//
// Two launches and the context's two buffers.  F holds phi, P is the idle ping-pong buffer.
//   stage 1   p = E_s(phi): the context's single Euler step, F -> P (phi4_step_kernel, launched by
//             sq_phi4_steps.cpp; not here).
//   stage 2   phi4_heun_kernel: the stencil field is P (p and its six neighbours), the other field is F (phi
//             at the lane's own quads).  The lane draws the four normals of its quad again, from the counter
//             {quad, kStreamField << 24, s lo, s hi} and the key stage 1 used, through philox_field and
//             box_muller_q as plane_compute calls them, forms e = site_update4<NZ>(p, ...) and stores phi'
//             IN PLACE over phi.
// In place is safe by the leap kernel's argument (sq_phi4_hmc.hip): F is read at the site itself only, by the
// lane that later stores there, the load ahead of the store in program order; every stencil read of the
// launch goes to P, which it does not write.  So a Heun step needs no third buffer, the context's current
// buffer is the same one before and after, and the step moves 8 + 12 bytes per site.
//
// Drawing the normals twice instead of storing them: 4 B written and 4 B read more per site and a stage 1 of
// its own against about 100 VALU instructions per float4; stage 1 stays the Euler kernel byte for byte.
//
// The march is phi4_step_kernel's (sq_phi4_march_dev.h): a wave owns an x-span of 4 QX V sites by R rows per
// lane and marches a z-chunk with planes z-1, z, z+1 of p in a register queue, x-neighbours by DPP, one
// buffer descriptor per plane with loop-invariant lane offsets; phi's float4 at the site comes by one 16-byte
// buffer load per quad, issued ahead of the next plane's loads; the normals of a plane's R V quads are drawn
// together, round-major, while those loads are in flight.  NZ = false is the C = 0 instance: no Philox, no
// Box-Muller.  Raw steps keep no guard flag (as sq_step keeps none outside frames); the clamp acts in all
// three stages.
#include "sq_phi4_heun.h"
#include "sq_phi4_march_dev.h"  // hmc_march, hmc_plane, hmc_unit; sq_phi4.hip's device functions through sq_phi4_ens_dev.h

namespace sq {

namespace {

// Stage 2 on plane z.  A.in: p; phi: the quads of A.out at the lane's sites; A.out: phi' over them.
template <int QX, int R, int V, bool MS, bool NZ>
struct HeunBody {
    const Phi4StepArgs &A;
    uint32_t qplane;  // quads per plane
    __device__ __forceinline__ void operator()(const Lane<QX, R, V> &L, const Slot<R, V> &P, const Slot<R, V> &C,
                                               const Slot<R, V> &N, const float4 (&phi)[R * V], int z, size_t plane,
                                               uint32_t pbytes) {
        const __amdgpu_buffer_rsrc_t ws = plane_rsrc(A.out, padded_index(A, z), plane, pbytes);
        // stage 1's normals of plane z: plane_compute's counters (the quad's linear index is its byte
        // offset / 16), its philox_field call and its Box-Muller pairs
        f32x4n xi[R * V];
        if constexpr (NZ) {
            u32x4 c[R * V];
            const uint32_t qbase = (uint32_t)global_z(A, z) * qplane;
#pragma unroll
            for (int k = 0; k < R * V; ++k) c[k] = u32x4{qbase + (L.voff[k] >> 4), kStreamField << 24, A.s_lo, A.s_hi};
            philox_field<R * V>(c, A.k0, A.k1);
#pragma unroll
            for (int k = 0; k < R * V; ++k) {  // scaled by 1/sqrt(2 ln 2); A.sigq carries the factor
                box_muller_q(c[k].x, c[k].y, xi[k].a, xi[k].b);
                box_muller_q(c[k].z, c[k].w, xi[k].c, xi[k].d);
            }
        } else {
#pragma unroll
            for (int k = 0; k < R * V; ++k) xi[k] = f32x4n{0.f, 0.f, 0.f, 0.f};
        }
        const float cl = A.clampv;
        auto site = [&](int k, const float4 &c, float lft, float rgt, const float4 &up, const float4 &dn,
                        const float4 &zm, const float4 &zp) {
            // fin = false: the full guard, the same bits as stage 1's fast path
            const float4 e = site_update4<NZ>(c, lft, rgt, up, dn, zm, zp, xi[k], A, false, f32x2{A.m2, A.m2});
            float4 o;
            o.x = ens_guard(__fmul_rn(0.5f, __fadd_rn(phi[k].x, e.x)), cl);
            o.y = ens_guard(__fmul_rn(0.5f, __fadd_rn(phi[k].y, e.y)), cl);
            o.z = ens_guard(__fmul_rn(0.5f, __fadd_rn(phi[k].z, e.z)), cl);
            o.w = ens_guard(__fmul_rn(0.5f, __fadd_rn(phi[k].w, e.w)), cl);
            // full-row waves: sc0 sc1 (write-through) stores, the step kernel's default there; measured against
            // plain stores 29.7 / 295 against 30.8 / 299 us per launch at 256^3 / 512^3
            if (L.rows_ok) bstore4<QX == 64 ? 17 : 0>(ws, L.voff[k], o);
        };
        hmc_plane<QX, R, V, MS>(A, L, P, C, N, z, plane, pbytes, site);
    }
};

template <int QX, int R, int V, bool MS, bool NZ>
__global__ __launch_bounds__(256) void phi4_heun_kernel(const Phi4StepArgs A) {
    const int unit = hmc_unit();
    if (unit >= A.nunits) return;
    HeunBody<QX, R, V, MS, NZ> body{A, (uint32_t)(((size_t)A.Lx * (size_t)A.Ly) >> 2)};
    hmc_march<QX, R, V, MS>(A, A.out, unit, body);
}

template <int QX, int V, bool MS, bool NZ>
const void *heun_fn_r(int r) {
    return r == 4   ? (const void *)&phi4_heun_kernel<QX, 4, V, MS, NZ>
           : r == 2 ? (const void *)&phi4_heun_kernel<QX, 2, V, MS, NZ>
                    : (const void *)&phi4_heun_kernel<QX, 1, V, MS, NZ>;
}
// phi4_step_launch's choice of the tile instance (hmc_pick's)
template <bool NZ>
const void *heun_pick(const Phi4Geom &g, bool ms) {
    switch (g.qx) {
    case 64:
        if (g.v == 2) return ms ? heun_fn_r<64, 2, true, NZ>(g.r) : heun_fn_r<64, 2, false, NZ>(g.r);
        return ms ? heun_fn_r<64, 1, true, NZ>(g.r) : heun_fn_r<64, 1, false, NZ>(g.r);
    case 32: return heun_fn_r<32, 1, false, NZ>(g.r);
    case 16: return heun_fn_r<16, 1, false, NZ>(g.r);
    case 8: return heun_fn_r<8, 1, false, NZ>(g.r);
    case 4: return heun_fn_r<4, 1, false, NZ>(g.r);
    case 2: return heun_fn_r<2, 1, false, NZ>(g.r);
    default: return nullptr;
    }
}

}  // namespace

hipError_t phi4_heun_launch(const Phi4StepArgs &a, const Phi4Geom &g, hipStream_t s) {
    const bool ms = a.nxseg > 1;
    const void *fn = a.sig != 0.0f ? heun_pick<true>(g, ms) : heun_pick<false>(g, ms);
    // the whole periodic slab in chunks of zc planes, as the march decomposes it
    if (fn == nullptr || a.in == nullptr || a.out == nullptr || a.in == a.out || !a.periodic || a.nunits <= 0 ||
        a.zlo != 0 || a.zhi != a.nz || a.zstep != a.zc || a.zc < 1 || (long long)a.zc * a.nzc < a.nz || a.gz < 1)
        return hipErrorInvalidValue;
    Phi4StepArgs q = a;
    void *args[] = {&q};
    return hipLaunchKernel(fn, dim3((unsigned)((a.nunits + 3) / 4)), dim3(256), args, 0, s);
}

}  // namespace sq
