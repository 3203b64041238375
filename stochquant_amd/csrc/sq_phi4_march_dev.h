// sq_phi4_march_dev.h -- the register z-march of the single phi^4 lattice's passes that read a field with its
// stencil and write none through the step kernel's own path: the HMC leap and term kernels (sq_phi4_hmc.hip) and
// the measurement kernel (sq_phi4_measure.hip).  Device code only.
//
// The march is phi4_step_kernel's: a wave owns an x-span of 4 QX V sites by R rows per lane and marches a
// z-chunk with planes z-1, z, z+1 of the stencil field in a register queue (Slot, load_slot), x-neighbours by
// DPP, segment edges and y-halo rows loaded as that kernel loads them, one buffer descriptor per plane with
// loop-invariant lane offsets.
#pragma once
#include "sq_phi4_ens_dev.h"  // sq_phi4.hip's device functions

namespace sq {

namespace {

// One wave's unit of a pass: unit_run's decomposition and lane offsets, the
// three-slot queue over A.in, and per plane z the quads `oth` of site_field at
// the lane's own sites (OTH; without it site_field is not read and oth holds
// nothing).  body(L, P, C, N, oth, z) sees planes z-1, z, z+1.
template <int QX, int R, int V, bool MS, bool OTH = true, class Body>
__device__ __forceinline__ void hmc_march(const Phi4StepArgs &A, const float *site_field, int unit, Body &body) {
    constexpr int RS = 64 / QX;
    const int xs = unit % A.nxseg;
    const int rest = unit / A.nxseg;
    const int yg = rest % A.nyg;
    const int zk = rest / A.nyg;
    const int zbeg = A.zlo + zk * A.zstep;
    const int zend = min(zbeg + A.zc, A.zhi);
    const int Lx = A.Lx, Ly = A.Ly;
    const size_t plane = (size_t)Lx * (size_t)Ly;
    const uint32_t pbytes = (uint32_t)(plane * sizeof(float));
    Lane<QX, R, V> L;
    L.lane = threadIdx.x & 63;
    const int xq = L.lane & (QX - 1);
    const int rsid = L.lane / QX;
    const int xspan = xs * (4 * QX * V);
    const int x = xspan + 4 * xq;
    const int y0r = yg * (RS * R) + rsid * R;
    L.rows_ok = y0r < Ly;  // lanes past Ly read row 0 and neither store nor sum
    const int y0 = L.rows_ok ? y0r : 0;
    const int ym = y0 == 0 ? Ly - 1 : y0 - 1;
    const int yp = (y0 + R == Ly) ? 0 : y0 + R;
    const int xl = (xspan == 0 ? Lx : xspan) - 1;
    const int xr = (xspan + 4 * QX * V == Lx) ? 0 : xspan + 4 * QX * V;
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int v = 0; v < V; ++v) {
            L.voff[r * V + v] = (uint32_t)(((y0 + r) * Lx + x + 4 * QX * v) * 4);
            L.qoff[r * V + v] = 0;
        }
        L.vl[r] = (uint32_t)(((y0 + r) * Lx + xl) * 4);
        L.vr[r] = (uint32_t)(((y0 + r) * Lx + xr) * 4);
    }
#pragma unroll
    for (int v = 0; v < V; ++v) {
        L.vm[v] = (uint32_t)((ym * Lx + x + 4 * QX * v) * 4);
        L.vp[v] = (uint32_t)((yp * Lx + x + 4 * QX * v) * 4);
    }
    Slot<R, V> S0, S1, S2;
    float4 oth[R * V];
    auto other = [&](int z) {
        if constexpr (OTH) {
            const __amdgpu_buffer_rsrc_t rs = plane_rsrc(site_field, padded_index(A, z), plane, pbytes);
#pragma unroll
            for (int k = 0; k < R * V; ++k) oth[k] = bload4(rs, L.voff[k]);
        }
    };
    load_slot<QX, R, V>(A, L, S0, zbeg - 1, false, plane, pbytes);
    load_slot<QX, R, V>(A, L, S1, zbeg, true, plane, pbytes);
    for (int z = zbeg; z < zend; z += 3) {
        other(z);
        load_slot<QX, R, V>(A, L, S2, z + 1, z + 1 < zend, plane, pbytes);
        body(L, S0, S1, S2, oth, z, plane, pbytes);
        if (z + 1 >= zend) break;
        other(z + 1);
        load_slot<QX, R, V>(A, L, S0, z + 2, z + 2 < zend, plane, pbytes);
        body(L, S1, S2, S0, oth, z + 1, plane, pbytes);
        if (z + 2 >= zend) break;
        other(z + 2);
        load_slot<QX, R, V>(A, L, S1, z + 3, z + 3 < zend, plane, pbytes);
        body(L, S2, S0, S1, oth, z + 2, plane, pbytes);
    }
}

// The stencil of plane z for every quad of the lane, as plane_compute forms it:
// site(k, c, lft, rgt, up, dn, zm, zp) per quad k = r V + v.
template <int QX, int R, int V, bool MS, class Site>
__device__ __forceinline__ void hmc_plane(const Phi4StepArgs &A, const Lane<QX, R, V> &L, const Slot<R, V> &P,
                                          const Slot<R, V> &C, const Slot<R, V> &N, int z, size_t plane,
                                          uint32_t pbytes, Site &site) {
    float el[R], er[R];
    if constexpr (MS) {
        const __amdgpu_buffer_rsrc_t rs = plane_rsrc(A.in, padded_index(A, z), plane, pbytes);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            el[r] = 0.f;
            er[r] = 0.f;
            if (L.lane == 0) el[r] = bload1(rs, L.vl[r]);
            if (L.lane == 63) er[r] = bload1(rs, L.vr[r]);
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        float rl[V], rr[V];
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const float4 cc = C.row[r * V + v];
            if constexpr (QX == 64) {
                rl[v] = from_left_lane(cc.w);
                rr[v] = from_right_lane(cc.x);
            } else {
                const int seg = L.lane & ~(QX - 1), xq = L.lane & (QX - 1);
                rl[v] = __shfl(cc.w, seg | ((xq + QX - 1) & (QX - 1)), 64);
                rr[v] = __shfl(cc.x, seg | ((xq + 1) & (QX - 1)), 64);
            }
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int k = r * V + v;
            const float4 up = r > 0 ? C.row[r > 0 ? k - V : 0] : C.hm[v];
            const float4 dn = r < R - 1 ? C.row[r < R - 1 ? k + V : 0] : C.hp[v];
            float lft = rl[v], rgt = rr[v];
            if constexpr (V > 1) {
                if (L.lane == 0) lft = rl[(v + V - 1) % V];
                if (L.lane == 63) rgt = rr[(v + 1) % V];
            }
            if constexpr (MS) {
                if (v == 0 && L.lane == 0) lft = el[r];
                if (v == V - 1 && L.lane == 63) rgt = er[r];
            }
            site(k, C.row[k], lft, rgt, up, dn, P.row[k], N.row[k]);
        }
    }
}

// the step kernel's block -> unit map: consecutive logical blocks on one XCD
__device__ __forceinline__ int hmc_unit() {
    const int nb = gridDim.x, b = blockIdx.x;
    const int lb = (nb & 7) == 0 ? (b & 7) * (nb >> 3) + (b >> 3) : b;
    return __builtin_amdgcn_readfirstlane(lb * 4 + (int)(threadIdx.x >> 6));
}

}  // namespace

}  // namespace sq
