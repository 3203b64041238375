// sq_phi4_measure.hip -- in-stream measurements of the single phi^4 lattice (sq_phi4_measure,
// sq_phi4_step_hmc_meas, sq_phi4_step_hmc_cluster_meas): the sums of phi, phi^2, phi^4 and of
// the forward nearest-neighbour products, the slice sums S(z), their momentum projections A_m(z), B_m(z) and the
// time-slice correlators g(t), g_m(t) of a field that lives in device memory.  One measurement is three
// launches on the slab's step stream; the host reads nothing between them and no launch uses an atomic.
//
//   march   phi4_meas_kernel<QX, R, V, MS, MOM>: the step kernel's register z-march (sq_phi4_march_dev.h) over
//           the field alone, the tile instances and the block -> unit map of the HMC passes.  It reads 4 bytes
//           per site plus the halo rows the march loads anyway, and writes no field.  Per plane the wave stores
//           1 + 2 M doubles to part[z][j][q], j = x-span + nxseg row-group the unit's index within its plane;
//           per unit three doubles to tot[unit][3].
//   fold    phi4_meas_fold_kernel: one lane per (z, q) adds the plane's partials, j ascending; block 0 also folds tot.
//           Loads go out in batches of 16 ahead of the additions, which stay in order.
//   corr    phi4_meas_corr_kernel: one lane per t, blocks over (momentum, t-chunk); block (0, 0) also forms
//           S1, writes the row {S1, S2, S4, NN} and counts the measurement.
//
// Summation order, complete (include/stochquant.h states the same).  Every value is a double; every product and
// every sum is rounded once (no fused multiply-add); the field's floats are converted exactly.
//   A quad is four sites x0 .. x0 + 3 of one row, values p0 .. p3, with r the site right of p3, d0 .. d3 the row
//   below and n0 .. n3 the next plane (all periodic).  A lane owns, per plane, rows y0 .. y0 + R - 1 and per row V
//   quads, v ascending (x0 = span + 4 (lane mod QX) + 4 QX v).
//   S:   row sum rs = 0.0; rs += (p0 + p1) + (p2 + p3) per quad, v ascending.  Then the QX lanes of the row by
//        the butterfly below (levels 1 .. QX / 2); t = 0.0; t += rs per row, r ascending; then t over the 64 / QX
//        row groups of the wave by the butterfly's remaining levels.  part[z][j][0] = t.
//   A, B of momentum m: per row re = 0.0, im = 0.0; per quad, v ascending,
//          re += (p0 cx[x0] + p1 cx[x0+1]) + (p2 cx[x0+2] + p3 cx[x0+3]),  im the same with sx;
//        re and im over the row's lanes (levels 1 .. QX / 2); a = 0.0, b = 0.0; per row, r ascending,
//          a += re cy[y] - im sy[y],  b += re sy[y] + im cy[y]
//        (the header's four-line recipe, the y-twiddle applied to the row's sums: the projection is separable);
//        then a and b over the row groups.  part[z][j][1 + 2 m] = a, [2 + 2 m] = b.  With (0, 0) every cx, cy is
//        1.0 and every sx, sy 0.0, so for a finite field a is t bit for bit and b is +0.0.
//   The butterfly: at level k = 1, 2, 4, 8, 16, 32 in this order every lane adds its partner's value to its own,
//        the partner being lane ^ 1, lane ^ 2, the lane mirrored within its group of 8, mirrored within its row of
//        16, lane ^ 16, lane ^ 32.  Before level k the 2 k lanes of a group hold k-lane sums; a + b = b + a in IEEE
//        arithmetic, so all of them hold the same bits afterwards: the balanced tree over the lanes in lane order.
//   S2, S4, NN: one double each per lane over its whole z-chunk, planes ascending, within a plane r, then v:
//          S2 += (p0^2 + p1^2) + (p2^2 + p3^2);  S4 += (p0^2 p0^2 + p1^2 p1^2) + (p2^2 p2^2 + p3^2 p3^2);
//          NN += (((p0 p1 + p1 p2) + (p2 p3 + p3 r)) + ((p0 d0 + p1 d1) + (p2 d2 + p3 d3)))
//                + ((p0 n0 + p1 n1) + (p2 n2 + p3 n3));
//        the wave by all six butterfly levels; tot[unit][0 .. 2].
//   Lanes whose rows lie past Ly (rows_ok false) add nothing: their values stay +0.0.
//   fold: S(z), A_m(z), B_m(z) = part[z][j][q] added j ascending from 0.0.  S2, S4, NN = tot[.][c] in 256
//        contiguous runs of ceil(nunits / 256) units, unit ascending within a run from 0.0, then the runs in order
//        from 0.0 (verdict_fold's order).
//   corr: S1 = S(z) added z ascending from 0.0.  g(t) = sum_z S(z) S((z + t) mod Lz) and g_m(t) = sum_z [A A' + B B']
//        as acc = (acc + A A') + B B', z ascending from 0.0, t = 0 .. Lz / 2.  Accumulating: G[t] = G[t] + g(t),
//        Gp[m][t] = Gp[m][t] + g_m(t), S1acc = S1acc + S1, one addition each.
// Nothing above depends on the call, on how calls are split or on where the measurement was enqueued: the bits
// of every result depend on the lattice's shape and the field alone.
#include "sq_phi4_measure.h"
#include "sq_phi4_march_dev.h"

namespace sq {

namespace {

// butterfly levels LO <= k < HI (powers of two) of the order stated above
template <int LO, int HI>
__device__ __forceinline__ double meas_xor_sum(double v) {
    if constexpr (LO <= 1 && HI > 1) v += dpp_d<0xB1, 0xf, 0xf>(v, 0.0);   // quad_perm [1, 0, 3, 2]
    if constexpr (LO <= 2 && HI > 2) v += dpp_d<0x4E, 0xf, 0xf>(v, 0.0);   // quad_perm [2, 3, 0, 1]
    if constexpr (LO <= 4 && HI > 4) v += dpp_d<0x141, 0xf, 0xf>(v, 0.0);  // row_half_mirror
    if constexpr (LO <= 8 && HI > 8) v += dpp_d<0x140, 0xf, 0xf>(v, 0.0);  // row_mirror
    if constexpr (LO <= 16 && HI > 16) v += __shfl_xor(v, 16, 64);
    if constexpr (LO <= 32 && HI > 32) v += __shfl_xor(v, 32, 64);
    return v;
}

template <int QX, int R, int V, bool MS, bool MOM>
struct MeasBody {
    const Phi4StepArgs &A;
    const Phi4MeasArgs &W;
    int j, nj, nq;  // the unit within its plane, units per plane, doubles per (plane, unit)
    int x0, y0;     // the lane's first site of segment 0 and its first row (0 where rows_ok is false)
    double s2, s4, nn;
    __device__ __forceinline__ void operator()(const Lane<QX, R, V> &L, const Slot<R, V> &P, const Slot<R, V> &C,
                                               const Slot<R, V> &N, const float4 (&)[R * V], int z, size_t plane,
                                               uint32_t pbytes) {
        double rs[R];
#pragma unroll
        for (int r = 0; r < R; ++r) rs[r] = 0.0;
        auto site = [&](int k, const float4 &c, float, float rgt, const float4 &, const float4 &dn, const float4 &,
                        const float4 &zp) {
            if (!L.rows_ok) return;
            const double x = c.x, y = c.y, zz = c.z, w = c.w, r = rgt;
            const double x2 = x * x, y2 = y * y, z2 = zz * zz, w2 = w * w;
            rs[k / V] += (x + y) + (zz + w);
            s2 += (x2 + y2) + (z2 + w2);
            s4 += (x2 * x2 + y2 * y2) + (z2 * z2 + w2 * w2);
            nn += (((x * y + y * zz) + (zz * w + w * r)) +
                   ((x * (double)dn.x + y * (double)dn.y) + (zz * (double)dn.z + w * (double)dn.w))) +
                  ((x * (double)zp.x + y * (double)zp.y) + (zz * (double)zp.z + w * (double)zp.w));
        };
        hmc_plane<QX, R, V, MS>(A, L, P, C, N, z, plane, pbytes, site);
        double t = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) t += meas_xor_sum<1, QX>(rs[r]);
        t = meas_xor_sum<QX, 64>(t);
        double *out = W.part + ((size_t)z * (size_t)nj + (size_t)j) * (size_t)nq;
        if (L.lane == 0) out[0] = t;
        if constexpr (MOM) {
#pragma unroll 1
            for (int m = 0; m < W.M; ++m) {
                const double *cx = W.cx + (size_t)m * A.Lx + x0, *sx = W.sx + (size_t)m * A.Lx + x0;
                const double *cy = W.cy + (size_t)m * A.Ly + y0, *sy = W.sy + (size_t)m * A.Ly + y0;
                double2 tc[V][2], ts[V][2];
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    const double2 *c2 = reinterpret_cast<const double2 *>(cx + 4 * QX * v);
                    const double2 *s2p = reinterpret_cast<const double2 *>(sx + 4 * QX * v);
                    tc[v][0] = c2[0];
                    tc[v][1] = c2[1];
                    ts[v][0] = s2p[0];
                    ts[v][1] = s2p[1];
                }
                double a = 0.0, b = 0.0;
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    double re = 0.0, im = 0.0;
                    if (L.rows_ok) {
#pragma unroll
                        for (int v = 0; v < V; ++v) {
                            const float4 c = C.row[r * V + v];
                            const double p0 = c.x, p1 = c.y, p2 = c.z, p3 = c.w;
                            re += (p0 * tc[v][0].x + p1 * tc[v][0].y) + (p2 * tc[v][1].x + p3 * tc[v][1].y);
                            im += (p0 * ts[v][0].x + p1 * ts[v][0].y) + (p2 * ts[v][1].x + p3 * ts[v][1].y);
                        }
                    }
                    re = meas_xor_sum<1, QX>(re);
                    im = meas_xor_sum<1, QX>(im);
                    const double yc = cy[r], ys = sy[r];
                    a += re * yc - im * ys;
                    b += re * ys + im * yc;
                }
                a = meas_xor_sum<QX, 64>(a);
                b = meas_xor_sum<QX, 64>(b);
                if (L.lane == 0) {
                    out[1 + 2 * m] = a;
                    out[2 + 2 * m] = b;
                }
            }
        }
    }
};

template <int QX, int R, int V, bool MS, bool MOM>
__global__ __launch_bounds__(256) void phi4_meas_kernel(const Phi4StepArgs A, const Phi4MeasArgs W) {
    const int unit = hmc_unit();
    if (unit >= A.nunits) return;  // wave-uniform
    constexpr int RS = 64 / QX;
    const int lane = threadIdx.x & 63;
    const int xs = unit % A.nxseg, yg = (unit / A.nxseg) % A.nyg;
    const int y0r = yg * (RS * R) + (lane / QX) * R;
    MeasBody<QX, R, V, MS, MOM> body{A,
                                     W,
                                     xs + A.nxseg * yg,
                                     A.nxseg * A.nyg,
                                     MOM ? 1 + 2 * W.M : 1,
                                     xs * (4 * QX * V) + 4 * (lane & (QX - 1)),
                                     y0r < A.Ly ? y0r : 0,
                                     0.0,
                                     0.0,
                                     0.0};
    hmc_march<QX, R, V, MS, false>(A, nullptr, unit, body);
    const double s2 = meas_xor_sum<1, 64>(body.s2), s4 = meas_xor_sum<1, 64>(body.s4),
                 nn = meas_xor_sum<1, 64>(body.nn);
    if (lane == 0) {
        double *o = W.tot + 3 * (size_t)unit;
        o[0] = s2;
        o[1] = s4;
        o[2] = nn;
    }
}

constexpr int kFoldLanes = 64;   // one wave per block: the (z, q) outputs spread over the compute units
constexpr int kFoldRuns = 256;   // verdict_fold's runs of the units' totals
constexpr int kBatch = 16;

// a + p[0] + p[stride] + ... + p[(n - 1) stride], in this order.  The loads of kBatch terms go out together and
// the additions stay in order: one lane's dependent chain would otherwise pay a memory latency per term.
__device__ __forceinline__ double meas_ordered_sum(const double *p, size_t stride, int n, double a) {
    double v[kBatch];
    int i = 0;
    for (; i + kBatch <= n; i += kBatch) {
#pragma unroll
        for (int k = 0; k < kBatch; ++k) v[k] = p[(size_t)(i + k) * stride];
#pragma unroll
        for (int k = 0; k < kBatch; ++k) a = __dadd_rn(a, v[k]);
    }
    for (; i < n; ++i) a = __dadd_rn(a, p[(size_t)i * stride]);
    return a;
}

__global__ __launch_bounds__(kFoldLanes) void phi4_meas_fold_kernel(const Phi4MeasFoldArgs F) {
    __shared__ double lds[3][kFoldRuns];
    const long long idx = (long long)blockIdx.x * kFoldLanes + threadIdx.x;
    if (idx < (long long)F.nz * F.nq) {
        const int z = (int)(idx / F.nq), q = (int)(idx % F.nq);
        const double *p = F.part + (size_t)z * (size_t)F.nj * (size_t)F.nq + (size_t)q;
        F.sl[(size_t)q * (size_t)F.nz + (size_t)z] = meas_ordered_sum(p, (size_t)F.nq, F.nj, 0.0);
    }
    if (blockIdx.x != 0) return;
    const int run = (F.nunits + kFoldRuns - 1) / kFoldRuns;
    for (int r = threadIdx.x; r < kFoldRuns; r += kFoldLanes) {
        const int lo = min(r * run, F.nunits), n = min((r + 1) * run, F.nunits) - lo;
#pragma unroll
        for (int c = 0; c < 3; ++c) lds[c][r] = meas_ordered_sum(F.tot + 3 * (size_t)lo + c, 3, n, 0.0);
    }
    __syncthreads();
    if (threadIdx.x < 3) F.sums[threadIdx.x] = meas_ordered_sum(lds[threadIdx.x], 1, kFoldRuns, 0.0);
}

constexpr int kCorrLanes = 256;

// sum_z [A(z) A(zt) + B(z) B(zt)] (AB false: the A term alone), zt = (z + t) mod nz, z ascending from 0.0, the
// reads of kBatch planes issued together.  at(z) = {A(z), B(z)}: the caller's accessor knows where the slices lie
// (LDS or device memory), so no read goes through a generic pointer.
template <bool AB, class At>
__device__ __forceinline__ double meas_corr_sum(At at, int nz, int t) {
    double acc = 0.0;
    int z = 0;
    for (; z + kBatch <= nz; z += kBatch) {
        double2 p[kBatch], q[kBatch];
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            int zt = z + k + t;  // t < nz, so one wrap
            zt = zt >= nz ? zt - nz : zt;
            p[k] = at(z + k);
            q[k] = at(zt);
        }
#pragma unroll
        for (int k = 0; k < kBatch; ++k) {
            acc = __dadd_rn(acc, __dmul_rn(p[k].x, q[k].x));
            if constexpr (AB) acc = __dadd_rn(acc, __dmul_rn(p[k].y, q[k].y));
        }
    }
    for (; z < nz; ++z) {
        int zt = z + t;
        zt = zt >= nz ? zt - nz : zt;
        const double2 p = at(z), q = at(zt);
        acc = __dadd_rn(acc, __dmul_rn(p.x, q.x));
        if constexpr (AB) acc = __dadd_rn(acc, __dmul_rn(p.y, q.y));
    }
    return acc;
}

// blockIdx.y = 0: g from S; 1 + m: g_m from A_m, B_m.  In LDS a block keeps S as doubles, and A_m, B_m
// interleaved as one 16-byte pair per plane (16 nz bytes; every pair is aligned whatever nz is).
__global__ __launch_bounds__(kCorrLanes) void phi4_meas_corr_kernel(const Phi4MeasCorrArgs K) {
    extern __shared__ __attribute__((aligned(16))) double corr_lds[];
    const int mi = blockIdx.y, nz = K.nz, tid = threadIdx.x;
    const bool first = mi == 0 && blockIdx.x == 0;
    const bool accum = mi == 0 ? (K.acc & 1) != 0 : (K.acc & 2) != 0;
    const bool form = K.gout != nullptr || accum;
    if (!form && !first) return;  // block-uniform
    const double *A = mi == 0 ? K.sl : K.sl + (size_t)(2 * mi - 1) * (size_t)nz;
    const double *B = A + nz;  // mi > 0 only
    const double2 *pair = reinterpret_cast<const double2 *>(corr_lds);
    if (K.lds && form) {
        for (int z = tid; z < nz; z += kCorrLanes) {
            if (mi == 0) {
                corr_lds[z] = A[z];
            } else {
                corr_lds[2 * z] = A[z];
                corr_lds[2 * z + 1] = B[z];
            }
        }
        __syncthreads();
    }
    const int t = blockIdx.x * kCorrLanes + tid;
    if (form && t < K.nt) {
        double acc;
        if (mi == 0 && K.lds) acc = meas_corr_sum<false>([&](int z) { return make_double2(corr_lds[z], 0.0); }, nz, t);
        else if (mi == 0) acc = meas_corr_sum<false>([&](int z) { return make_double2(A[z], 0.0); }, nz, t);
        else if (K.lds) acc = meas_corr_sum<true>([&](int z) { return pair[z]; }, nz, t);
        else acc = meas_corr_sum<true>([&](int z) { return make_double2(A[z], B[z]); }, nz, t);
        if (K.gout != nullptr) K.gout[(size_t)mi * (size_t)K.nt + t] = acc;
        if (accum) {
            double *G = mi == 0 ? K.G : K.Gp + (size_t)(mi - 1) * (size_t)K.nt;
            G[t] = __dadd_rn(G[t], acc);
        }
    }
    if (first && tid == kCorrLanes - 1) {  // the block's last lane: the first ones carry a t
        const double s1 = meas_ordered_sum(K.sl, 1, nz, 0.0);  // S from device memory
        K.row[0] = s1;
        K.row[1] = K.sums[0];
        K.row[2] = K.sums[1];
        K.row[3] = K.sums[2];
        if (K.acc & 1) {
            *K.S1acc = __dadd_rn(*K.S1acc, s1);
            K.nmeas[0] += 1;
        }
        if (K.acc & 2) K.nmeas[1] += 1;
    }
}

__global__ __launch_bounds__(256) void phi4_meas_clear_kernel(double *p, size_t n) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) p[i] = 0.0;
}

template <int QX, int R, int V, bool MS>
const void *meas_fn(bool mom) {
    return mom ? (const void *)&phi4_meas_kernel<QX, R, V, MS, true> : (const void *)&phi4_meas_kernel<QX, R, V, MS, false>;
}
template <int QX, int V, bool MS>
const void *meas_fn_r(int r, bool mom) {
    return r == 4 ? meas_fn<QX, 4, V, MS>(mom) : r == 2 ? meas_fn<QX, 2, V, MS>(mom) : meas_fn<QX, 1, V, MS>(mom);
}
// hmc_pick's choice of the tile instance, which is phi4_step_launch's
const void *meas_pick(const Phi4Geom &g, bool ms, bool mom) {
    switch (g.qx) {
    case 64:
        if (g.v == 2) return ms ? meas_fn_r<64, 2, true>(g.r, mom) : meas_fn_r<64, 2, false>(g.r, mom);
        return ms ? meas_fn_r<64, 1, true>(g.r, mom) : meas_fn_r<64, 1, false>(g.r, mom);
    case 32: return meas_fn_r<32, 1, false>(g.r, mom);
    case 16: return meas_fn_r<16, 1, false>(g.r, mom);
    case 8: return meas_fn_r<8, 1, false>(g.r, mom);
    case 4: return meas_fn_r<4, 1, false>(g.r, mom);
    case 2: return meas_fn_r<2, 1, false>(g.r, mom);
    default: return nullptr;
    }
}

}  // namespace

hipError_t phi4_meas_launch(const Phi4StepArgs &a, const Phi4Geom &g, const Phi4MeasArgs &w, hipStream_t s) {
    const void *fn = meas_pick(g, a.nxseg > 1, w.M > 0);
    const bool ok = a.in != nullptr && a.periodic && a.nunits > 0 && a.zlo == 0 && a.zhi == a.nz && a.zstep == a.zc &&
                    a.zc >= 1 && (long long)a.zc * a.nzc >= a.nz && a.gz >= 1 && w.part != nullptr && w.tot != nullptr &&
                    w.M >= 0 && w.M <= kPhi4MeasMaxMomenta &&
                    (w.M == 0 || (w.cx != nullptr && w.sx != nullptr && w.cy != nullptr && w.sy != nullptr));
    if (!ok || fn == nullptr) return hipErrorInvalidValue;
    Phi4StepArgs q = a;
    Phi4MeasArgs v = w;
    void *args[] = {&q, &v};
    return hipLaunchKernel(fn, dim3((unsigned)((a.nunits + 3) / 4)), dim3(256), args, 0, s);
}

hipError_t phi4_meas_fold_launch(const Phi4MeasFoldArgs &f, hipStream_t s) {
    if (f.part == nullptr || f.tot == nullptr || f.sl == nullptr || f.sums == nullptr || f.nz < 1 || f.nj < 1 ||
        f.nq < 1 || f.nunits < 1)
        return hipErrorInvalidValue;
    const long long n = (long long)f.nz * f.nq;
    hipLaunchKernelGGL(phi4_meas_fold_kernel, dim3((unsigned)((n + kFoldLanes - 1) / kFoldLanes)), dim3(kFoldLanes), 0, s,
                       f);
    return hipGetLastError();
}

int phi4_meas_corr_lds(long long nz, int M) {
    const long long need = (M > 0 ? 16 : 8) * nz;
    return need <= kPhi4MeasCorrLds ? (int)need : 0;
}

hipError_t phi4_meas_corr_launch(const Phi4MeasCorrArgs &k, hipStream_t s) {
    if (k.sl == nullptr || k.sums == nullptr || k.row == nullptr || k.nz < 1 || k.nt != k.nz / 2 + 1 || k.M < 0 ||
        k.M > kPhi4MeasMaxMomenta || (k.acc & ~3) != 0 || k.lds != phi4_meas_corr_lds(k.nz, k.M) ||
        (k.acc != 0 && (k.G == nullptr || k.Gp == nullptr || k.S1acc == nullptr || k.nmeas == nullptr)))
        return hipErrorInvalidValue;
    const dim3 grid((unsigned)((k.nt + kCorrLanes - 1) / kCorrLanes), (unsigned)(1 + k.M));
    hipLaunchKernelGGL(phi4_meas_corr_kernel, grid, dim3(kCorrLanes), (size_t)k.lds, s, k);
    return hipGetLastError();
}

hipError_t phi4_meas_clear_launch(double *p, size_t n, hipStream_t s) {
    if (p == nullptr) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((n + 255) / 256, 1024));
    hipLaunchKernelGGL(phi4_meas_clear_kernel, dim3(grid), dim3(256), 0, s, p, n);
    return hipGetLastError();
}

}  // namespace sq
