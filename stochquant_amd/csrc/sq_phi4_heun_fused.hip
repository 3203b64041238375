// sq_phi4_heun_fused.hip -- one whole Heun step of the single phi^4 lattice in ONE launch, for rows of
// 256 S sites (sq_phi4_step_heun_fused).  The two-launch step (sq_phi4_heun.hip) moves
// 8 + 12 bytes per site; this one reads the field once and writes it once, 8 bytes per site, and evaluates
// Philox / Box-Muller once per site instead of twice.
//
//   p    = E_s(phi)
//   e    = E_s(p), the same counter and so the same normals
//   phi' = guard(0.5f (phi + e)), one fp32 add and one fp32 multiply per site
//
// The layout is phi4_tb2_kernel's temporal blocking (sq_phi4.hip): a block owns one 256-site x-segment of
// kTbRows = 8 output rows [y0, y0+8) of a z-chunk [z0, z1); row wave w = 0..9 holds row y0-1+w (lane l: sites
// x0+4l .. x0+4l+3); S > 1 adds the x-halo wave w = 10 (the 16 sites x0-1 | x0+256 of the 8 output rows).
// Marching p over [z0-1, z1]:
//   1. every row wave loads input plane p+1 (its row and both y-halo rows) and forms its row of
//      p-stage plane p, T(p) = site_update4(I(p).row, ..., xa), xa the quad's normals at counter s, and
//      publishes it in LDS slot (p - (z0-1)) % 3; the x-halo wave does the same for its sites (tx).  An output
//      row wave keeps xa in a two-deep queue X beside T;
//   2. one block barrier;
//   3. output row waves, p > z0: e = site_update4(T(p-1), x-neighbours by DPP / tx, y-neighbours from LDS,
//      T(p-2), T(p), X(p-1)) and phi' = guard(0.5f (phi + e)) with phi = I(p-1).row, stored to plane p-1 of the
//      other buffer with sc0 sc1 (write-through) stores, as tb2 stores.
//
// Why this is all the march holds.  Stage 1 of plane p reads input planes p-1, p, p+1: three live input planes
// (of plane p-1 only the row itself survives stage 1, and that row is exactly the phi the average of plane
// p-1 needs in the same iteration, so no input is loaded twice and none is kept for the average alone).
// Stage 2 of plane p-1 reads stage-1 planes p-2, p-1, p: three stage-1 planes.  Both stages of a site use the
// counter {quad, kStreamField << 24, s lo, s hi}, so stage 2 of plane p-1 wants the normals stage 1 drew one
// iteration earlier at the same lane's sites: one kept quad of four floats (X(p-1)), beside the one just drawn.
// The Euler pair of tb2 keys its second step with s+1 and can keep only the step-independent prefix of the
// Philox rounds (NoisePre); here nothing of the noise is evaluated twice.
//
// Same bits as the two launches.  Stage 1 is tb2's first step: site_update4 with fin = A.fin on the same
// operands in the same order, the normals through noise_prefix / tb_noise, which are philox_field's bit for bit
// (tests/test_gpu_phi4.py holds tb2 to two single steps).  Stage 2 passes fin = true where phi4_heun_kernel
// passes false: its inputs are stage 1's guarded outputs, finite and inside the clamp whatever phi was (NaN and
// infinities included), so by site_update4's argument the update is finite or an infinity, never NaN, and the
// guard's fast path gives the full guard's bits (tb2's second step rests on the same argument).  phi itself may
// be anything after an upload: it enters only the average, whose guard is the full one (heun_guard).
//
// Chunk edges.  Stage-1 planes z0-1 and z1 and the halo rows y0-1, y0+8 (and the x-halo sites) are recomputed
// by the blocks that own them too; the counter-based noise makes the copies identical.  Per chunk that is two
// stage-1 planes more, per block two rows more; stage 2 is computed once per site.
//
// Registers.  The narrow tb2 instance has 72 VGPRs with its carried prefix queue (2 x 3 live words); X is
// 2 x 4 floats and the second Philox evaluation is gone, so the aim is the same budget: at most 80 VGPRs
// without scratch for the narrow instances (two 10-wave blocks per CU; WPE = 1 leaves the allocator free) and,
// for the wide ones, WPE = 6 (<= 80 VGPRs, two 11-wave blocks per CU) against WPE = 1.  Built: narrow 76 / 74
// VGPRs (one descriptor / per-plane descriptors), 62 without noise, no scratch; wide WPE = 1 88 VGPRs, no
// scratch, WPE = 6 80 VGPRs and 36 / 24 bytes of scratch per lane (the faster, WPE = 1, is the default).
// No frame records, gate, staging, neighbour sync or pipelined form.
#define SQ_PHI4_KERNELS_ONLY
#include "sq_phi4.hip"
#include "sq_phi4_heun_fused.h"

namespace sq {

namespace {

// ens_guard's expression (sq_phi4_ens_dev.h), the full guard: NaN and > cl to +cl, < -cl to -cl
__device__ __forceinline__ float heun_guard(float v, float cl) { return fmaxf(fminf(v, cl), -cl); }

// One plane of the march, in tb_plane's names.  Row waves: I0 (p-1), I1 (p), I2 (p+1, loaded here); T0 (p-2),
// T1 (p-1), T2 (p, computed here); X1 the normals of plane p-1's quad, X2 those of plane p's (drawn here).
// The x-halo wave keeps the centres of its sites in row.x.  J = (p - (z0 - 1)) % 3: plane p's LDS slot.
template <bool NZ, bool WIDE, bool WH, int J>
__device__ __forceinline__ void heun_tb_plane(const Phi4StepArgs &A, const TbCtx &K, TbRun &R, int p, const TbIn &I0,
                                              const TbIn &I1, TbIn &I2, const float4 &T0, const float4 &T1, float4 &T2,
                                              const f32x4n &X1, f32x4n &X2, float4 (*lds)[kTbWaves][64],
                                              float (*tx)[kTbWaves][2]) {
    constexpr int sl = J, sp = (J + 2) % 3;  // slots of planes p and p-1
    __amdgpu_buffer_rsrc_t rs, rc;
    uint32_t ss = 0, sc = 0;
    if constexpr (WH) {
        rs = rc = K.rin;
        ss = R.snext;
        sc = R.scur;
    } else {
        rs = plane_rsrc(A.in, tb_pidx(A, p + 1), K.plane, K.pbytes);
        rc = plane_rsrc(A.in, tb_pidx(A, p), K.plane, K.pbytes);
    }
    if (!WIDE || K.w < kTbWaves) {
        I2.row = bload4(rs, K.voff, ss);
        I2.hm = bload4(rs, K.vm, ss);
        I2.hp = bload4(rs, K.vp, ss);
        float ex = 0.f;
        if constexpr (WIDE) ex = bload1(rc, K.vex, sc);
        // the step's normals of plane p's quad: drawn once, used by both stages
        X2 = tb_noise<NZ>(A, noise_prefix(R.qz + K.qoff, K.nw0.a0), K.nw0);
        float lft, rgt;
        if constexpr (WIDE) {
            lft = from_left_lane_or(I1.row.w, ex);
            rgt = from_right_lane_or(I1.row.x, ex);
        } else {
            lft = from_left_lane(I1.row.w);
            rgt = from_right_lane(I1.row.x);
        }
        T2 = site_update4<NZ>(I1.row, lft, rgt, I1.hm, I1.hp, I0.row, I2.row, X2, A, A.fin != 0, K.m2v);
        lds[sl][K.w][K.lane] = T2;
    } else {
        // the x-halo wave: stage 1 at its 16 sites of plane p
        I2.row.x = bload1(rs, K.voff, ss);
        const float xm = bload1(rc, K.vex, sc), xp = bload1(rc, K.vx2, sc), ym = bload1(rc, K.vm, sc),
                    yp = bload1(rc, K.vp, sc);
        const f32x4n n = tb_noise<NZ>(A, noise_prefix(R.qz + K.qoff, K.nw0.a0), K.nw0);
        // lanes 0..7 hold x0-1 (component 3 of its quad), 8..15 x0+256 (component 0)
        const float xi = K.lane >= 8 ? n.a : n.d;
        const float t = tb_site(I1.row.x, xm, xp, ym, yp, I0.row.x, I2.row.x, xi, A, NZ);
        if (K.lane < 16) tx[sl][(K.lane & 7) + 1][K.lane >> 3] = t;
    }
    __syncthreads();
    if (K.outw && p > K.z0) {
        const float4 up = lds[sp][K.w - 1][K.lane], dn = lds[sp][K.w + 1][K.lane];
        float lft, rgt;
        if constexpr (WIDE) {
            const float2 e = *reinterpret_cast<const float2 *>(&tx[sp][K.w][0]);  // one broadcast LDS read
            lft = from_left_lane_or(T1.w, e.x);
            rgt = from_right_lane_or(T1.x, e.y);
        } else {
            lft = from_left_lane(T1.w);
            rgt = from_right_lane(T1.x);
        }
        // stage 2 reads stage 1's guarded output: always finite (the file header)
        const float4 e = site_update4<NZ>(T1, lft, rgt, up, dn, T0, T2, X1, A, true, K.m2v);
        const float cl = A.clampv;
        float4 o;  // phi = I0.row: the step's input at plane p-1, still in the queue
        o.x = heun_guard(__fmul_rn(0.5f, __fadd_rn(I0.row.x, e.x)), cl);
        o.y = heun_guard(__fmul_rn(0.5f, __fadd_rn(I0.row.y, e.y)), cl);
        o.z = heun_guard(__fmul_rn(0.5f, __fadd_rn(I0.row.z, e.z)), cl);
        o.w = heun_guard(__fmul_rn(0.5f, __fadd_rn(I0.row.w, e.w)), cl);
        if constexpr (WH) {
            // the plane offset in the VGPR offset, soffset 0: see bstore4
            bstore4<17>(K.rout, K.voff + (uint32_t)(p - 1 + A.gz) * K.pbytes, o);
        } else {
            const __amdgpu_buffer_rsrc_t ws = plane_rsrc(A.out, p - 1 + A.gz, K.plane, K.pbytes);
            bstore4<17>(ws, K.voff, o);
        }
    }
    // advance to plane p+1
    const uint32_t q = R.qz + K.qplane;
    R.qz = q == K.qwrap ? 0u : q;
    if constexpr (WH) {
        R.scur = R.snext;
        R.snext = p == K.swrap_at ? (uint32_t)A.gz * K.pbytes : R.snext + K.pbytes;
    }
}

// WPE: waves per SIMD the registers are budgeted for, as phi4_tb2_kernel's.
template <bool NZ, bool WIDE, int WPE, bool WH>
__global__ __launch_bounds__((kTbWaves + (WIDE ? 1 : 0)) * 64)
__attribute__((amdgpu_waves_per_eu(WPE))) void phi4_heun_tb_kernel(const Phi4StepArgs A) {
    const int nb = gridDim.x, b = blockIdx.x;
    // y-bands fastest, then x-segments, then z-chunks, consecutive blocks on one XCD (tb_block)
    const TbBlock tbk = tb_block<WIDE>(A, b, nb);
    const int yb = tbk.yb, xs = tbk.xs;
    const int Lx = A.Lx, Ly = A.Ly;
    const int x0 = 256 * xs;
    TbCtx K;
    K.w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    K.lane = threadIdx.x & 63;
    K.outw = K.w >= 1 && K.w <= kTbRows;
    K.z0 = tbk.z0;
    const int z1 = tbk.z1;
    K.z1 = z1;
    K.snapw = 0;
    K.plane = (size_t)Lx * (size_t)Ly;
    K.pbytes = (uint32_t)(K.plane * sizeof(float));
    K.qplane = (uint32_t)(K.plane >> 2);
    if constexpr (WH) {
        const int nbytes = (int)((uint32_t)(A.nz + 2 * A.gz) * K.pbytes);  // < 2^31 (phi4_heun_tb_launch)
        K.rin = __builtin_amdgcn_make_buffer_rsrc((void *)A.in, (short)0, nbytes, 0x00020000);
        K.rout = __builtin_amdgcn_make_buffer_rsrc((void *)A.out, (short)0, nbytes, 0x00020000);
    }
    K.qwrap = (uint32_t)A.Lzg * K.qplane;  // < 2^32 quads (create_phi4)
    K.m2v = f32x2{A.m2, A.m2};
    asm volatile("" : "+v"(K.m2v));  // opaque: kept in VGPRs, not rematerialised from SGPRs per update
    K.swrap_at = A.nz - 2;  // periodic: plane p+1 = nz is local plane 0 (tb_pidx)
    K.nw0 = A.nw0;          // one counter for both stages: nw1 and da stay unused
    const int xl = (x0 == 0 ? Lx : x0) - 1, xr = x0 + 256 == Lx ? 0 : x0 + 256;  // just outside the segment
    auto wrapy = [Ly](int y) { return y < 0 ? y + Ly : (y >= Ly ? y - Ly : y); };
    if (!WIDE || K.w < kTbWaves) {
        const int y = wrapy(yb * kTbRows - 1 + K.w);
        const int ym = wrapy(y - 1), yp = wrapy(y + 1);
        K.voff = (uint32_t)((y * Lx + x0 + 4 * K.lane) * 4);
        K.vm = (uint32_t)((ym * Lx + x0 + 4 * K.lane) * 4);
        K.vp = (uint32_t)((yp * Lx + x0 + 4 * K.lane) * 4);
        K.vex = (uint32_t)((y * Lx + (K.lane == 63 ? xr : xl)) * 4);
        K.vx2 = 0;
        K.qoff = (uint32_t)((y * Lx + x0 + 4 * K.lane) >> 2);
    } else {  // x-halo wave lanes 0..7: (x0-1, y0+l); 8..15: (x0+256, y0+l-8); the rest repeat lane 0
        const int l = K.lane < 16 ? K.lane : 0;
        const int y = wrapy(yb * kTbRows + (l & 7)), ym = wrapy(y - 1), yp = wrapy(y + 1);
        const int xe = (l >> 3) ? xr : xl;
        const int xem = xe == 0 ? Lx - 1 : xe - 1, xep = xe == Lx - 1 ? 0 : xe + 1;
        K.voff = (uint32_t)((y * Lx + xe) * 4);
        K.vex = (uint32_t)((y * Lx + xem) * 4);
        K.vx2 = (uint32_t)((y * Lx + xep) * 4);
        K.vm = (uint32_t)((ym * Lx + xe) * 4);
        K.vp = (uint32_t)((yp * Lx + xe) * 4);
        K.qoff = (uint32_t)((y * Lx + xe) >> 2);
    }
    __shared__ float4 lds[3][kTbWaves][64];
    __shared__ float tx[WIDE ? 3 : 1][kTbWaves][2];

    TbIn I0, I1, I2;
    {
        const __amdgpu_buffer_rsrc_t r0 = plane_rsrc(A.in, tb_pidx(A, K.z0 - 2), K.plane, K.pbytes);
        const __amdgpu_buffer_rsrc_t r1 = plane_rsrc(A.in, tb_pidx(A, K.z0 - 1), K.plane, K.pbytes);
        if (!WIDE || K.w < kTbWaves) {
            I0.row = bload4(r0, K.voff);
            I0.hm = I0.hp = I0.row;
            I1.row = bload4(r1, K.voff);
            I1.hm = bload4(r1, K.vm);
            I1.hp = bload4(r1, K.vp);
        } else {
            I0.row = make_float4(bload1(r0, K.voff), 0.f, 0.f, 0.f);
            I1.row = make_float4(bload1(r1, K.voff), 0.f, 0.f, 0.f);
            I0.hm = I0.hp = I1.hm = I1.hp = I0.row;
        }
    }
    float4 T0 = make_float4(0.f, 0.f, 0.f, 0.f), T1 = T0, T2 = T0;
    f32x4n X0{0.f, 0.f, 0.f, 0.f}, X1 = X0, X2 = X0;  // the step's normals, rotating as T
    TbRun R;
    R.scur = (uint32_t)tb_pidx(A, K.z0 - 1) * K.pbytes;
    R.snext = (uint32_t)tb_pidx(A, K.z0) * K.pbytes;
    R.qz = (uint32_t)global_z(A, K.z0 - 1) * K.qplane;
    R.qzm = 0;
    // three-plane queues unrolled three ways so no rotation moves are emitted; one exit, at the loop's end
    // (phi4_tb2_kernel's carried-queue form)
    const PrioQ pq(K.z0, z1 - K.z0 + 2);
    for (int p = K.z0 - 1; p <= z1; p += 3) {
        if (A.prio) pq.set(p);
        heun_tb_plane<NZ, WIDE, WH, 0>(A, K, R, p, I0, I1, I2, T0, T1, T2, X1, X2, lds, tx);
        if (p + 1 <= z1) {
            heun_tb_plane<NZ, WIDE, WH, 1>(A, K, R, p + 1, I1, I2, I0, T1, T2, T0, X2, X0, lds, tx);
            if (p + 2 <= z1) heun_tb_plane<NZ, WIDE, WH, 2>(A, K, R, p + 2, I2, I0, I1, T2, T0, T1, X0, X1, lds, tx);
        }
    }
}

template <bool NZ, bool WIDE, int WPE>
const void *heun_tb_fn(bool wh) {
    return wh ? (const void *)&phi4_heun_tb_kernel<NZ, WIDE, WPE, true>
              : (const void *)&phi4_heun_tb_kernel<NZ, WIDE, WPE, false>;
}

}  // namespace

bool phi4_heun_tb_supported(int Lx, int Ly, int Lz) { return Lx > 0 && Lx % 256 == 0 && Ly > 0 && Ly % kTbRows == 0 && Lz >= 2; }

bool phi4_heun_tb_one_descriptor(long long Lx, long long Ly, long long nz, long long gz) {
    return (nz + 2 * gz) * Lx * Ly * 4 < (1ll << 31);
}

hipError_t phi4_heun_tb_launch(const Phi4StepArgs &a, hipStream_t s) {
    // tb2's argument checks for the periodic single slab: one range [0, nz) in nzr chunks of zc planes
    if (!phi4_heun_tb_supported(a.Lx, a.Ly, a.nz) || a.in == nullptr || a.out == nullptr || a.in == a.out ||
        a.nunits <= 0 || a.nxseg != a.Lx / 256 || a.nyg != a.Ly / kTbRows || a.nzr < 1 || a.nzc != a.nzr ||
        a.nunits != a.nxseg * a.nyg * a.nzc || a.zc < 1 || (long long)a.zc * a.nzr < a.zlen ||
        (long long)a.zc * (a.nzr - 1) >= a.zlen)
        return hipErrorInvalidValue;
    if (!a.periodic || a.zlo != 0 || a.zlen != a.nz || a.gz < 0 || a.Lzg != (long long)a.nz || a.zg0 != 0)
        return hipErrorInvalidValue;
    if (a.gate != nullptr || a.flag != nullptr || a.st_md != nullptr || a.st_a != nullptr || a.snap != nullptr ||
        a.dcoef != nullptr || a.stamps != nullptr || a.tctl != nullptr || a.fold.cin != nullptr || a.clr.md != nullptr)
        return hipErrorInvalidValue;
    const bool wide = a.nxseg > 1, nz = a.sig != 0.0f;
    const bool wh = phi4_heun_tb_one_descriptor(a.Lx, a.Ly, a.nz, a.gz);
    // the wide instances' register budget: 1 (88 VGPRs, no scratch) measured 346 us per step at 512^3 against
    // 399 for 6 (80 VGPRs, 24-36 B of scratch per lane); SQ_HEUN_TB_WPE=6 pins the other, as SQ_TB2_WPE does tb2's
    static const int wpe = getenv("SQ_HEUN_TB_WPE") ? atoi(getenv("SQ_HEUN_TB_WPE")) : 1;
    const void *fn;
    if (wide && wpe == 6)
        fn = nz ? heun_tb_fn<true, true, 6>(wh) : heun_tb_fn<false, true, 6>(wh);
    else if (wide)
        fn = nz ? heun_tb_fn<true, true, 1>(wh) : heun_tb_fn<false, true, 1>(wh);
    else
        fn = nz ? heun_tb_fn<true, false, 1>(wh) : heun_tb_fn<false, false, 1>(wh);
    Phi4StepArgs q = a;
    static const int prio = getenv("SQ_TB2_PRIO") ? atoi(getenv("SQ_TB2_PRIO")) : 1;  // tb2's switch
    q.prio = prio;
    void *args[] = {&q};
    return hipLaunchKernel(fn, dim3((unsigned)a.nunits), dim3((kTbWaves + (wide ? 1 : 0)) * 64), args, 0, s);
}

}  // namespace sq
