// sq_phi4_cluster.hip -- Swendsen-Wang cluster sweeps of the single phi^4
// lattice (sq_phi4_cluster): the ensemble's sweep
// (include/stochquant.h, the block above sq_phi4_ens_cluster; clu_bond of
// sq_phi4_ens_cluster_dev.h is the one bond rule) for a field that lives in
// device memory, so that the labelling has to cross work-groups.
//
// One sweep is three launches on one stream.  Launch boundaries are the only
// grid-wide ordering: no kernel waits for another work-group, none is launched
// cooperatively, none polls.  Beside the field a sweep uses one uint32 label
// and one bond byte per site.
//
//   1. phi4_cluster_tile_kernel, one work-group per brick of tx x ty x tz sites
//      (partial last bricks in y and z; tx divides Lx).  A lane takes the sites
//      l = lane, lane + 512, .. of the brick, l = (lz ey + ly) tx + lx the
//      brick-local index, which orders the brick's sites as the global index
//      does.  Per site: phi_i and its three periodic forward neighbours from
//      device memory (the neighbours are cache hits: the brick's own sites but
//      for one face per direction), the site's Philox block, the three bond
//      bits by clu_bond, the bond byte to device memory.  A forward bond stays
//      IN THE BRICK iff the neighbour's local coordinate is the site's plus one:
//      a bond through the periodic wrap is a seam bond even where the brick
//      spans the axis, which is what makes extents 1 (the site its own
//      neighbour) and 2 (a doubled bond) no special case.  The in-brick bits go
//      to a byte per site in LDS; behind a barrier every site adds its three
//      backward bits from the bytes of l - 1, l - tx, l - tx ey.  No coordinate
//      is needed for that: where the site has no such neighbour in the brick,
//      that index is below 0 or names the last site of the row or plane before,
//      whose forward bit was cleared as leaving the brick.  (The byte is updated
//      in place while neighbours read its bits 0 .. 2, which the update keeps.)
//      Then the ensemble's passes on the LDS labels (the proof is in the header
//      comment of sq_phi4_ens_cluster_dev.h): minimum over the bonded
//      neighbours at l +- 1, l +- tx, l +- tx ey, pointer jumping, the parent
//      hooked by ds_min_u32, the three rotating flags, a bound of sites-in-brick
//      + 1 passes.  label[i] = the global index of the local root.  A brick
//      that reaches the bound raises the sweep's trip word and writes
//      label[i] = i.
//
//   2. phi4_cluster_seam_kernel, one lane per quad of four x-consecutive sites
//      (one 32-bit load of their bond bytes; a quad without an on-bond ends
//      there).  Every on-bond that leaves its brick -- the local coordinate is
//      the brick's last one, the periodic wrap included -- is united in the
//      label array by clu_unite:
//          find both roots; if equal, done;
//          old = atomicMin(&L[hi], lo);
//          old == hi: hi was a root and now points to lo, done;
//          else continue with (old, lo).
//      Why it ends and is right.  (a) A word only falls: every write to L in
//      this kernel is an atomic minimum.  (b) Every value a word ever holds is
//      a site of the word's own component: it starts as the local root, and
//      every minimum written is a root found from a site bonded to it, or a
//      value read from such a word.  (c) Hence L[i] <= i always, and a chain
//      i, L[i], L[L[i]], .. is strictly decreasing until it meets a word with
//      L[r] = r: find walks `while ((p = L[r]) < r) r = p`, which strictly
//      lowers r whatever the memory holds.  (d) A retry continues with old < hi
//      (else it ends), and lo is where the other chain stood: inside one
//      clu_unite both chains only ever move down, so hops and retries together
//      are at most 2 sites.  That is the written bound, 2 sites + 2; a lane that
//      reaches it raises the trip word and ends.  It cannot spin.  (e) A link
//      hi -> lo is made only where the atomic saw hi as a root, so the links
//      form a forest whose trees are the components once every seam bond has
//      been united, and the root of a tree is its smallest index (it points to
//      nothing smaller of its own component).  Stale reads are harmless: an
//      older parent is a larger site of the same component whose own chain
//      leads to the same root, and the atomic's return value, not the read,
//      decides a link.  find also lowers the word of the first site it left to
//      the root it found (one atomic minimum without a return value): the
//      seam sites of one local cluster share that word, the local root's.
//      Only plain vector atomics on global memory.
//
//   3. phi4_cluster_flip_kernel, one lane per quad.  Each site chases its chain
//      to the root (the same strictly decreasing walk: at most i + 1 reads by
//      construction, no bound to reach) and the quad writes the roots back as
//      the final labels; a racing reader sees an older parent or the final one,
//      both valid.  The root's Philox word 3 is computed again (once per run of
//      equal labels in the quad); odd: the sign bit is toggled, the quad stored
//      only where a bit changed.  Clusters (label == index), flipped clusters
//      and flipped sites are integers: a lane's three counts go to three LDS
//      words, the block's to the device record by one 64-bit atomic add each,
//      so any order gives the same totals.  Where the trip word is raised the
//      kernel writes no field word and no label and counts one unconverged
//      sweep.  Lane 0 counts the sweep and clears the other trip word.
//
// The brick.  LDS holds 5 bytes per site (label, bond byte), so LDS would
// admit 32,000 sites.  Against that: the passes a brick needs grow with the
// length of the longest cluster path inside it, every pass costs a barrier of
// the whole work-group, and a work-group alone on its CU has nothing to hide
// the barrier behind.  8192 sites are 40 KiB: three work-groups of 512 lanes
// per CU.  The seam surface falls slowly beyond that: the forward bonds that
// leave a brick are 1/tx + 1/ty + 1/tz per site, 0.156 at 32 x 16 x 16, 0.125
// at 32 x 32 x 16 (twice the sites).  x is cut at 32 (or Lx below that), a
// power of two so that lx is a mask and a quad never straddles a seam; y at 16;
// z takes what is left of 8192 sites (16 at the full 32 x 16), which becomes
// deeper where Lx or Ly are small.  SQ_CLUSTER_TILE overrides it.
#include "sq_phi4_ens_cluster_dev.h"  // clu_bond, clu_min; philox4x32_10 and ens_smem through sq_phi4_ens_dev.h
#include "sq_phi4_cluster.h"

namespace sq {

namespace {

constexpr uint32_t kCluStr = kPhi4EnsStreamCluster << 24;

struct CluBrick {
    int x0, y0, z0, ey, ez;
};

__device__ __forceinline__ CluBrick clu_brick(const Phi4ClusterArgs &A) {
    const int b = blockIdx.x;
    const int bx = b % A.t.ntx, r = b / A.t.ntx, by = r % A.t.nty, bz = r / A.t.nty;
    CluBrick k;
    k.x0 = bx * A.t.tx;
    k.y0 = by * A.t.ty;
    k.z0 = bz * A.t.tz;
    k.ey = min(A.t.ty, A.Ly - k.y0);
    k.ez = min(A.t.tz, A.Lz - k.z0);
    return k;
}

// the global index of brick-local site l
__device__ __forceinline__ uint32_t clu_global(const Phi4ClusterArgs &A, const CluBrick &k, int l, int &lx, int &ly,
                                               int &lz) {
    lx = l & (A.t.tx - 1);
    const int r = l >> A.ltx;
    lz = r / k.ey;
    ly = r - lz * k.ey;
    return ((uint32_t)(k.z0 + lz) * (uint32_t)A.Ly + (uint32_t)(k.y0 + ly)) * (uint32_t)A.Lx + (uint32_t)(k.x0 + lx);
}

__global__ __launch_bounds__(kPhi4ClusterLanes) void phi4_cluster_tile_kernel(const Phi4ClusterArgs A) {
#pragma clang fp contract(off)
    const CluBrick k = clu_brick(A);
    const int tx = A.t.tx, pl = tx * k.ey, N = pl * k.ez, cap = tx * A.t.ty * A.t.tz;
    const int T = blockDim.x;
    uint32_t *lab = reinterpret_cast<uint32_t *>(ens_smem);
    uint8_t *msk = reinterpret_cast<uint8_t *>(ens_smem + 4 * (size_t)cap);
    uint32_t *flag = reinterpret_cast<uint32_t *>(ens_smem + 5 * (size_t)cap);  // cap is a multiple of 8
    const double beta = 2.0 * (double)A.h / ((double)A.sig * (double)A.sig);
    const double nb2 = -(2.0 * beta);
    const uint32_t plane = (uint32_t)A.Lx * (uint32_t)A.Ly;
    const float *F = A.field;

    // bonds: the byte to device memory, the in-brick bits and label = l to LDS
    for (int l = threadIdx.x; l < N; l += T) {
        int lx, ly, lz;
        const uint32_t i = clu_global(A, k, l, lx, ly, lz);
        const uint32_t jx = k.x0 + lx + 1 == A.Lx ? i - (uint32_t)(A.Lx - 1) : i + 1u;
        const uint32_t jy = k.y0 + ly + 1 == A.Ly ? i - (uint32_t)(A.Ly - 1) * (uint32_t)A.Lx : i + (uint32_t)A.Lx;
        const uint32_t jz = k.z0 + lz + 1 == A.Lz ? i - (uint32_t)(A.Lz - 1) * plane : i + plane;
        const float a = F[i], ax = F[jx], ay = F[jy], az = F[jz];
        const u32x4 o = philox4x32_10(u32x4{i, kCluStr, A.clo, A.chi}, A.k0, A.k1);
        const uint32_t g = clu_bond(a, ax, o.x, nb2) | (clu_bond(a, ay, o.y, nb2) << 1) | (clu_bond(a, az, o.z, nb2) << 2);
        A.bonds[i] = (uint8_t)g;
        const uint32_t in = (lx + 1 < tx ? 1u : 0u) | (ly + 1 < k.ey ? 2u : 0u) | (lz + 1 < k.ez ? 4u : 0u);
        msk[l] = (uint8_t)(g & in);
        lab[l] = (uint32_t)l;
    }
    if (threadIdx.x < 3) flag[threadIdx.x] = 0u;
    __syncthreads();
    // backward bits 3 .. 5 from the neighbours' forward bits; bits 0 .. 2 of every byte stay as they are
    for (int l = threadIdx.x; l < N; l += T) {
        uint32_t b = msk[l];
        if (l >= 1 && (msk[l - 1] & 1u)) b |= 8u;
        if (l >= tx && (msk[l - tx] & 2u)) b |= 16u;
        if (l >= pl && (msk[l - pl] & 4u)) b |= 32u;
        msk[l] = (uint8_t)b;
    }
    __syncthreads();

    // the passes
    const int bound = N + 1;
    bool conv = false;
    for (int p = 0; p < bound; ++p) {
        const int fp = p % 3;
        if (threadIdx.x == 0) flag[fp == 2 ? 0 : fp + 1] = 0u;
        bool stored = false;
        for (int l = threadIdx.x; l < N; l += T) {
            const uint32_t b = msk[l];
            if (b == 0u) continue;  // a single site: its label is l
            const uint32_t own = lab[l];
            uint32_t m = own;
            if (b & 1u) m = clu_min(m, lab[l + 1]);
            if (b & 8u) m = clu_min(m, lab[l - 1]);
            if (b & 2u) m = clu_min(m, lab[l + tx]);
            if (b & 16u) m = clu_min(m, lab[l - tx]);
            if (b & 4u) m = clu_min(m, lab[l + pl]);
            if (b & 32u) m = clu_min(m, lab[l - pl]);
            m = clu_min(m, lab[m]);  // m < N: a label of the brick
            if (m < own) {
                atomicMin(&lab[own], m);  // the parent takes the label as well (own == l for a root: one operation)
                if (own != (uint32_t)l) atomicMin(&lab[l], m);
                stored = true;
            }
        }
        if (stored) flag[fp] = 1u;
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane((int)flag[fp]) == 0) {
            conv = true;
            break;
        }
    }
    if (!conv && threadIdx.x == 0) A.st->trip[A.par] = 1;  // block-uniform; the labels below are then the sites' own
    for (int l = threadIdx.x; l < N; l += T) {
        int lx, ly, lz;
        const uint32_t i = clu_global(A, k, l, lx, ly, lz);
        A.label[i] = conv ? clu_global(A, k, (int)lab[l], lx, ly, lz) : i;
    }
}

__device__ __forceinline__ uint32_t clu_load(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root above s: r falls strictly, n counts the hops against bound.  The first site left takes the root found.
__device__ __forceinline__ bool clu_find(uint32_t *L, uint32_t &s, unsigned long long &n, unsigned long long bound) {
    uint32_t r = s, first = s;
    for (;;) {
        const uint32_t p = clu_load(L + r);
        if (p >= r) break;
        if (r == s) first = p;
        r = p;
        if (++n > bound) return false;
    }
    if (first > r) atomicMin(L + first, r);
    s = r;
    return true;
}

// Unite the components of sites a and b (the file's header has the argument); false: the bound was reached.
__device__ __forceinline__ bool clu_unite(uint32_t *L, uint32_t a, uint32_t b, unsigned long long bound) {
    unsigned long long n = 0;
    for (;;) {
        if (!clu_find(L, a, n, bound) || !clu_find(L, b, n, bound)) return false;
        if (a == b) return true;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const uint32_t old = atomicMin(L + hi, lo);
        if (old >= hi) return true;  // hi was a root and points to lo now
        a = old;                     // old < hi: hi had a parent already; that parent's tree and lo's are united instead
        b = lo;
        if (++n > bound) return false;
    }
}

__global__ __launch_bounds__(256) void phi4_cluster_seam_kernel(const Phi4ClusterArgs A) {
    const uint32_t sites = (uint32_t)A.Lx * (uint32_t)A.Ly * (uint32_t)A.Lz;
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= sites / 4u || A.st->trip[A.par] != 0) return;
    const uint32_t w = reinterpret_cast<const uint32_t *>(A.bonds)[q];
    if ((w & 0x07070707u) == 0u) return;
    const uint32_t qrow = (uint32_t)A.Lx / 4u, row = q / qrow, x = 4u * (q - row * qrow);
    const uint32_t z = row / (uint32_t)A.Ly, y = row - z * (uint32_t)A.Ly;
    const uint32_t plane = (uint32_t)A.Lx * (uint32_t)A.Ly;
    const bool ywrap = y + 1u == (uint32_t)A.Ly, zwrap = z + 1u == (uint32_t)A.Lz;
    const bool yseam = ywrap || y % (uint32_t)A.t.ty == (uint32_t)A.t.ty - 1u;
    const bool zseam = zwrap || z % (uint32_t)A.t.tz == (uint32_t)A.t.tz - 1u;
    const bool xseam = ((x + 3u) & (uint32_t)(A.t.tx - 1)) == (uint32_t)(A.t.tx - 1);  // of the quad's last site
    const unsigned long long bound = 2ull * sites + 2ull;
    bool ok = true;
#pragma unroll
    for (uint32_t s = 0; s < 4u; ++s) {
        const uint32_t b = (w >> (8u * s)) & 7u, i = 4u * q + s;
        if (s == 3u && xseam && (b & 1u))
            ok = clu_unite(A.label, i, x + 4u == (uint32_t)A.Lx ? i - (uint32_t)(A.Lx - 1) : i + 1u, bound) && ok;
        if (yseam && (b & 2u))
            ok = clu_unite(A.label, i, ywrap ? i - (uint32_t)(A.Ly - 1) * (uint32_t)A.Lx : i + (uint32_t)A.Lx, bound) && ok;
        if (zseam && (b & 4u))
            ok = clu_unite(A.label, i, zwrap ? i - (uint32_t)(A.Lz - 1) * plane : i + plane, bound) && ok;
    }
    if (!ok) A.st->trip[A.par] = 1;
}

__global__ __launch_bounds__(256) void phi4_cluster_flip_kernel(const Phi4ClusterArgs A) {
    __shared__ uint32_t cnt[3];
    const uint32_t sites = (uint32_t)A.Lx * (uint32_t)A.Ly * (uint32_t)A.Lz;
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (A.st->trip[A.par] != 0) {  // the same word for every block: no launch of this sweep writes it any more
        if (q == 0u) {
            A.st->stat[0] += 1;
            A.st->stat[4] += 1;
            A.st->trip[A.par ^ 1] = 0;
        }
        return;
    }
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0u;
    __syncthreads();
    if (q < sites / 4u) {
        const uint32_t *L = A.label;
        uint32_t l[4];
        uint32_t fb = 0u, prev = 0u, nc = 0u, nfc = 0u, nfs = 0u;
#pragma unroll
        for (uint32_t s = 0; s < 4u; ++s) {
            const uint32_t i = 4u * q + s;
            uint32_t r = i;
            for (;;) {  // r falls strictly: at most i + 1 reads
                const uint32_t p = L[r];
                if (p >= r) break;
                r = p;
            }
            l[s] = r;
            uint32_t odd;
            if (s > 0u && r == l[s > 0u ? s - 1u : 0u]) odd = prev;
            else odd = philox4x32_10(u32x4{r, kCluStr, A.clo, A.chi}, A.k0, A.k1).w & 1u;
            prev = odd;
            fb |= odd << s;
            nc += r == i ? 1u : 0u;
            nfc += (r == i ? 1u : 0u) & odd;
            nfs += odd;
        }
        reinterpret_cast<uint4 *>(A.label)[q] = make_uint4(l[0], l[1], l[2], l[3]);
        if (fb) {
            uint4 *F = reinterpret_cast<uint4 *>(A.field) + q;
            uint4 v = *F;
            v.x ^= (fb & 1u) << 31;
            v.y ^= ((fb >> 1) & 1u) << 31;
            v.z ^= ((fb >> 2) & 1u) << 31;
            v.w ^= ((fb >> 3) & 1u) << 31;
            *F = v;
        }
        if (nc) atomicAdd(&cnt[0], nc);
        if (nfc) atomicAdd(&cnt[1], nfc);
        if (nfs) atomicAdd(&cnt[2], nfs);
    }
    __syncthreads();
    if (threadIdx.x < 3 && cnt[threadIdx.x] != 0u)
        atomicAdd(reinterpret_cast<unsigned long long *>(A.st->stat + 1 + threadIdx.x), (unsigned long long)cnt[threadIdx.x]);
    if (q == 0u) {
        A.st->stat[0] += 1;  // this lane alone writes the word
        A.st->trip[A.par ^ 1] = 0;
    }
}

__global__ void phi4_cluster_reset_kernel(Phi4ClusterState *st) {
    if (threadIdx.x < 5) st->stat[threadIdx.x] = 0;
}

bool clu_args_ok(const Phi4ClusterArgs &a) {
    const Phi4ClusterTile &t = a.t;
    const long long sites = (long long)a.Lx * a.Ly * a.Lz;
    return a.field != nullptr && a.label != nullptr && a.bonds != nullptr && a.st != nullptr && a.Lx >= 8 &&
           (a.Lx & 7) == 0 && a.Ly >= 1 && a.Lz >= 1 && sites < (1ll << 31) && t.tx >= 8 && t.tx <= 256 &&
           (t.tx & (t.tx - 1)) == 0 && t.tx == (1 << a.ltx) && a.Lx % t.tx == 0 && t.ty >= 1 && t.tz >= 1 &&
           (long long)t.tx * t.ty * t.tz <= kPhi4ClusterMaxTile && t.ntx == a.Lx / t.tx &&
           t.nty == (a.Ly + t.ty - 1) / t.ty && t.ntz == (a.Lz + t.tz - 1) / t.tz &&
           t.lds >= 5 * t.tx * t.ty * t.tz + 12 && (a.par == 0 || a.par == 1) && a.sig != 0.0f;
}

unsigned clu_quad_blocks(const Phi4ClusterArgs &a) {
    const long long quads = (long long)a.Lx * a.Ly * a.Lz / 4;
    return (unsigned)((quads + 255) / 256);
}

}  // namespace

hipError_t phi4_cluster_tile_launch(const Phi4ClusterArgs &a, hipStream_t s) {
    if (!clu_args_ok(a)) return hipErrorInvalidValue;
    const long long grid = (long long)a.t.ntx * a.t.nty * a.t.ntz;
    if (grid >= (1ll << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(phi4_cluster_tile_kernel, dim3((unsigned)grid), dim3(kPhi4ClusterLanes), (size_t)a.t.lds, s, a);
    return hipGetLastError();
}

hipError_t phi4_cluster_seam_launch(const Phi4ClusterArgs &a, hipStream_t s) {
    if (!clu_args_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(phi4_cluster_seam_kernel, dim3(clu_quad_blocks(a)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t phi4_cluster_flip_launch(const Phi4ClusterArgs &a, hipStream_t s) {
    if (!clu_args_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(phi4_cluster_flip_kernel, dim3(clu_quad_blocks(a)), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t phi4_cluster_reset_launch(Phi4ClusterState *st, hipStream_t s) {
    if (st == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(phi4_cluster_reset_kernel, dim3(1), dim3(64), 0, s, st);
    return hipGetLastError();
}

}  // namespace sq
