"""The NumPy statement of the Swendsen-Wang cluster sweep of include/stochquant.h: the per-site Philox blocks, the
forward bonds, the connected components labelled by their smallest site index, the flips and the statistics.  The
oracle of test_gpu_phi4_ens_cluster.py; checked without a GPU by test_phi4_cluster_model.py.

Everything works on a batch of N independent lattices of one shape, phi of shape (N, sites) in the row order of the
field array, site i = (z Ly + y) Lx + x; the shape (Lx, Ly, Lz) is free here (2 x 2 x 2 serves the enumeration)."""
import numpy as np

STREAM_CLUSTER = 5      # kPhi4EnsStreamCluster (sq_phi4_ens.h)
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 of the counters (c0, c1, c2, c3) under the keys (k0, k1), all broadcastable integer arrays:
    the four output words as uint32 arrays.  oracle.philox's values (test_phi4_cluster_model.py compares)."""
    c = [np.asarray(v, dtype=np.uint64) & _LO for v in np.broadcast_arrays(c0, c1, c2, c3)]
    k0, k1 = np.asarray(k0, dtype=np.uint64) & _LO, np.asarray(k1, dtype=np.uint64) & _LO
    for r in range(10):
        if r:
            k0, k1 = (k0 + np.uint64(_W0)) & _LO, (k1 + np.uint64(_W1)) & _LO
        p0, p1 = _M0 * c[0], _M1 * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ k0, p1 & _LO, (p0 >> _S32) ^ c[3] ^ k1, p0 & _LO]
    return [v.astype(np.uint32) for v in c]


def blocks(seeds, c, sites):
    """o[n, i, 0 .. 3]: the block of site i of lattice n at sweep counter c under the lattice's seed."""
    seeds = np.asarray(seeds, dtype=np.uint64).reshape(-1, 1)
    i = np.arange(sites, dtype=np.uint64).reshape(1, -1)
    w = philox(i, STREAM_CLUSTER << 24, c & 0xFFFFFFFF, c >> 32, seeds & _LO, seeds >> _S32)
    return np.stack(w, axis=-1)


def beta(rec):
    """β = 2 h / (sig sig) of a replica from its record (h, m2, lam6, sig), floats held in double."""
    h, sig = float(rec[0]), float(rec[3])
    return 2.0 * h / (sig * sig)


def forward(shape):
    """fwd[mu][i]: the periodic forward neighbour of site i in direction mu = x, y, z."""
    Lx, Ly, Lz = shape
    idx = np.arange(Lx * Ly * Lz).reshape(Lz, Ly, Lx)
    return np.stack([np.roll(idx, -1, axis=2 - mu).reshape(-1) for mu in range(3)])


def bonds(phi, betas, o, shape, factor=2.0):
    """(bits, margin): bits[n, i] holds the forward bonds of site i in bits 0, 1, 2 = x, y, z -- on iff t = φ_i φ_j >
    0 and u >= exp(-(factor β) t), factor = 2 in the definition --, and margin the smallest |exp(..) - u| over the
    bonds with t > 0 (inf without one): below 1e-12 a bond cannot be decided across two exp implementations."""
    phi = np.asarray(phi, dtype=np.float32)
    with np.errstate(invalid="ignore"):         # a signalling NaN among the inputs
        f = phi.astype(np.float64)
    b = np.asarray(betas, dtype=np.float64).reshape(-1, 1)
    bits = np.zeros(phi.shape, dtype=np.uint8)
    margin = np.inf
    for mu, nb in enumerate(forward(shape)):
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            t = f * f[:, nb]
            u = (o[:, :, mu].astype(np.float64) + 0.5) * 2.0 ** -32
            thr = np.exp(-(factor * b) * t)
            pos = t > 0.0
            on = pos & (u >= thr)
        if pos.any():
            margin = min(margin, float(np.abs(thr[pos] - u[pos]).min()))
        bits |= (on.astype(np.uint8) << mu)
    return bits, margin


def components(bits, shape):
    """(labels, passes): labels[n, i] the smallest site index of the connected component of site i in the graph of
    lattice n's on-bonds, by minimum propagation over the bonds with pointer jumping."""
    N, sites = bits.shape
    lab = np.tile(np.arange(sites, dtype=np.int64), (N, 1))
    off = (np.arange(N, dtype=np.int64) * sites).reshape(-1, 1)
    src, dst = [], []
    for mu, nb in enumerate(forward(shape)):
        n, i = np.nonzero((bits >> mu) & 1)
        src.append(n * sites + i)
        dst.append(n * sites + nb[i])
    src, dst = np.concatenate(src), np.concatenate(dst)
    g = (lab + off).reshape(-1)                 # global indices: lattice n's sites are n sites + i
    passes = 0
    while True:
        passes += 1
        new = g.copy()
        np.minimum.at(new, src, g[dst])
        np.minimum.at(new, dst, g[src])
        new = np.minimum(new, new[new])
        if np.array_equal(new, g):
            break
        g = new
    return (g.reshape(N, sites) - off).astype(np.int32), passes


def sweep(phi, betas, seeds, c, shape, factor=2.0):
    """One sweep of every lattice: a dict with the new fields "phi" (only sign bits differ), "bits", "labels",
    "margin", "flip" (bool per site), and "stats" [n] = (clusters, flipped clusters, flipped sites)."""
    phi = np.ascontiguousarray(phi, dtype=np.float32)
    N, sites = phi.shape
    o = blocks(seeds, c, sites)
    bits, margin = bonds(phi, betas, o, shape, factor)
    lab, passes = components(bits, shape)
    odd = (o[:, :, 3] & 1).astype(bool)
    flip = np.take_along_axis(odd, lab.astype(np.int64), axis=1)
    root = lab == np.arange(sites)[None, :]
    new = (phi.view(np.uint32) ^ (flip.astype(np.uint32) << np.uint32(31))).view(np.float32)
    stats = np.stack([root.sum(axis=1), (root & odd).sum(axis=1), flip.sum(axis=1)], axis=1).astype(np.int64)
    return {"phi": new, "bits": bits, "labels": lab, "margin": margin, "flip": flip, "stats": stats, "passes": passes}


def exact_weights(mags, live, beta_, shape):
    """The exact probabilities of the 2^n sign configurations of the n live sites (indices `live`, magnitudes
    `mags`, every other site decoupled) under exp(β Σ_bonds φ_i φ_j), the sum over all forward bonds of the
    lattice -- a doubled bond (extent 2) counts twice.  Configuration k has sign -1 at live site j iff bit j of k."""
    n = len(live)
    pos = {s: j for j, s in enumerate(live)}
    k = np.arange(2 ** n)
    s = 1.0 - 2.0 * ((k[:, None] >> np.arange(n)[None, :]) & 1)
    v = s * np.asarray(mags, dtype=np.float64)[None, :]
    e = np.zeros(2 ** n)
    for nb in forward(shape):
        for i in live:
            if int(nb[i]) in pos:
                e += v[:, pos[i]] * v[:, pos[int(nb[i])]]
    w = np.exp(beta_ * e)
    return w / w.sum()


def sign_code(phi, live):
    """The configuration number of exact_weights for every lattice of phi (N, sites)."""
    neg = np.signbit(np.asarray(phi)[:, live]).astype(np.int64)
    return (neg << np.arange(len(live))[None, :]).sum(axis=1)


def diameter(bits_row, shape, label_row, root):
    """The eccentricity of site `root` in its cluster (BFS over the on-bonds of one lattice): a lower bound of the
    cluster's graph diameter, and the number of passes plain minimum propagation needs to carry the root's label
    to the farthest site."""
    fwd = forward(shape)
    sites = bits_row.shape[0]
    adj = [[] for _ in range(sites)]
    for mu in range(3):
        for i in np.nonzero((bits_row >> mu) & 1)[0]:
            j = int(fwd[mu][i])
            adj[int(i)].append(j)
            adj[j].append(int(i))
    dist = {int(root): 0}
    frontier = [int(root)]
    while frontier:
        nxt = []
        for i in frontier:
            for j in adj[i]:
                if j not in dist:
                    dist[j] = dist[i] + 1
                    nxt.append(j)
        frontier = nxt
    assert all(int(label_row[i]) == int(root) for i in dist)
    return max(dist.values())


# ---- the uploaded fields of the oracle test (test_gpu_phi4_ens_cluster.py), made here so that every property
# they are there for is asserted without a GPU (test_phi4_cluster_model.py) ----
ORACLE_DTAU = 0.01
ORACLE_C = (1.0, 0.7, 1.0, 0.25)        # per replica; 0.25: β = 16, a bond between two sites at 4 is on for certain
ORACLE_SWEEPS = (7, 2 ** 40 + 5)        # two sweeps from each counter: the high counter word is used
ORACLE_SEED0 = 0x5EEDC1


def oracle_seeds(R, base=ORACLE_SEED0):
    return [base + 0x9E3779B97F4A7C15 * (r + 1) & (2 ** 64 - 1) for r in range(R)]


def serpentine(shape):
    """The sites of a self-avoiding path with no lattice bond between two of its sites other than consecutive ones,
    in path order, from site 0.  In a plane: the rows y = 0, 2, .. <= Ly - 2 over x = 0 .. Lx - 2, joined at
    alternating ends through one site of the odd row between them (Ly = 2: one row and the site beside its end);
    the planes z = 0, 2, .. <= Lz - 2 hold the same sites, walked to and fro, joined through one site of the odd
    plane between them.  Row Ly - 1, column Lx - 1 and plane Lz - 1 stay empty, so no periodic wrap closes it."""
    Lx, Ly, Lz = shape
    plane = []
    for k, y in enumerate(range(0, Ly - 1, 2)):
        xs = list(range(Lx - 1))
        if k % 2:
            xs.reverse()
        if k:
            plane.append((xs[0], y - 1))
        plane += [(x, y) for x in xs]
    if Ly == 2:
        plane.append((Lx - 2, 1))
    path = []
    for k, z in enumerate(range(0, Lz - 1, 2)):
        pl = plane[::-1] if k % 2 else plane
        if k:
            path.append((pl[0][0], pl[0][1], z - 1))
        path += [(x, y, z) for x, y in pl]
    return [(z * Ly + y) * Lx + x for x, y, z in path]


def oracle_fields(shape):
    """The four start fields (4, sites) float32 of `shape`: (0) iid normal x 0.6, (1) all positive, |normal| + 0.5,
    (2) two z-domains of opposite sign at magnitude 1.2, (3) +4 along serpentine(shape), +1e-30 elsewhere."""
    Lx, Ly, Lz = shape
    sites = Lx * Ly * Lz
    rng = np.random.default_rng([Lx, Ly, Lz, 2024])
    f = np.empty((4, sites), dtype=np.float32)
    f[0] = (0.6 * rng.normal(size=sites)).astype(np.float32)
    f[1] = (np.abs(rng.normal(size=sites)) + 0.5).astype(np.float32)
    z = np.arange(sites) // (Lx * Ly)
    f[2] = np.where(z < Lz // 2, 1.2, -1.2).astype(np.float32)
    f[3] = np.float32(1e-30)
    f[3, serpentine(shape)] = np.float32(4.0)
    return f


def record(dtau, m2, lam, C):
    """The replica's float record in double: h, m2, lam6, sig (phi4_base_args' expressions)."""
    import math
    h = np.float32(dtau)
    lam6 = np.float32(float(np.float32(lam)) / 6.0)
    sig = np.float32(math.sqrt(2.0 * float(h)) * C)
    return float(h), float(np.float32(m2)), float(lam6), float(sig)


def oracle_betas(C=ORACLE_C, dtau=ORACLE_DTAU):
    return [beta(record(dtau, 0.0, 0.0, c)) for c in C]


def oracle_run(shape):
    """The model's four sweeps (ORACLE_SWEEPS, two from each counter) of oracle_fields(shape): a list of
    (c, sweep(..) result), each from the previous one's fields."""
    phi = oracle_fields(shape)
    seeds, betas = oracle_seeds(4), oracle_betas()
    out = []
    for c0 in ORACLE_SWEEPS:
        for c in (c0, c0 + 1):
            res = sweep(phi, betas, seeds, c, shape)
            out.append((c, res))
            phi = res["phi"]
    return out


# ---- detailed balance by enumeration: eight live sites with fixed magnitudes, everything else decoupled ----
DB_CHI2_BOUND = 255.0 + 6.0 * np.sqrt(510.0)     # χ² of 255 degrees of freedom: mean + 6 σ, about 390
DB_MIN_EXPECTED = 5.0
DB_C = 1.6                                       # β = 1 / C² = 0.39: the rarest configuration is expected >= 5 times
DB_SHAPE, DB_R, DB_SNAPSHOTS, DB_GAP = (8, 2, 2), 4096, 8, 10      # the device's graph: 32,768 samples


def db_magnitudes():
    """Eight magnitudes in [0.3, 0.8]."""
    return np.asarray([0.55, 0.3, 0.8, 0.45, 0.7, 0.35, 0.6, 0.5], dtype=np.float32)


def db_live(shape):
    """The live sites: all eight of 2 x 2 x 2; x in {0, 1} of 8 x 2 x 2 (a single x-bond, doubled y- and z-bonds)."""
    Lx, Ly, Lz = shape
    return [(z * Ly + y) * Lx + x for z in range(2) for y in range(2) for x in range(2)]


def db_start(shape, N, seed=99):
    """(N, sites) start fields: db_magnitudes() with random signs at the live sites, +1e-30 elsewhere (a bond to
    such a site is off for certain: exp rounds to 1 > u)."""
    rng = np.random.default_rng(seed)
    live = db_live(shape)
    f = np.full((N, shape[0] * shape[1] * shape[2]), 1e-30, dtype=np.float32)
    f[:, live] = db_magnitudes()[None, :] * rng.choice(np.float32([-1.0, 1.0]), size=(N, 8))
    return f


def chi2(codes, p):
    """(χ², smallest expected count) of the sample of configuration numbers against the probabilities p."""
    n = np.bincount(codes, minlength=len(p)).astype(np.float64)
    e = p * len(codes)
    return float(((n - e) ** 2 / e).sum()), float(e.min())
