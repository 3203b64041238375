// sq_phi4_ens_corr.cpp -- the phi^4 ensemble's time-slice correlator, its momentum projections, and the replica
// statistics every *correlator call shares.
#include "sq_phi4_ens_host.h"

#include "sq_phi4_ens_ckpt_format.h"

using namespace sq;

namespace sq {

const char *ens_momenta_shape_error(int sites, int Lz) {
    return sq::phi4_ens_shape(sites, Lz).pc_ok
               ? nullptr
               : "the lattice shape leaves no LDS for the momentum projections (16 Lz bytes)";
}

int ens_apply_momenta(sq_phi4_ens *e, int M, const int *nxy) {
    DeviceGuard g(e->dev);
    const size_t Lx = (size_t)e->Lx, Ly = (size_t)e->Ly, R = (size_t)e->R, nt = (size_t)e->nt;
    const size_t nx = SQ_PHI4_ENS_MAX_MOMENTA * Lx, ny = SQ_PHI4_ENS_MAX_MOMENTA * Ly;
    int rc = ens_reserve(e->ptab, 2 * (nx + ny));
    if (!rc) rc = ens_reserve(e->pG, R * (size_t)M * nt);
    if (rc) return rc;
    std::vector<double> tab(2 * (nx + ny), 0.0);
    for (int m = 0; m < M; ++m) {
        rc = sq_phi4_ens_momentum_table(e->Lx, nxy[2 * m], &tab[(size_t)m * Lx], &tab[nx + (size_t)m * Lx]);
        if (!rc)
            rc = sq_phi4_ens_momentum_table(e->Ly, nxy[2 * m + 1], &tab[2 * nx + (size_t)m * Ly],
                                            &tab[2 * nx + ny + (size_t)m * Ly]);
        if (rc) return rc;
    }
    SQ_HIP(hipMemcpy(e->ptab.data(), tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice));
    e->pM = M;  // the accumulators' layout is [R][M][nt] from here on: all of them start over
    for (int i = 0; i < 2 * M; ++i) e->pn[i] = nxy[i];
    if (M > 0) SQ_HIP(hipMemsetAsync(e->pG.data(), 0, sizeof(double) * R * (size_t)M * nt, e->stream));
    SQ_HIP(hipMemsetAsync(e->pN.data(), 0, sizeof(long long) * R, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

Phi4EnsCorrArgs ens_corr_args(const sq_phi4_ens *e) {
    sq::Phi4EnsCorrArgs c{};
    c.G = e->cG.data();
    c.S1 = e->cS1.data();
    c.nmeas = e->cN.data();
    return c;
}

Phi4EnsPCorrArgs ens_pcorr_args(const sq_phi4_ens *e, bool corr) {
    sq::Phi4EnsPCorrArgs p{};
    const size_t nx = (size_t)SQ_PHI4_ENS_MAX_MOMENTA * (size_t)e->Lx, ny = (size_t)SQ_PHI4_ENS_MAX_MOMENTA * (size_t)e->Ly;
    p.Gp = e->pG.data();
    p.nmeas_p = e->pN.data();
    p.cx = e->ptab.data();
    p.sx = e->ptab.data() + nx;
    p.cy = e->ptab.data() + 2 * nx;
    p.sy = e->ptab.data() + 2 * nx + ny;
    p.M = e->pM;
    if (corr) p.corr = ens_corr_args(e);
    return p;
}

int ens_replicas_used(const std::vector<long long> &N, const char *what, int *used, int *u) {
    *u = 0;
    for (long long n : N) *u += n > 0 ? 1 : 0;
    if (used) *used = *u;
    if (*u == 0) return fail(SQ_E_STATE, std::string("no replica has a ") + what + " measurement");
    return SQ_OK;
}

void ens_replica_stats(const sq_phi4_ens *e, const double *G, size_t stride, const double *S1, const long long *N,
                       int u, int n, double *mean, double *err) {
    const size_t R = (size_t)e->R;
    const double V = (double)e->sites, Lz = (double)e->Lz;
    std::vector<double> c((size_t)u);
    for (int t = 0; t < n; ++t) {
        size_t k = 0;
        double sum = 0.0;
        for (size_t r = 0; r < R; ++r) {
            if (N[r] <= 0) continue;
            const double nm = (double)N[r];
            double v = G[r * stride + (size_t)t] / (nm * V);
            if (S1) {
                const double sb = S1[r] / nm;
                v -= sb * sb / (Lz * V);
            }
            c[k++] = v;
            sum += v;
        }
        const double m = sum / (double)u;
        mean[t] = m;
        if (err) {
            double q = 0.0;
            for (int i = 0; i < u; ++i) q += (c[(size_t)i] - m) * (c[(size_t)i] - m);
            err[t] = u > 1 ? sqrt(q / ((double)u * (double)(u - 1))) : 0.0;
        }
    }
}

}  // namespace sq

extern "C" {

int sq_phi4_ens_corr_sums(sq_phi4_ens *e, int first, int count, double *G, double *S1, long long *nmeas) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    const size_t nt = (size_t)e->nt, n = (size_t)count, f = (size_t)first;
    if (G) SQ_HIP(hipMemcpy(G, e->cG.data() + f * nt, sizeof(double) * n * nt, hipMemcpyDeviceToHost));
    if (S1) SQ_HIP(hipMemcpy(S1, e->cS1.data() + f, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (nmeas) SQ_HIP(hipMemcpy(nmeas, e->cN.data() + f, sizeof(long long) * n, hipMemcpyDeviceToHost));
    return SQ_OK;
}

int sq_phi4_ens_corr_reset(sq_phi4_ens *e, int first, int count) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    const size_t nt = (size_t)e->nt, n = (size_t)count, f = (size_t)first;
    SQ_HIP(hipMemsetAsync(e->cG.data() + f * nt, 0, sizeof(double) * n * nt, e->stream));
    SQ_HIP(hipMemsetAsync(e->cS1.data() + f, 0, sizeof(double) * n, e->stream));
    SQ_HIP(hipMemsetAsync(e->cN.data() + f, 0, sizeof(long long) * n, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_slices(sq_phi4_ens *e, int first, int count, double *S, double *g) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0 || (!S && !g)) return SQ_OK;
    DeviceGuard dg(e->dev);
    const size_t nt = (size_t)e->nt, Lz = (size_t)e->Lz, n = (size_t)count;
    rc = ens_reserve(e->ctmp, n * (Lz + nt));
    if (rc) return rc;
    double *devS = e->ctmp.data(), *devg = devS + n * Lz;
    SQ_HIP(sq::phi4_ens_slices_launch(ens_args(e), first, count, devS, devg, e->stream));
    if (S) SQ_HIP(hipMemcpyAsync(S, devS, sizeof(double) * n * Lz, hipMemcpyDeviceToHost, e->stream));
    if (g) SQ_HIP(hipMemcpyAsync(g, devg, sizeof(double) * n * nt, hipMemcpyDeviceToHost, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_correlator(sq_phi4_ens *e, int connected, double *mean, double *err, int n, int *used) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (n < 0 || n > e->nt) return fail(SQ_E_ARG, "n must lie in [0, Lz / 2 + 1]");
    if (!mean && n > 0) return fail(SQ_E_ARG, "null argument");
    const size_t R = (size_t)e->R, nt = (size_t)e->nt;
    std::vector<double> G(R * nt), S1(R);
    std::vector<long long> N(R);
    int rc = sq_phi4_ens_corr_sums(e, 0, e->R, G.data(), S1.data(), N.data()), u;
    if (!rc) rc = ens_replicas_used(N, "correlator", used, &u);
    if (rc) return rc;
    ens_replica_stats(e, G.data(), nt, connected ? S1.data() : nullptr, N.data(), u, n, mean, err);
    return SQ_OK;
}

int sq_phi4_ens_momentum_table(int L, int n, double *c, double *s) {
    if (L < 2 || n < 0 || n >= L) return fail(SQ_E_ARG, "a momentum table needs L >= 2 and 0 <= n < L");
    if (!c || !s) return fail(SQ_E_ARG, "null argument");
    for (int k = 0; k < L; ++k) {
        const long long j = ((long long)n * (long long)k) % (long long)L;
        if ((4 * j) % L == 0) {  // a multiple of a quarter turn: exact
            const int q = (int)(4 * j / L);
            c[k] = q == 0 ? 1.0 : (q == 2 ? -1.0 : 0.0);
            s[k] = q == 1 ? 1.0 : (q == 3 ? -1.0 : 0.0);
        } else {
            const double a = 2.0 * M_PI * (double)j / (double)L;
            c[k] = cos(a);
            s[k] = sin(a);
        }
    }
    return SQ_OK;
}

int sq_phi4_ens_set_momenta(sq_phi4_ens *e, int M, const int *nxy) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (const char *why = sq::ckpt::momenta_error(e->Lx, e->Ly, M, nxy)) return fail(SQ_E_ARG, why);
    if (const char *why = ens_momenta_shape_error((int)e->sites, e->Lz)) return fail(SQ_E_ARG, why);
    return ens_apply_momenta(e, M, nxy);
}

int sq_phi4_ens_get_momenta(sq_phi4_ens *e, int *M, int *nxy) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (!M) return fail(SQ_E_ARG, "null argument");
    *M = e->pM;
    if (nxy)
        for (int i = 0; i < 2 * e->pM; ++i) nxy[i] = e->pn[i];
    return SQ_OK;
}

int sq_phi4_ens_pcorr_sums(sq_phi4_ens *e, int first, int count, double *G, long long *nmeas) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    const size_t row = (size_t)e->pM * (size_t)e->nt, n = (size_t)count, f = (size_t)first;
    if (G && row) SQ_HIP(hipMemcpy(G, e->pG.data() + f * row, sizeof(double) * n * row, hipMemcpyDeviceToHost));
    if (nmeas) SQ_HIP(hipMemcpy(nmeas, e->pN.data() + f, sizeof(long long) * n, hipMemcpyDeviceToHost));
    return SQ_OK;
}

int sq_phi4_ens_pcorr_reset(sq_phi4_ens *e, int first, int count) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (count == 0) return SQ_OK;
    DeviceGuard g(e->dev);
    const size_t row = (size_t)e->pM * (size_t)e->nt, n = (size_t)count, f = (size_t)first;
    if (row) SQ_HIP(hipMemsetAsync(e->pG.data() + f * row, 0, sizeof(double) * n * row, e->stream));
    SQ_HIP(hipMemsetAsync(e->pN.data() + f, 0, sizeof(long long) * n, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_pslices(sq_phi4_ens *e, int first, int count, double *AB, double *g) {
    int rc = ens_range(e, first, count);
    if (rc) return rc;
    if (e->pM == 0) return fail(SQ_E_STATE, "no momenta set (sq_phi4_ens_set_momenta)");
    if (count == 0 || (!AB && !g)) return SQ_OK;
    DeviceGuard dg(e->dev);
    const size_t nab = (size_t)count * (size_t)e->pM * 2 * (size_t)e->Lz, ng = (size_t)count * (size_t)e->pM * (size_t)e->nt;
    rc = ens_reserve(e->ptmp, nab + ng);
    if (rc) return rc;
    double *devAB = e->ptmp.data(), *devg = devAB + nab;
    SQ_HIP(sq::phi4_ens_pslices_launch(ens_args(e), ens_pcorr_args(e, false), first, count, devAB, devg, e->stream));
    if (AB) SQ_HIP(hipMemcpyAsync(AB, devAB, sizeof(double) * nab, hipMemcpyDeviceToHost, e->stream));
    if (g) SQ_HIP(hipMemcpyAsync(g, devg, sizeof(double) * ng, hipMemcpyDeviceToHost, e->stream));
    SQ_HIP(hipStreamSynchronize(e->stream));
    return SQ_OK;
}

int sq_phi4_ens_pcorrelator(sq_phi4_ens *e, double *mean, double *err, int n, int *used) {
    if (!e) return fail(SQ_E_ARG, "null ensemble");
    if (n < 0 || n > e->nt) return fail(SQ_E_ARG, "n must lie in [0, Lz / 2 + 1]");
    if (!mean && n > 0) return fail(SQ_E_ARG, "null argument");
    if (e->pM == 0) return fail(SQ_E_STATE, "no momenta set (sq_phi4_ens_set_momenta)");
    const size_t R = (size_t)e->R, nt = (size_t)e->nt, M = (size_t)e->pM;
    std::vector<double> G(R * M * nt);
    std::vector<long long> N(R);
    int rc = sq_phi4_ens_pcorr_sums(e, 0, e->R, G.data(), N.data()), u;
    if (!rc) rc = ens_replicas_used(N, "momentum", used, &u);
    if (rc) return rc;
    for (size_t m = 0; m < M; ++m)
        ens_replica_stats(e, G.data() + m * nt, M * nt, nullptr, N.data(), u, n, mean + m * (size_t)n,
                          err ? err + m * (size_t)n : nullptr);
    return SQ_OK;
}

int sq_phi4_ens_pcorr_shape_info(const int dims[3], int out[6]) {
    int rc = ens_shape_dims(dims, out);
    if (rc) return rc;
    const sq::Phi4EnsShape s = sq::phi4_ens_shape(dims[0] * dims[1] * dims[2], dims[2]);
    if (!s.pc_ok) return fail(SQ_E_ARG, "the lattice shape leaves no LDS for the momentum projections (16 Lz bytes)");
    const int pl = sq::phi4_ens_pcorr_bytes(dims[2]);
    const sq::Phi4EnsLds st = s.lds(sq::kPhi4EnsLdsStep, pl), fr = s.lds(sq::kPhi4EnsLdsFrames, pl);
    out[0] = st.images;
    out[1] = st.bytes;
    out[2] = fr.images;
    out[3] = fr.bytes;
    out[4] = s.lds(sq::kPhi4EnsLdsStored, pl).bytes;
    out[5] = dims[2] / 2 + 1;
    return SQ_OK;
}

int sq_phi4_ens_corr_shape_info(const int dims[3], int out[6]) {
    int rc = ens_shape_dims(dims, out);
    if (rc) return rc;
    const sq::Phi4EnsShape s = sq::phi4_ens_shape(dims[0] * dims[1] * dims[2], dims[2]);
    const int sl = sq::phi4_ens_corr_bytes(dims[2]);
    const sq::Phi4EnsLds st = s.lds(sq::kPhi4EnsLdsStep, sl), fr = s.lds(sq::kPhi4EnsLdsFrames, sl);
    out[0] = st.images;
    out[1] = st.bytes;
    out[2] = fr.images;
    out[3] = fr.bytes;
    out[4] = s.lds(sq::kPhi4EnsLdsStored, sl).bytes;
    out[5] = dims[2] / 2 + 1;
    return SQ_OK;
}

}  // extern "C"
