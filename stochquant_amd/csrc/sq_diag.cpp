// sq_diag.cpp -- device self-tests and the copy-bandwidth probe of the C ABI:
// none of them takes a context.
#include <algorithm>
#include <cstring>

#include "sq_ctx.h"

using namespace sq;

extern "C" {

int sq_selftest_normals(int device, unsigned long long seed, unsigned int stream,
                        unsigned long long quad0, unsigned long long step, float *out, size_t nquads) {
    if (!out) return fail(SQ_E_ARG, "null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SQ_E_NODEV, "no HIP device");
    DeviceGuard g(device);
    float *d = nullptr;
    SQ_HIP(hipMalloc(&d, nquads * 4 * sizeof(float)));
    hipError_t e = sq::selftest_normals_launch(d, nquads, quad0, stream, step, (uint32_t)seed,
                                               (uint32_t)(seed >> 32), nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, d, nquads * 4 * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(SQ_E_HIP, hipGetErrorString(e));
    return SQ_OK;
}

int sq_selftest_dpp(int device, float *out64x2) {
    if (!out64x2) return fail(SQ_E_ARG, "null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SQ_E_NODEV, "no HIP device");
    DeviceGuard g(device);
    float *d = nullptr;
    SQ_HIP(hipMalloc(&d, 128 * sizeof(float)));
    hipError_t e = sq::selftest_dpp_launch(d, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out64x2, d, 128 * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(SQ_E_HIP, hipGetErrorString(e));
    return SQ_OK;
}

int sq_selftest_dpp_mix(int device, int mode, int blocks, int iters, unsigned int *errs64) {
    if (!errs64 || mode < 0 || mode > 3 || blocks < 1 || blocks > 65536 || iters < 1)
        return fail(SQ_E_ARG, "bad dpp_mix arguments");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SQ_E_NODEV, "no HIP device");
    DeviceGuard g(device);
    unsigned *d = nullptr;
    float *sink = nullptr;
    SQ_HIP(hipMalloc(&d, 64 * sizeof(unsigned)));
    hipError_t e = hipMalloc(&sink, 1024 * sizeof(float));
    if (e == hipSuccess) e = hipMemset(d, 0, 64 * sizeof(unsigned));
    if (e == hipSuccess) e = sq::selftest_dpp_mix_launch(mode, blocks, iters, d, sink, nullptr);
    if (e == hipSuccess) e = hipMemcpy(errs64, d, 64 * sizeof(unsigned), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    (void)hipFree(sink);
    if (e != hipSuccess) return fail(SQ_E_HIP, hipGetErrorString(e));
    return SQ_OK;
}

int sq_selftest_philox(int device, const unsigned int ctr[4], const unsigned int key[2],
                       unsigned int out[4]) {
    if (!ctr || !key || !out) return fail(SQ_E_ARG, "null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SQ_E_NODEV, "no HIP device");
    DeviceGuard g(device);
    uint32_t h[6] = {ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]};
    uint32_t *d = nullptr;
    SQ_HIP(hipMalloc(&d, 10 * sizeof(uint32_t)));
    hipError_t e = hipMemcpy(d, h, sizeof h, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = sq::selftest_philox_launch(d, d + 6, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, d + 6, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(SQ_E_HIP, hipGetErrorString(e));
    return SQ_OK;
}

int sq_selftest_libm(int device, int fn, const float *x, float *y, long long n) {
    if (!x || !y || n < 0 || fn < 0 || fn > 2) return fail(SQ_E_ARG, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SQ_E_NODEV, "no HIP device");
    if (n == 0) return SQ_OK;
    DeviceGuard g(device);
    float *d = nullptr;
    SQ_HIP(hipMalloc(&d, 2 * (size_t)n * sizeof(float)));
    hipError_t e = hipMemcpy(d, x, (size_t)n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = sq::selftest_libm_launch(fn, d, d + n, n, nullptr);
    if (e == hipSuccess) e = hipMemcpy(y, d + n, (size_t)n * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(SQ_E_HIP, hipGetErrorString(e));
    return SQ_OK;
}

int sq_selftest_bm_tables(int device, float *out) {
    if (!out) return fail(SQ_E_ARG, "null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SQ_E_NODEV, "no HIP device");
    DeviceGuard g(device);
    const size_t bytes = 4 * ((size_t)1 << 23) * sizeof(float);
    float *d = nullptr;
    SQ_HIP(hipMalloc(&d, bytes));
    hipError_t e = sq::selftest_bm_tables_launch(d, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(SQ_E_HIP, hipGetErrorString(e));
    return SQ_OK;
}

int sq_selftest_lcg(int device, unsigned long long seed, int N, int loops, unsigned int *w1,
                    unsigned int *w2, unsigned long long *seeds, double *xi, int generator) {
    if (!w1 || !w2 || !seeds || !xi || N < 1 || loops < 1) return fail(SQ_E_ARG, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SQ_E_NODEV, "no HIP device");
    DeviceGuard g(device);
    const long long n = (long long)(N + 1) * loops;
    char *d = nullptr;
    SQ_HIP(hipMalloc(&d, (size_t)n * 24 + 8 * sq::kLcgScratch));
    uint32_t *dw1 = (uint32_t *)d, *dw2 = dw1 + n;
    unsigned long long *ds = (unsigned long long *)(dw2 + n);
    double *dx = (double *)(ds + n);
    unsigned long long *scr = generator == 1 ? (unsigned long long *)(dx + n) : nullptr;
    hipError_t e = sq::qm1d_gs_lcg_launch(seed, N, n, dw1, dw2, ds, dx, scr, nullptr);
    if (e == hipSuccess) e = hipMemcpy(w1, dw1, n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(w2, dw2, n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(seeds, ds, n * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(xi, dx, n * 8, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(SQ_E_HIP, hipGetErrorString(e));
    return SQ_OK;
}

int sq_copy_bandwidth(int device, size_t bytes, int iters, double *gbps) {
    if (!gbps || iters < 1 || bytes < 1024) return fail(SQ_E_ARG, "bad argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(SQ_E_NODEV, "no HIP device");
    DeviceGuard g(device);
    const size_t n4 = bytes / 16;
    float4 *a = nullptr, *b = nullptr;
    SQ_HIP(hipMalloc(&a, n4 * 16));
    SQ_HIP(hipMalloc(&b, n4 * 16));
    SQ_HIP(hipMemset(a, 0, n4 * 16));
    hipEvent_t e0, e1;
    SQ_HIP(hipEventCreate(&e0));
    SQ_HIP(hipEventCreate(&e1));
    double best = 0;
    for (int nt = 0; nt < 2; ++nt) {
        SQ_HIP(sq::copy_launch(a, b, n4, nt != 0, nullptr));
        SQ_HIP(hipEventRecord(e0, nullptr));
        for (int i = 0; i < iters; ++i)
            SQ_HIP(sq::copy_launch((i & 1) ? b : a, (i & 1) ? a : b, n4, nt != 0, nullptr));
        SQ_HIP(hipEventRecord(e1, nullptr));
        SQ_HIP(hipEventSynchronize(e1));
        float ms = 0;
        SQ_HIP(hipEventElapsedTime(&ms, e0, e1));
        best = std::max(best, 2.0 * (double)n4 * 16.0 * iters / (ms * 1e-3) / 1e9);
    }
    *gbps = best;
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(a);
    (void)hipFree(b);
    return SQ_OK;
}

}  // extern "C"
