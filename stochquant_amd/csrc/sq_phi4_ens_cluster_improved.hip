// sq_phi4_ens_cluster_improved.hip -- the Swendsen-Wang sweep of sq_phi4_ens_cluster.hip with the cluster sums
// of the improved estimators (include/stochquant.h): the second kind of instance of that file's
// kernel template, phi4_ens_cluster_kernel<K, Phi4EnsClusterSumArgs>, in a translation unit of its own.  The
// kernel's comment in sq_phi4_ens_cluster.hip describes the limb passes.
#define SQ_PHI4_ENS_CLUSTER_KERNEL_ONLY
#include "sq_phi4_ens_cluster.hip"

namespace sq {

Phi4EnsClusterSumShape phi4_ens_cluster_sum_shape(int sites) {
    const Phi4EnsShape sh = phi4_ens_shape(sites);
    Phi4EnsClusterSumShape s;
    s.K = sh.K;
    s.T = sh.T;
    s.lds_bytes = sh.mom_lds_bytes + 4 * 8;  // the per-weight totals behind the scratch
    s.park = sh.K == 8 ? 1 : 0;  // the kernel's PARK
    return s;
}

hipError_t phi4_ens_cluster_improved_launch(const Phi4EnsArgs &a, const Phi4EnsClusterArgs &w,
                                            const Phi4EnsClusterSumArgs &x, int nrep, hipStream_t s) {
    if (!ens_shape_ok(a) || nrep < 1 || w.stat == nullptr || x.series == nullptr || x.tab == nullptr)
        return hipErrorInvalidValue;
    const Phi4EnsClusterSumShape sh = phi4_ens_cluster_sum_shape(a.Lx * a.Ly * a.Lz);
    if (sh.park && x.park == nullptr) return hipErrorInvalidValue;
    Phi4EnsArgs q = a;
    Phi4EnsClusterArgs wq = w;
    Phi4EnsClusterSumArgs xq = x;
    void *args[] = {&q, &wq, &xq};
    const void *fn = sh.K == 1   ? (const void *)&phi4_ens_cluster_kernel<1, Phi4EnsClusterSumArgs>
                     : sh.K == 2 ? (const void *)&phi4_ens_cluster_kernel<2, Phi4EnsClusterSumArgs>
                     : sh.K == 4 ? (const void *)&phi4_ens_cluster_kernel<4, Phi4EnsClusterSumArgs>
                                 : (const void *)&phi4_ens_cluster_kernel<8, Phi4EnsClusterSumArgs>;
    hipError_t e = ens_lds_attr(fn, sh.lds_bytes);
    if (e != hipSuccess) return e;
    return hipLaunchKernel(fn, dim3((unsigned)nrep), dim3((unsigned)sh.T), args, (size_t)sh.lds_bytes, s);
}

}  // namespace sq
