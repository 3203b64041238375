// sq_phi4_ens_cluster_improved.hip -- the Swendsen-Wang sweep of sq_phi4_ens_cluster.hip with the cluster sums
// of the improved estimators (include/stochquant.h): the second kind of instance of the kernel
// template of sq_phi4_ens_cluster_dev.h, phi4_ens_cluster_kernel<K, Phi4EnsClusterSumArgs>, in a translation unit
// of its own.  The kernel's comment there describes the limb passes.
#include "sq_phi4_ens_cluster_dev.h"
#include "sq_phi4_ens_launch.h"

namespace sq {

Phi4EnsClusterSumShape phi4_ens_cluster_sum_shape(int sites) {
    Phi4EnsClusterSumShape s{phi4_ens_shape(sites), 0};
    s.park = s.K == 8 ? 1 : 0;  // the kernel's PARK
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
    return ens_launch(SQ_ENS_KERNEL(sh.K, phi4_ens_cluster_kernel, Phi4EnsClusterSumArgs), nrep, sh.T,
                      sh.lds(kPhi4EnsLdsStored, kPhi4EnsClusterSumBytes).bytes, args, s);
}

}  // namespace sq
