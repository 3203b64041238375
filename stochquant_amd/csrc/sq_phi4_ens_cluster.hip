// sq_phi4_ens_cluster.hip -- Swendsen-Wang cluster sweeps of the embedded Ising
// signs of the phi^4 lattice ensemble: the plain instances of
// phi4_ens_cluster_kernel, whose comment in sq_phi4_ens_cluster_dev.h describes
// the sweep, and their launcher.
#include "sq_phi4_ens_cluster_dev.h"
#include "sq_phi4_ens_launch.h"

namespace sq {

hipError_t phi4_ens_cluster_launch(const Phi4EnsArgs &a, const Phi4EnsClusterArgs &w, int nrep, hipStream_t s) {
    if (!ens_shape_ok(a) || nrep < 1 || w.stat == nullptr) return hipErrorInvalidValue;
    const Phi4EnsShape sh = phi4_ens_shape(a.Lx * a.Ly * a.Lz);
    Phi4EnsArgs q = a;
    Phi4EnsClusterArgs wq = w;
    void *args[] = {&q, &wq};
    return ens_launch(SQ_ENS_KERNEL(sh.K, phi4_ens_cluster_kernel), nrep, sh.T, sh.lds(kPhi4EnsLdsStored).bytes, args,
                      s);
}

}  // namespace sq
