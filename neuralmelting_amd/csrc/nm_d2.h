// nm_d2.h — the squared distance of the cluster stage, for DBSCAN's scans (nm_cluster.h) and for k-means (nm_kmeans.h), which is
// built into another object: d = a[c] - b[c], acc = fma(d, d, acc), c ascending, the first square a plain product.  The error
// bound and the symmetry are derived in nm_cluster.h.
#pragma once
#include <hip/hip_runtime.h>

namespace nm {

// the squared distance of the header, in the one order that every pass uses
template <int ND> __device__ __forceinline__ double cl_d2(const double *a, const double *b)
{
    double d = a[0] - b[0];
    double acc = d * d;
#pragma unroll
    for (int c = 1; c < ND; ++c) {
        d = a[c] - b[c];
        acc = __builtin_fma(d, d, acc);
    }
    return acc;
}

} // namespace nm
