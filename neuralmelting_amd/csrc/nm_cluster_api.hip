// nm_cluster_api.hip — the cluster stage (include/nm_cluster.h; kernels: nm_cluster.h): the screen, the three scans and the
// numbering of the roots on the host between the union and the border pass.
#include "../../include/nm_cluster.h"
#include "nm_cluster.h"
#include "nm_host.h"

#include <cmath>
#include <vector>

using namespace nm;

namespace {
thread_local std::string g_cluster_error;
std::string &stage_error() { return g_cluster_error; }

// the slots of nm_cluster_last_timing
enum { CL_T_UPLOAD, CL_T_DEGREE, CL_T_UNION, CL_T_NUMBER, CL_T_BORDER, CL_T_COUNT };
thread_local double g_cluster_ms[CL_T_COUNT];

// the three scans for one ndim (the union pass's workgroups are of unequal length: scan_grid's many short ones suit it)
struct Scans {
    void (*degree)(int, const double *, double, int *);
    void (*unite)(int, const double *, double, int, const int *, int *);
    void (*border)(int, const double *, double, const int *, const int *, int, int *);
};
const auto SCANS = scan_table<CL_MAXDIM>([](auto nd) {
    constexpr int ND = decltype(nd)::value;
    return Scans{nm_cluster_degree_kernel<ND>, nm_cluster_union_kernel<ND>, nm_cluster_border_kernel<ND>};
});
} // namespace

extern "C" {
const char *nm_cluster_last_error(void) { return g_cluster_error.c_str(); }

int nm_cluster_last_timing(double *ms) { return last_timing("nm_cluster_last_timing", g_cluster_ms, ms); }

int nm_cluster_dbscan(int device, int64_t npoints, int ndim, const double *x, double eps, int min_pts, int32_t *label, int32_t *degree,
                      int32_t *nclusters)
{
    static const char *const fn = "nm_cluster_dbscan";
    if (npoints < 1 || npoints > CL_MAXN) return refuse(fn, "npoints must lie in 1..2^21");
    if (ndim < 1 || ndim > CL_MAXDIM) return refuse(fn, "ndim must lie in 1..16");
    if (!std::isfinite(eps) || !(eps > 0.0)) return refuse(fn, "eps must be finite and positive");
    if (min_pts < 1) return refuse(fn, "min_pts must be at least 1");
    if (!x || !label || !degree || !nclusters) return refuse(fn, "a needed pointer is null");
    if (const int rc = stage_device(fn, device)) return rc;
    const int n = (int)npoints;
    const double e2 = eps * eps;                                // rounded once, here
    const Scans &k = SCANS[ndim - 1];
    const dim3 grid = scan_grid<ClScan>(n, n), flat((unsigned)((n + CL_BLOCK - 1) / CL_BLOCK));
    Laps<CL_T_COUNT> laps;
    DevBuf<double> d_x;
    DevBuf<int> d_parent, d_degree, d_root, d_cnum, d_blab;     // d_root holds the roots, then the list of the points that are not core
    laps.lap(CL_T_UPLOAD);
    STAGE_CHK(fn, d_x.upload(x, (size_t)n * ndim));
    STAGE_CHK(fn, d_parent.alloc(n));
    STAGE_CHK(fn, d_degree.alloc(n));
    STAGE_CHK(fn, d_root.alloc(n));
    STAGE_CHK(fn, d_cnum.alloc(n));
    STAGE_CHK(fn, d_blab.alloc(n));
    STAGE_CHK(fn, hipMemset(d_blab, 0x7f, (size_t)n * sizeof(int)));        // CL_NONE
    int first = -1;
    STAGE_CHK(fn, scan_screen<ClScan>(n, ndim, d_x, first));
    if (first >= 0) return fail(NM_ERR_ARG, std::string(fn) + ": x is not finite in point " + std::to_string(first));
    hipLaunchKernelGGL(nm_cluster_init_kernel, flat, dim3(CL_BLOCK), 0, 0, n, d_parent, d_degree);
    STAGE_CHK(fn, hipGetLastError());
    laps.lap(CL_T_UPLOAD);
    hipLaunchKernelGGL(k.degree, grid, dim3(CL_BLOCK), 0, 0, n, d_x, e2, d_degree);
    STAGE_CHK(fn, hipGetLastError());
    laps.lap(CL_T_DEGREE);
    hipLaunchKernelGGL(k.unite, grid, dim3(CL_BLOCK), 0, 0, n, d_x, e2, min_pts, d_degree, d_parent);
    hipLaunchKernelGGL(nm_cluster_flatten_kernel, flat, dim3(CL_BLOCK), 0, 0, n, min_pts, d_degree, d_parent, d_root);
    STAGE_CHK(fn, hipGetLastError());
    laps.lap(CL_T_UNION);
    // the numbering: a root is the smallest index of its component, so in index order every root is numbered before its members;
    // the points that are not core are listed (over their roots: i is read before open[nopen <= i] is written)
    std::vector<int> root((size_t)n), cnum((size_t)n);
    STAGE_CHK(fn, d_root.download(root.data(), n));
    int count = 0, nopen = 0;
    for (int i = 0; i < n; ++i) {
        cnum[i] = root[i] < 0 ? CL_NONE : root[i] == i ? count++ : cnum[root[i]];
        if (cnum[i] == CL_NONE) root[nopen++] = i;
    }
    STAGE_CHK(fn, hipMemcpy(d_cnum, cnum.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    if (nopen) STAGE_CHK(fn, hipMemcpy(d_root, root.data(), (size_t)nopen * sizeof(int), hipMemcpyHostToDevice));
    laps.lap(CL_T_NUMBER);
    if (nopen && count) {                                       // without a cluster every point that is not core is noise
        hipLaunchKernelGGL(k.border, scan_grid<ClScan>(nopen, n), dim3(CL_BLOCK), 0, 0, n, d_x, e2, d_cnum, d_root, nopen, d_blab);
        STAGE_CHK(fn, hipGetLastError());
    }
    laps.lap(CL_T_BORDER);
    STAGE_CHK(fn, hipDeviceSynchronize());
    laps.book(g_cluster_ms);
    STAGE_CHK(fn, d_blab.download(root.data(), n));             // the borders' numbers, in the buffer the roots have left
    STAGE_CHK(fn, d_degree.download(degree, n));
    for (int i = 0; i < n; ++i) label[i] = cnum[i] != CL_NONE ? cnum[i] : root[i] != CL_NONE ? root[i] : -1;
    *nclusters = count;
    return NM_OK;
}
} // extern "C"
