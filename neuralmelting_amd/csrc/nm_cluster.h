// nm_cluster.h — the kernels of the cluster stage (include/nm_cluster.h: the definitions): DBSCAN of N points x[n][c], float64,
// row-major, as three all-pairs scans over one skeleton and two small kernels around them.  No N x N array exists: the device
// holds x (N ndim doubles) and five int arrays of N.
//
// The skeleton is described in nm_scan.h, which holds its row loader, grid and screen; the shape here is ClScan: CL_ROWS = CL_RPT
// CL_BLOCK rows of a workgroup in registers, tiles of CL_TILE columns in LDS, a grid of (row blocks) x (column slices).  The tile
// loop (cl_scan) stands here, with what is this stage's own: one int per column that the pass defines, a wave without a row at work
// walks the barriers only, a column whose int says so is skipped by the whole workgroup, and a pass hears of the columns within eps2
// of a row.  A row past the end is given eps2 = -1, which no distance meets.
//
// cl_d2 is the one distance: d = a[c] - b[c], acc = fma(d, d, acc), c ascending, the first square a plain product.  Negating every
// d changes no bit, so d2(i, j) == d2(j, i); a pair gets the same bits in every pass.  A difference rounds once, so its square
// carries two roundings; the first product rounds once more and then passes through the ndim - 1 fused multiply-adds, one
// rounding each, and no other term passes through more: the error is at most (ndim + 2) u d2, the header's bound.
//
//   nm_cluster_init_kernel    behind nm_scan.h's screen for values that are not finite, one thread per point: parent[i] = i,
//                             degree[i] = 0.
//   nm_cluster_degree_kernel  the scan over all tiles: a row counts the columns within eps2 (itself among them); the slices are
//                             joined by integer atomicAdd on degree[i].
//   nm_cluster_union_kernel   the scan over the tiles up to the block's own last row (an edge is united from its larger end; in
//                             the block's diagonal tiles from both, which changes nothing).  The tile's int is a snapshot of
//                             parent[j], or -1 where j is not core; a column that is not core is skipped by the whole workgroup.
//                             A core row keeps the last root it found for itself; where a neighbour's snapshot equals it the two
//                             are known to share a set (sets only grow, and the cached root was an ancestor of the row when it was
//                             read), and nothing is done.  Else the real find and union run on the global array, and the row
//                             caches what they return.  A stale snapshot or a stale cached root only costs a union that finds both
//                             ends under one root.  A wave without a core row walks the barriers only; a block without one leaves.
//   nm_cluster_flatten_kernel behind the kernel boundary: root[i] = the root of core point i, -1 for the others.
//   (host)                    the roots are numbered in ascending order: root[i] <= i, so one pass in index order, which also lists
//                             the points that are not core.
//   nm_cluster_border_kernel  the scan over all tiles with that list as its rows, so its work is (points that are not core) x N and
//                             nothing where every point is core: the tile's int is the cluster number of a core column, CL_NONE for
//                             the others (skipped by the whole workgroup); a row keeps the minimum over its neighbours, the slices
//                             are joined by integer atomicMin.
//
// The union-find is nm_distr.h's (nm_solid_union_kernel), on one array for all N points.  Lock-free, no thread ever waits for
// another: no spin loop, no polled flag, no cooperative launch.  Invariants of parent[]:
//   (1) parent[x] <= x always: it starts as x, and every write stores a smaller value;
//   (2) every write lowers a value: a hook is atomicCAS(parent[r], r, smaller root), a compression is atomicMin(parent[x],
//       grandparent); so a value read earlier is still an ancestor, and a root (parent[r] == r) is never written by a compression;
//   (3) the atomicCAS of a hook fails only if r is no longer a root, which only another hook's success can cause: the array sees at
//       most N - 1 successful hooks, so all threads together retry at most that often per root they aimed at;
//   (4) a find terminates: along parent[] the indices decrease strictly until a root, at most N - 1 steps.
// The smaller root always wins, so the root of a finished component is its smallest index, whatever the order of execution: the
// flattened roots, and with them every output, are a property of the input alone.  Reads of parent[] that race with other
// workgroups are relaxed atomic loads at agent scope (they pass the caches that are not coherent across the device); the flatten
// kernel runs behind a kernel boundary and reads plainly.  Integer atomics only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nm_d2.h"
#include "nm_scan.h"

namespace nm {

constexpr int CL_BLOCK = 256;                       // threads of a workgroup
constexpr int CL_RPT = 2;                           // rows of a thread
constexpr int CL_ROWS = CL_RPT * CL_BLOCK;          // rows of a workgroup
constexpr int CL_TILE = 256;                        // columns staged in LDS at a time: 32 KiB of coordinates at ndim = 16
constexpr int CL_MAXDIM = 16;
constexpr int64_t CL_MAXN = (int64_t)1 << 21;
constexpr int CL_NONE = 0x7f7f7f7f;                 // no cluster (yet): the byte pattern that hipMemset writes
constexpr int CL_GRID = 2048;                       // workgroups a scan aims at at least: 8 per compute unit
constexpr int CL_SPAN = 128;                        // tiles a workgroup walks at most

using ClScan = ScanShape<CL_BLOCK, CL_RPT, CL_TILE, CL_GRID, CL_SPAN>;
static_assert(CL_TILE <= CL_BLOCK, "a tile's ints are staged by one thread each");

// (cl_d2, the squared distance of the header in the one order that every pass uses, stands in nm_d2.h: k-means shares it)

__device__ __forceinline__ int cl_peek(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x, halving the path on the way (invariants 2 and 4)
__device__ __forceinline__ int cl_find(int *parent, int x)
{
    for (;;) {
        const int p = cl_peek(parent + x);
        if (p == x) return x;
        const int g = cl_peek(parent + p);
        if (g < p) atomicMin(parent + x, g);
        x = g;
    }
}

// unites the sets of x and y and returns their common root as of that moment: the larger of the two roots is hooked under the
// smaller with one atomicCAS.  A failure means that the larger one has been hooked by someone else (invariant 3): find again
// from where we are, nothing to wait for.
__device__ __forceinline__ int cl_unite(int *parent, int x, int y)
{
    for (;;) {
        x = cl_find(parent, x);
        y = cl_find(parent, y);
        if (x == y) return x;
        const int hi = x > y ? x : y, lo = x > y ? y : x;
        if (atomicCAS(parent + hi, hi, lo) == hi) return lo;
        x = hi; y = lo;
    }
}

__global__ void __launch_bounds__(CL_BLOCK) nm_cluster_init_kernel(int n, int *__restrict__ parent, int *__restrict__ degree)
{
    const int i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n) return;
    parent[i] = i;
    degree[i] = 0;
}

// The tile loop.  stage(j) is the tile's int of column j (called by one thread per column); skip(v) says that a column with the
// int v concerns no row (the same answer in every thread); hit(r, j, v) is called for row slot r where column j lies within
// eps2[r].  `busy` is the wave's: a wave with nothing to do stages and walks the barriers only.  Tiles t0, t0 + tstep, ... < tend.
template <int ND, class Stage, class Skip, class Hit>
__device__ __forceinline__ void cl_scan(int n, const double *__restrict__ x, const double (&row)[CL_RPT][ND], const double (&eps2)[CL_RPT],
                                        bool busy, int t0, int tstep, int tend, Stage stage, Skip skip, Hit hit)
{
    __shared__ __align__(16) double sx[CL_TILE * ND];
    __shared__ int sv[CL_TILE];
    const int tid = threadIdx.x;
    for (int t = t0; t < tend; t += tstep) {
        const int j0 = t * CL_TILE, cnt = n - j0 < CL_TILE ? n - j0 : CL_TILE;
        __syncthreads();                                        // the tile before has been read by every wave
        const double *src = x + (size_t)j0 * ND;
        for (int k = tid; k < cnt * ND; k += CL_BLOCK) sx[k] = src[k];
        if (tid < cnt) sv[tid] = stage(j0 + tid);
        __syncthreads();
        if (!busy) continue;                                    // wave-uniform
        for (int jj = 0; jj < cnt; ++jj) {
            const int v = sv[jj];
            if (skip(v)) continue;                              // the same in every thread
            double col[ND];
#pragma unroll
            for (int c = 0; c < ND; ++c) col[c] = sx[jj * ND + c];
#pragma unroll
            for (int r = 0; r < CL_RPT; ++r)
                if (cl_d2<ND>(row[r], col) <= eps2[r]) hit(r, j0 + jj, v);
        }
    }
}

template <int ND> __global__ void __launch_bounds__(CL_BLOCK)
nm_cluster_degree_kernel(int n, const double *__restrict__ x, double e2, int *degree)
{
    int idx[CL_RPT], count[CL_RPT];
    bool valid[CL_RPT];
    double row[CL_RPT][ND], eps2[CL_RPT];
    scan_rows<ClScan, ND>(x, nullptr, n, blockIdx.x, idx, valid, row);
#pragma unroll
    for (int r = 0; r < CL_RPT; ++r) { eps2[r] = valid[r] ? e2 : -1.0; count[r] = 0; }
    const int ntiles = (n + CL_TILE - 1) / CL_TILE;
    cl_scan<ND>(n, x, row, eps2, true, blockIdx.y, gridDim.y, ntiles, [](int) { return 0; }, [](int) { return false; },
                [&](int r, int, int) { ++count[r]; });
#pragma unroll
    for (int r = 0; r < CL_RPT; ++r)
        if (valid[r] && count[r]) atomicAdd(degree + idx[r], count[r]);
}

template <int ND> __global__ void __launch_bounds__(CL_BLOCK)
nm_cluster_union_kernel(int n, const double *__restrict__ x, double e2, int min_pts, const int *__restrict__ degree, int *parent)
{
    int idx[CL_RPT], root[CL_RPT];
    bool valid[CL_RPT];
    double row[CL_RPT][ND], eps2[CL_RPT];
    const int rb = gridDim.x - 1 - blockIdx.x;                  // the last row block has the most tiles: it starts first
    scan_rows<ClScan, ND>(x, nullptr, n, rb, idx, valid, row);
    bool any = false;
#pragma unroll
    for (int r = 0; r < CL_RPT; ++r) {
        const bool core = valid[r] && degree[idx[r]] >= min_pts;
        eps2[r] = core ? e2 : -1.0;
        root[r] = idx[r];
        any = any || core;
    }
    if (!__syncthreads_or(any)) return;                         // the same answer in every thread
    const bool busy = __any(any);
    const int last = (rb + 1) * CL_ROWS < n ? (rb + 1) * CL_ROWS : n;       // one past the block's last row
    cl_scan<ND>(n, x, row, eps2, busy, blockIdx.y, gridDim.y, (last + CL_TILE - 1) / CL_TILE,
                [&](int j) { return degree[j] >= min_pts ? cl_peek(parent + j) : -1; }, [](int v) { return v < 0; },
                [&](int r, int j, int v) { if (v != root[r]) root[r] = cl_unite(parent, idx[r], j); });
}

__global__ void __launch_bounds__(CL_BLOCK)
nm_cluster_flatten_kernel(int n, int min_pts, const int *__restrict__ degree, const int *__restrict__ parent, int *__restrict__ root)
{
    const int i = blockIdx.x * CL_BLOCK + threadIdx.x;
    if (i >= n) return;
    int r = -1;
    if (degree[i] >= min_pts) {
        r = i;
        for (int p = parent[r]; p != r; p = parent[r]) r = p;   // invariant 4
    }
    root[i] = r;
}

template <int ND> __global__ void __launch_bounds__(CL_BLOCK)
nm_cluster_border_kernel(int n, const double *__restrict__ x, double e2, const int *__restrict__ cnum, const int *__restrict__ open, int nopen,
                         int *blab)
{
    int idx[CL_RPT], best[CL_RPT];
    bool valid[CL_RPT];
    double row[CL_RPT][ND], eps2[CL_RPT];
    scan_rows<ClScan, ND>(x, open, nopen, blockIdx.x, idx, valid, row);
#pragma unroll
    for (int r = 0; r < CL_RPT; ++r) {
        eps2[r] = valid[r] ? e2 : -1.0;
        best[r] = CL_NONE;
    }
    const bool busy = __any(valid[0]);                          // the second row of a thread lies behind the first
    const int ntiles = (n + CL_TILE - 1) / CL_TILE;
    cl_scan<ND>(n, x, row, eps2, busy, blockIdx.y, gridDim.y, ntiles, [&](int j) { return cnum[j]; }, [](int v) { return v == CL_NONE; },
                [&](int r, int, int v) { best[r] = v < best[r] ? v : best[r]; });
#pragma unroll
    for (int r = 0; r < CL_RPT; ++r)
        if (best[r] != CL_NONE) atomicMin(blab + idx[r], best[r]);
}

} // namespace nm
