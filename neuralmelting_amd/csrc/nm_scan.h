// nm_scan.h — what the all-pairs scans of the cluster and the manifold stage share (nm_cluster.h, nm_tsne.h): the one description
// of their skeleton, its row loader and its screen for values that are not finite on the device, its grid and the tables of its
// instantiations on the host.
//
// The skeleton.  A workgroup of S::BLOCK threads owns S::ROWS = S::RPT S::BLOCK rows: thread t keeps the coordinates of rows
// r0 + t, r0 + S::BLOCK + t, ... in registers (the number of coordinates is a template parameter).  The columns are walked in tiles
// of S::TILE points: a tile is one contiguous piece of x and is copied into LDS as it lies between two barriers.  Every thread
// then reads the same column at the same time (a broadcast read of LDS, free of bank conflicts) and meets it with each of its
// rows, so a column's LDS read is paid once per S::RPT pairs.  The grid is (row blocks) x (column slices): slice s of S walks the
// tiles s, s + S, s + 2 S, ... so a small N still fills the device and a triangular range stays balanced.  A tile's last column
// comes from the loop bound, which is the same in every thread: no test per pair.  A row past the end is point 0 again.
//
// The tile loop itself stands in each stage's header (cl_scan, ts_scan), a dozen lines beside what a pair computes.  One loop here
// that took the stage's part as a functor was built and did not compile to the same machine code: on the MI355X it ran the union
// pass 2.5 % faster and the degree pass (ndim 2) 1.1 % and the gather pass 1.9 % slower than the loops as they stand
// (profiles/r28_scan_ab.txt).  There is no floating-point arithmetic in this file: where it is included changes no bit.
#pragma once
#include <hip/hip_runtime.h>

#include "nm_own.h"

#include <array>
#include <cstddef>
#include <type_traits>
#include <utility>

namespace nm {

// the shape of a stage's scans: threads of a workgroup, rows of a thread, columns of a tile; for the host the workgroups a scan
// aims at at least and the tiles a workgroup walks at most
template <int BLOCK_, int RPT_, int TILE_, int GRID_, int SPAN_> struct ScanShape {
    static constexpr int BLOCK = BLOCK_, RPT = RPT_, ROWS = RPT_ * BLOCK_, TILE = TILE_, GRID = GRID_, SPAN = SPAN_;
};

// the rows of thread tid of row block rb: their indices, whether they exist, and their coordinates (of point 0 where they do not).
// The rows are 0 .. nrows - 1 themselves, or, with a list, the points list[0 .. nrows - 1].
template <class S, int ND>
__device__ __forceinline__ void scan_rows(const double *__restrict__ x, const int *__restrict__ list, int nrows, int rb, int (&idx)[S::RPT],
                                          bool (&valid)[S::RPT], double (&row)[S::RPT][ND])
{
#pragma unroll
    for (int r = 0; r < S::RPT; ++r) {
        const int k = rb * S::ROWS + r * S::BLOCK + (int)threadIdx.x;
        valid[r] = k < nrows;
        idx[r] = !valid[r] ? 0 : list ? list[k] : k;
        const double *src = x + (size_t)idx[r] * ND;
#pragma unroll
        for (int c = 0; c < ND; ++c) row[r][c] = src[c];
    }
}

// one thread per point: the first point with a value that is not finite (integer atomicMin on *bad)
template <class S> __global__ void __launch_bounds__(S::BLOCK) nm_scan_screen_kernel(int n, int ndim, const double *__restrict__ x, int *bad)
{
    const int i = blockIdx.x * S::BLOCK + threadIdx.x;
    if (i >= n) return;
    bool ok = true;
    for (int c = 0; c < ndim; ++c) ok = ok && isfinite(x[(size_t)i * ndim + c]);
    if (!ok) atomicMin(bad, i);
}

// ---- the host side

// the grid of a scan of nrows rows over n columns: every row block, and as many column slices as bring it to S::GRID workgroups
// and leave a workgroup at most S::SPAN tiles (at most one slice per tile).  Many short workgroups, not one resident set of long
// ones: the device hands out the next as one ends.  A function of its arguments alone: so is the order of every sum over slices.
template <class S> dim3 scan_grid(int nrows, int n)
{
    const int blocks = (nrows + S::ROWS - 1) / S::ROWS, tiles = (n + S::TILE - 1) / S::TILE;
    int slices = (S::GRID + blocks - 1) / blocks;
    if (slices < (tiles + S::SPAN - 1) / S::SPAN) slices = (tiles + S::SPAN - 1) / S::SPAN;
    if (slices > tiles) slices = tiles;
    return dim3((unsigned)blocks, (unsigned)slices);
}

// {of(1), ..., of(N)}, the argument a std::integral_constant: a stage's kernels for every number of coordinates, which is a
// template parameter because the coordinates live in registers
template <class Of, int... I> auto scan_table(Of of, std::integer_sequence<int, I...>)
{
    return std::array<decltype(of(std::integral_constant<int, 1>{})), sizeof...(I)>{of(std::integral_constant<int, I + 1>{})...};
}
template <int N, class Of> auto scan_table(Of of) { return scan_table(of, std::make_integer_sequence<int, N>{}); }

// first = the first point of x[n][ndim] on the device that holds a value that is not finite, or -1
template <class S> hipError_t scan_screen(int n, int ndim, const double *d_x, int &first)
{
    const int none = 0x7fffffff;
    DevBuf<int> d_bad;
    hipError_t e = d_bad.upload(&none, 1);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(nm_scan_screen_kernel<S>, dim3((unsigned)((n + S::BLOCK - 1) / S::BLOCK)), dim3(S::BLOCK), 0, 0, n, ndim, d_x, d_bad.p);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    e = d_bad.download(&first, 1);
    if (first == none) first = -1;
    return e;
}

} // namespace nm
