// nm_spectral.h — the kernels of spectral clustering's embedding (include/nm_distr.h, nm_cluster_spectral: the definitions and the
// method; the entry point stands in nm_distr_api.hip, the distance is nm_d2.h's, which DBSCAN and k-means share).  The affinity
// A(i, j) = exp(-gamma d2(i, j)) is never stored: every application of it is one all-pairs pass on nm_scan.h's skeleton.  The
// device holds x (N ndim doubles), deg and deg^-1/2 (N doubles each), three arrays of N x W doubles (W the padded width of the
// block, below) and the partial sums of a pass (slices x N x W doubles, at most 1 GiB: SP_SPAN).
//
// The width.  A block of nblock columns is kept at W = 1 (nblock 1), 8 (nblock 2..8) or 16 (nblock 9..16) doubles a row, the
// columns past nblock zero: they stay zero through every kernel here (a product with zero, a sum of zeros) and cost arithmetic,
// not correctness.  16 ndim x 3 widths = 48 instantiations of the pass.
//
//   nm_spectral_pass_kernel    the pass t_i[c] = sum_{j != i} exp(-(gamma d2(i, j))) u_j[c], c < W.  SP_ROWS = SP_RPT SP_BLOCK rows
//                              of a workgroup in registers (scan_rows), tiles of SP_TILE columns in LDS: their coordinates and
//                              their W values of u, read as broadcasts.  The grid is (row blocks) x (column slices); slice s
//                              walks the tiles s, s + S, ... and stores its rows' partial sums, nothing is added across
//                              workgroups.  Only the tiles that hold the block's own rows test j != i.  u == null stands for
//                              u = 1: with W = 1 that is the degree.  The product gamma d2 rounds once, exp is the device
//                              library's, a term enters its sum by one fused multiply-add.
//   nm_spectral_degree_kernel  joins the slices of the degree pass in ascending order: deg[i], rs[i] = 1 / sqrt(deg[i]), and the
//                              first point whose degree is not positive (integer atomicMin, as nm_scan_screen_kernel).
//   nm_spectral_rows_kernel    per element of the block: joins the slices in ascending order, applies the outer deg^-1/2 and the
//                              recurrence's scalars: dst = alpha y + (beta cur + gam dst), y = rs[i] t; writes the next pass's
//                              u = rs[i] dst beside it.  alpha 1, beta 0, gam 0 is the plain application of M.
//   nm_spectral_axpby_kernel   the filter's first term, which needs no pass: b = alpha b + beta a, u = rs b.
//   nm_spectral_resid_kernel   r = w - theta[c] v, one fused multiply-add per element.
//   nm_spectral_gram_kernel    the block reductions A^T B, W^2 sums: the points are cut into chunks of SP_CHUNK = 4096; lane p of a
//                              wave adds the chunk's points p, p + 64, p + 128, ... in ascending order from +0, the 64 lanes are
//                              added by km_tree (lane 2 p with lane 2 p + 1, level by level); wave w takes the rows w, w + 4, ... of
//                              the result.  nm_spectral_gram_join_kernel adds the chunks in ascending order.
//   nm_spectral_apply_kernel   dst = src C, C (W x W) in LDS, a thread per point: out[c] = sum_k src[k] C[k][c], k ascending, the
//                              first a plain product and every further one a fused multiply-add; u = rs dst beside it if wanted.
//
// Nothing waits for anything inside a launch: no spin loop, no polled flag, no cooperative launch.  The only atomic is an integer
// atomicMin.  No sum depends on the schedule: slices, lanes, trees and chunks are fixed by the indices alone (scan_grid is a
// function of N alone), so a call returns the same bytes every time and on every device.
//
// Resources (make resources, gfx950): DESIGN.md §9 row f-12 lists the pass's registers; it has no scratch at any ndim and width.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nm_d2.h"
#include "nm_kmeans.h"
#include "nm_scan.h"

#include <type_traits>

namespace nm {

constexpr int SP_BLOCK = 256;                       // threads of a workgroup
constexpr int SP_RPT = 2;                           // rows of a thread
constexpr int SP_ROWS = SP_RPT * SP_BLOCK;          // rows of a workgroup of the pass
constexpr int SP_TILE = 128;                        // columns staged in LDS at a time: 32 KiB at ndim = 16 and width 16
constexpr int SP_GRID = 2048;                       // workgroups a pass aims at at least: 8 per compute unit
constexpr int SP_SPAN = 1024;                       // tiles a workgroup walks at most: 8 slices at 2^20 points, 1 GiB of partial sums at width 16
constexpr int SP_CHUNK = 4096;                      // points of a workgroup of the reductions: 64 lanes of 64 points
constexpr int SP_MAXDIM = 16;
constexpr int SP_MAXCOMP = 8;
constexpr int SP_MAXBLOCK = 16;
constexpr int64_t SP_MAXN = (int64_t)1 << 20;

using SpScan = ScanShape<SP_BLOCK, SP_RPT, SP_TILE, SP_GRID, SP_SPAN>;
static_assert(SP_TILE <= SP_BLOCK && SP_ROWS % SP_TILE == 0, "the tiles of a block's own rows are whole tiles");
static_assert((SP_MAXN / SP_TILE / SP_SPAN) * SP_MAXN * SP_MAXBLOCK * 8 < ((int64_t)2 << 30), "the partial sums stay below 2 GiB");

// the padded width of a block of nblock columns
inline int sp_width(int nblock) { return nblock == 1 ? 1 : nblock <= 8 ? 8 : 16; }

template <int ND, int W> __global__ void __launch_bounds__(SP_BLOCK)
nm_spectral_pass_kernel(int n, const double *__restrict__ x, double gamma, const double *__restrict__ u, double *__restrict__ part)
{
#pragma clang fp contract(off)                                  // gamma d2 rounds before exp sees it; a fused multiply-add is written as one
    __shared__ __align__(16) double sx[SP_TILE * ND];
    __shared__ __align__(16) double su[SP_TILE * W];
    int idx[SP_RPT];
    bool valid[SP_RPT];
    double row[SP_RPT][ND], acc[SP_RPT][W];
    scan_rows<SpScan, ND>(x, nullptr, n, blockIdx.x, idx, valid, row);
#pragma unroll
    for (int r = 0; r < SP_RPT; ++r)
#pragma unroll
        for (int c = 0; c < W; ++c) acc[r][c] = 0.0;
    const int tid = threadIdx.x, ntiles = (n + SP_TILE - 1) / SP_TILE;
    const int own0 = blockIdx.x * (SP_ROWS / SP_TILE), own1 = own0 + SP_ROWS / SP_TILE;      // the tiles of the block's own rows
    for (int t = blockIdx.y; t < ntiles; t += gridDim.y) {
        const int j0 = t * SP_TILE, cnt = n - j0 < SP_TILE ? n - j0 : SP_TILE;
        __syncthreads();                                        // the tile before has been read by every wave
        const double *src = x + (size_t)j0 * ND;
        for (int k = tid; k < cnt * ND; k += SP_BLOCK) sx[k] = src[k];
        for (int k = tid; k < cnt * W; k += SP_BLOCK) su[k] = u ? u[(size_t)j0 * W + k] : 1.0;
        __syncthreads();
        auto walk = [&](auto own) {
            for (int jj = 0; jj < cnt; ++jj) {
                double col[ND], a[SP_RPT];
#pragma unroll
                for (int c = 0; c < ND; ++c) col[c] = sx[jj * ND + c];
#pragma unroll
                for (int r = 0; r < SP_RPT; ++r) {
                    const double e = exp(-(gamma * cl_d2<ND>(row[r], col)));
                    a[r] = (decltype(own)::value && j0 + jj == idx[r]) ? 0.0 : e;
                }
#pragma unroll
                for (int c = 0; c < W; ++c) {
                    const double uc = su[jj * W + c];
#pragma unroll
                    for (int r = 0; r < SP_RPT; ++r) acc[r][c] = __builtin_fma(a[r], uc, acc[r][c]);
                }
            }
        };
        if (t >= own0 && t < own1) walk(std::true_type{});      // the same in every thread: two loops, no test per pair in the second
        else walk(std::false_type{});
    }
#pragma unroll
    for (int r = 0; r < SP_RPT; ++r)
        if (valid[r]) {
            double *dst = part + ((size_t)blockIdx.y * n + idx[r]) * W;
#pragma unroll
            for (int c = 0; c < W; ++c) dst[c] = acc[r][c];
        }
}

// deg[i] from the slices in ascending order, rs[i] = 1 / sqrt(deg[i]); *bad = the first point whose degree is not positive
__global__ void __launch_bounds__(SP_BLOCK)
nm_spectral_degree_kernel(int n, int slices, const double *__restrict__ part, double *__restrict__ deg, double *__restrict__ rs, int *bad)
{
    const int i = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i >= n) return;
    double d = 0.0;
    for (int s = 0; s < slices; ++s) d = d + part[(size_t)s * n + i];
    deg[i] = d;
    rs[i] = 1.0 / sqrt(d);
    if (!(d > 0.0)) atomicMin(bad, i);
}

// element e = i w + c of the block: t = the slices' sum, y = rs[i] t, dst = alpha y + (beta cur + gam dst), u = rs[i] dst
__global__ void __launch_bounds__(SP_BLOCK)
nm_spectral_rows_kernel(int ne, int w, int slices, const double *__restrict__ part, const double *__restrict__ rs, double alpha, double beta,
                        double gam, const double *__restrict__ cur, double *__restrict__ dst, double *__restrict__ u)
{
#pragma clang fp contract(off)
    const int e = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (e >= ne) return;
    double t = 0.0;
    for (int s = 0; s < slices; ++s) t = t + part[(size_t)s * ne + e];
    const double r = rs[e / w], y = r * t;
    double rest = gam != 0.0 ? gam * dst[e] : 0.0;              // the scalars are the same in every thread
    if (beta != 0.0) rest = __builtin_fma(beta, cur[e], rest);
    const double out = __builtin_fma(alpha, y, rest);
    dst[e] = out;
    if (u) u[e] = r * out;
}

__global__ void __launch_bounds__(SP_BLOCK)
nm_spectral_axpby_kernel(int ne, int w, const double *__restrict__ rs, double alpha, double beta, const double *__restrict__ a,
                         double *__restrict__ b, double *__restrict__ u)
{
#pragma clang fp contract(off)
    const int e = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (e >= ne) return;
    const double out = __builtin_fma(alpha, b[e], beta * a[e]);
    b[e] = out;
    u[e] = rs[e / w] * out;
}

__global__ void __launch_bounds__(SP_BLOCK)
nm_spectral_resid_kernel(int ne, int w, const double *__restrict__ theta, const double *__restrict__ v, const double *__restrict__ mv,
                         double *__restrict__ r)
{
    const int e = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (e >= ne) return;
    r[e] = __builtin_fma(-theta[e % w], v[e], mv[e]);
}

// part[chunk][ra][c] = the chunk's sum of a[i][ra] b[i][c]
template <int W> __global__ void __launch_bounds__(SP_BLOCK)
nm_spectral_gram_kernel(int n, const double *__restrict__ a, const double *__restrict__ b, double *__restrict__ part)
{
    const int wv = threadIdx.x >> 6, p = threadIdx.x & 63, i0 = blockIdx.x * SP_CHUNK;
    for (int ra = wv; ra < W; ra += SP_BLOCK / 64) {            // the wave's rows of the result; no barrier inside
        double acc[W];
#pragma unroll
        for (int c = 0; c < W; ++c) acc[c] = 0.0;
        for (int q = 0; q < SP_CHUNK / 64; ++q) {
            const int i = i0 + q * 64 + p;
            const bool in = i < n;
            const size_t at = (size_t)(in ? i : 0) * W;
            const double av = in ? a[at + ra] : 0.0;           // a point past the end adds +0, which changes no bit
#pragma unroll
            for (int c = 0; c < W; ++c) acc[c] = __builtin_fma(av, in ? b[at + c] : 0.0, acc[c]);
        }
#pragma unroll
        for (int c = 0; c < W; ++c) {
            const double v = km_tree(acc[c]);
            if (p == 0) part[((size_t)blockIdx.x * W + ra) * W + c] = v;
        }
    }
}

// out[e] = the chunks' sums of element e of the W x W result, ascending
__global__ void __launch_bounds__(SP_BLOCK) nm_spectral_gram_join_kernel(int nchunks, int ww, const double *__restrict__ part, double *__restrict__ out)
{
    const int e = threadIdx.x;
    if (e >= ww) return;
    double s = 0.0;
    for (int b = 0; b < nchunks; ++b) s = s + part[(size_t)b * ww + e];
    out[e] = s;
}

// dst = src C; a thread reads its whole row before it writes one, so dst may be src
template <int W> __global__ void __launch_bounds__(SP_BLOCK)
nm_spectral_apply_kernel(int n, const double *src, const double *__restrict__ cmat, const double *__restrict__ rs, double *dst, double *__restrict__ u)
{
    __shared__ double sc[W * W];
    for (int k = threadIdx.x; k < W * W; k += SP_BLOCK) sc[k] = cmat[k];
    __syncthreads();
    const int i = blockIdx.x * SP_BLOCK + threadIdx.x;
    if (i >= n) return;
    double row[W];
#pragma unroll
    for (int k = 0; k < W; ++k) row[k] = src[(size_t)i * W + k];
    const double r = u ? rs[i] : 0.0;
#pragma unroll
    for (int c = 0; c < W; ++c) {
        double o = row[0] * sc[c];
#pragma unroll
        for (int k = 1; k < W; ++k) o = __builtin_fma(row[k], sc[k * W + c], o);
        dst[(size_t)i * W + c] = o;
        if (u) u[(size_t)i * W + c] = r * o;
    }
}

} // namespace nm
