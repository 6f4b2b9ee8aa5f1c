// nm_tsne.h — the kernels of the manifold stage (include/nm_tsne.h: the definitions): exact t-SNE of N points.  No N x N array
// exists: the device holds x (N ndim doubles), the lists (N k ints and doubles), the symmetric lists (at most 2 N k entries) and a
// few arrays of N.
//
// The skeleton is described in nm_scan.h, which holds its row loader, grid and screen; the shape here is TsScan: TS_ROWS = TS_RPT
// TS_BLOCK rows of a workgroup in registers, tiles of TS_TILE columns in LDS, a grid of (row blocks) x (column slices).  The tile
// loop (ts_scan) stands here, with what is this stage's own: the tiles that may hold the block's own rows are walked by a loop of
// their own.  A row past the end is point 0 again and its results are dropped.
// ts_d2 is the header's distance: with contraction off for this whole file (the pragma below) the template and the loop over a
// run-time ndim round the same way, so a pair has the same bits in the select, the gather and the sort.
//
// Affinities.
//   (nm_scan.h)            the screen for values that are not finite.
//   nm_tsne_bit_kernel     between two counting scans, one thread per row: the bit tried last stays in key[i] where fewer than k
//                          columns lay below the threshold; the next threshold is key[i] with the next bit; the count is cleared.
//   nm_tsne_count_kernel   the scan: a row counts the columns j != i whose d2, read as an integer, is below thr[i] (a non-negative
//                          double orders like its bit pattern); slices are joined by integer atomicAdd.  Bits 62 .. 0 in turn leave
//                          key[i] = the k-th smallest d2 of the row; a last scan at thr = key counts the columns strictly below.
//   nm_tsne_gather_kernel  the scan with one slice, so a thread meets its row's columns in ascending order: it keeps every column
//                          below key[i] and the first k - below[i] of those equal to it (ties by index), k in all, in nbr[i][].
//   nm_tsne_row_kernel     one workgroup per row: d2 of the k survivors again, a bitonic sort of (bits of d2, j) in LDS, nbr[i][] in
//                          that order, then the search for beta (the header's bracketing, every thread following the same scalars)
//                          and p[i][].
//   Bounds of the row kernel, u = 2^-53.  t_m = d_m - dmin is one rounding of exact data (the d_m are what they are: the
//   definition is in terms of the computed d2).  a_m = beta t_m rounds once, so exp sees an argument off by a_m u and returns
//   e_m (1 + (a_m + 1) u) at most (a correctly rounded argument reduction, 1 ulp).  A thread adds ceil(k / 256) terms, the tree has
//   8 levels: S carries at most (ceil(k / 256) + 8) u of itself from the adding, all terms being positive, and
//   sum_m e_m a_m u / S = u sum_m a_m p_m = u (H - ln S) <= u ln k from the arguments.  So p_m = e_m / S is within
//   (ceil(k / 256) + 11 + a_m + ln k) u of the exact quotient of the exact exponentials at the computed beta, and the p_m, each
//   rounded once more, add to 1 within (ceil(k / 256) + 12) u: both below the header's B u with B = ceil(k / 256) + 32 (ln k <= 8.4).
//   H = ln S + beta (A / S), A = sum t_m e_m: ln S is off by the relative error of S plus one rounding; beta A / S has terms
//   a_m p_m, each off by (a_m + 4) u of itself plus the adding, so by u (sum a_m^2 p_m + (ceil(k / 256) + 12) sum a_m p_m) =
//   u (M2 + (ceil(k / 256) + 12) ln k) at most.  The bisection decides on this H, so the beta it ends at has a true H within that of
//   ln(perplexity) plus the step between neighbouring doubles, |H'| beta 2 u = 2 u beta^2 Var(t) <= 2 u M2.  Together
//   (ceil(k / 256) + 32) u (1 + ln k + M2): the header's bound.
//
// Gradient.  P is symmetrised by the host once per call (two counting sorts and a merge: rows of (j, P_ij) in ascending j, the
// value (p_{j|i} + p_{i|j}) / (2 N) so P_ij == P_ji bit for bit), because the lists arrive in host memory anyway.
//   nm_tsne_plogp_kernel   once per call, a wave per row: sum_j P_ij ln P_ij and sum_j P_ij.
//   nm_tsne_attract_kernel a wave per row of the symmetric lists, whatever its length (a hub's N - 1 entries are walked by 64 lanes):
//                          sum_j P_ij w_ij (y_i - y_j) per component and sum_j P_ij ln(1 + d2_y); lane l adds entries l, l + 64, ...
//                          and a butterfly joins the lanes.
//   nm_tsne_pairs_kernel   the all-pairs scan over y, the kernel that runs once per step: per pair q = 1 + d2_y, w = 1 / q, the row
//                          adds w (not for j == i: only the tiles that hold the block's own rows test for it) and w^2 (y_i - y_j);
//                          a slice stores its rows' partial sums, nothing is added across workgroups.
//   nm_tsne_rows_kernel    joins the slices of a row in ascending order and adds Z's, kl's row terms over the block (a tree).
//   nm_tsne_total_kernel   one workgroup: the blocks' sums in a fixed order: Z, kl = sum P ln P + sum P ln q + ln Z sum P.
//   nm_tsne_step_kernel    per element g = 4 (exaggeration A - R / Z), the header's update where the call descends, and the block's
//                          sum of g^2; nm_tsne_norm_kernel joins those and writes the step's trace row.
//   Bound of a component of grad_i, in units of u times the sum of the magnitudes of its terms.  A repulsive term w^2 (y_i - y_j):
//   the difference 1, d2_y ncomp + 2, q one more, ts_rcp two more, the square twice that and one, the product: 2 ncomp + 14
//   <= 20.  A row adds N / S of them in sequence and S slices after that: N / S + S <= N + 1.  Z: the same adding, then 9 levels of
//   trees and the blocks in sequence, N + 64 at most; the division by Z and the factor: 2.  Repulsive: 2 N + 64 + 20 + 2; the
//   attractive terms P w (y_i - y_j): 12 each, a lane adds deg / 64 of them, deg <= N - 1 for a hub and <= 2 k else, 6 levels.
//   Together below (3 N + k + 64) u for every N >= 2: a = 3, b = 1, c = 64.  kl's terms are added the same way.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nm_scan.h"

#include <type_traits>

#pragma clang fp contract(off)      // every product and sum below rounds on its own; a fused multiply-add is written as one

namespace nm {

constexpr int TS_BLOCK = 256;                       // threads of a workgroup
constexpr int TS_RPT = 2;                           // rows of a thread
constexpr int TS_ROWS = TS_RPT * TS_BLOCK;          // rows of a workgroup
constexpr int TS_TILE = 128;                        // columns staged in LDS at a time: 16 KiB of coordinates at ndim = 16
constexpr int TS_MAXDIM = 16;
constexpr int TS_MAXCOMP = 3;
constexpr int TS_MAXK = 4096;
constexpr int64_t TS_MAXN = (int64_t)1 << 20;
constexpr int TS_GRID = 2048;                       // workgroups a scan aims at at least: 8 per compute unit
constexpr int TS_SPAN = 256;                        // tiles a workgroup walks at most
constexpr int TS_STEPS = 200;                       // evaluations of the search for beta
constexpr int TS_ATT = 4;                           // doubles per row of the attractive sums: ncomp components, then sum P ln q
constexpr int TS_PART = 4;                          // doubles per row and slice of the all-pairs pass: ncomp components, then Z's row

using TsScan = ScanShape<TS_BLOCK, TS_RPT, TS_TILE, TS_GRID, TS_SPAN>;
static_assert(TS_TILE <= TS_BLOCK && TS_ROWS % TS_TILE == 0, "the tiles of a block's own rows are whole tiles");

template <int ND> __device__ __forceinline__ double ts_d2(const double *a, const double *b)
{
    double d = a[0] - b[0];
    double acc = d * d;
#pragma unroll
    for (int c = 1; c < ND; ++c) {
        d = a[c] - b[c];
        acc = acc + d * d;
    }
    return acc;
}

__device__ __forceinline__ double ts_d2n(const double *a, const double *b, int nd)
{
    double d = a[0] - b[0];
    double acc = d * d;
    for (int c = 1; c < nd; ++c) {
        d = a[c] - b[c];
        acc = acc + d * d;
    }
    return acc;
}

// The tile loop.  pair(r, j, col, own) is called for row slot r and every column j of the walked tiles, col its coordinates; `own` is a
// type that says whether the tile may hold the block's own rows.  Tiles t0, t0 + tstep, ... < tend.
template <int ND, class Pair>
__device__ __forceinline__ void ts_scan(int n, const double *__restrict__ x, int t0, int tstep, int tend, Pair pair)
{
    __shared__ __align__(16) double sx[TS_TILE * ND];
    const int tid = threadIdx.x;
    const int own0 = blockIdx.x * (TS_ROWS / TS_TILE), own1 = own0 + TS_ROWS / TS_TILE;      // the tiles of the block's own rows
    for (int t = t0; t < tend; t += tstep) {
        const int j0 = t * TS_TILE, cnt = n - j0 < TS_TILE ? n - j0 : TS_TILE;
        __syncthreads();                                        // the tile before has been read by every wave
        const double *src = x + (size_t)j0 * ND;
        for (int k = tid; k < cnt * ND; k += TS_BLOCK) sx[k] = src[k];
        __syncthreads();
        auto walk = [&](auto own) {
            for (int jj = 0; jj < cnt; ++jj) {
                double col[ND];
#pragma unroll
                for (int c = 0; c < ND; ++c) col[c] = sx[jj * ND + c];
#pragma unroll
                for (int r = 0; r < TS_RPT; ++r) pair(r, j0 + jj, col, own);
            }
        };
        if (t >= own0 && t < own1) walk(std::true_type{});      // the same in every thread: two loops, no test per pair in the second
        else walk(std::false_type{});
    }
}

// ---- affinities: the radix select

__global__ void __launch_bounds__(TS_BLOCK)
nm_tsne_bit_kernel(int n, int k, int tried, int next, unsigned long long *__restrict__ key, unsigned long long *__restrict__ thr, int *__restrict__ count)
{
    const int i = blockIdx.x * TS_BLOCK + threadIdx.x;
    if (i >= n) return;
    unsigned long long v = tried >= 0 ? key[i] : 0ull;
    if (tried >= 0 && count[i] < k) v |= 1ull << tried;        // fewer than k below the threshold: the k-th is at or above it
    key[i] = v;
    thr[i] = next >= 0 ? v | (1ull << next) : v;
    count[i] = 0;
}

template <int ND> __global__ void __launch_bounds__(TS_BLOCK)
nm_tsne_count_kernel(int n, const double *__restrict__ x, const unsigned long long *__restrict__ thr, int *count)
{
    int idx[TS_RPT], cnt[TS_RPT];
    bool valid[TS_RPT];
    double row[TS_RPT][ND];
    unsigned long long lim[TS_RPT];
    scan_rows<TsScan, ND>(x, nullptr, n, blockIdx.x, idx, valid, row);
#pragma unroll
    for (int r = 0; r < TS_RPT; ++r) { lim[r] = valid[r] ? thr[idx[r]] : 0ull; cnt[r] = 0; }
    const int ntiles = (n + TS_TILE - 1) / TS_TILE;
    ts_scan<ND>(n, x, blockIdx.y, gridDim.y, ntiles, [&](int r, int j, const double (&col)[ND], auto own) {
        const bool below = (unsigned long long)__double_as_longlong(ts_d2<ND>(row[r], col)) < lim[r];
        cnt[r] += (below && !(decltype(own)::value && j == idx[r])) ? 1 : 0;
    });
#pragma unroll
    for (int r = 0; r < TS_RPT; ++r)
        if (valid[r] && cnt[r]) atomicAdd(count + idx[r], cnt[r]);
}

// one column slice (gridDim.y == 1): a thread meets the columns of its rows in ascending order
template <int ND> __global__ void __launch_bounds__(TS_BLOCK)
nm_tsne_gather_kernel(int n, int k, const double *__restrict__ x, const unsigned long long *__restrict__ key, const int *__restrict__ below,
                      int *__restrict__ nbr)
{
    int idx[TS_RPT], pos[TS_RPT], ties[TS_RPT];
    bool valid[TS_RPT];
    double row[TS_RPT][ND];
    unsigned long long lim[TS_RPT];
    scan_rows<TsScan, ND>(x, nullptr, n, blockIdx.x, idx, valid, row);
#pragma unroll
    for (int r = 0; r < TS_RPT; ++r) {
        lim[r] = key[idx[r]];
        ties[r] = valid[r] ? k - below[idx[r]] : 0;            // columns equal to the key that are kept: the first by index
        pos[r] = valid[r] ? 0 : k;                              // a row past the end keeps nothing
    }
    const int ntiles = (n + TS_TILE - 1) / TS_TILE;
    ts_scan<ND>(n, x, 0, 1, ntiles, [&](int r, int j, const double (&col)[ND], auto own) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(ts_d2<ND>(row[r], col));
        if (b > lim[r] || (decltype(own)::value && j == idx[r])) return;
        if (b == lim[r]) {
            if (ties[r] <= 0) return;
            --ties[r];
        }
        if (pos[r] < k) nbr[(size_t)idx[r] * k + pos[r]++] = j; // (the counts make it k in all; the test keeps a fault out of reach)
    });
}

// ---- affinities: one workgroup per row

// the sums S = sum e_m and A = sum t_m e_m at beta, the same in every thread: a thread adds every TS_BLOCK-th term, a tree the rest
__device__ __forceinline__ void ts_row_sums(int k, const double *__restrict__ st, double beta, double (*red)[2], double &s, double &a)
{
    const int tid = threadIdx.x;
    double ls = 0.0, la = 0.0;
    for (int m = tid; m < k; m += TS_BLOCK) {
        const double e = exp(-(beta * st[m]));
        ls = ls + e;
        la = la + st[m] * e;
    }
    __syncthreads();                                            // the sums before have been read
    red[tid][0] = ls;
    red[tid][1] = la;
    for (int h = TS_BLOCK / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (tid < h) {
            red[tid][0] = red[tid][0] + red[tid + h][0];
            red[tid][1] = red[tid][1] + red[tid + h][1];
        }
    }
    __syncthreads();
    s = red[0][0];
    a = red[0][1];
}

__global__ void __launch_bounds__(TS_BLOCK)
nm_tsne_row_kernel(int n, int ndim, int k, const double *__restrict__ x, double logpx, int *__restrict__ nbr, double *__restrict__ p,
                   double *__restrict__ beta_out)
{
    __shared__ unsigned long long skey[TS_MAXK];                // the bits of d2, then t_m as a double in the same place
    __shared__ int sidx[TS_MAXK];
    __shared__ double red[TS_BLOCK][2];
    const int i = blockIdx.x, tid = threadIdx.x;
    int np2 = 1;
    while (np2 < k) np2 <<= 1;
    double xi[TS_MAXDIM];
    for (int c = 0; c < ndim; ++c) xi[c] = x[(size_t)i * ndim + c];
    for (int m = tid; m < np2; m += TS_BLOCK) {
        if (m < k) {
            int j = nbr[(size_t)i * k + m];
            j = j < 0 ? 0 : j >= n ? n - 1 : j;
            sidx[m] = j;
            skey[m] = (unsigned long long)__double_as_longlong(ts_d2n(xi, x + (size_t)j * ndim, ndim));
        } else {
            sidx[m] = 0x7fffffff;                               // padding sorts behind every entry
            skey[m] = ~0ull;
        }
    }
    // bitonic sort of (key, index), ascending
    for (int size = 2; size <= np2; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int m = tid; m < np2; m += TS_BLOCK) {
                const int o = m ^ stride;
                if (o > m) {
                    const unsigned long long ka = skey[m], kb = skey[o];
                    const int ia = sidx[m], ib = sidx[o];
                    const bool gt = ka > kb || (ka == kb && ia > ib);
                    if (gt == ((m & size) == 0)) { skey[m] = kb; skey[o] = ka; sidx[m] = ib; sidx[o] = ia; }
                }
            }
        }
    __syncthreads();
    const double dmin = __longlong_as_double((long long)skey[0]);
    __syncthreads();
    double *st = (double *)skey;
    for (int m = tid; m < k; m += TS_BLOCK) {
        nbr[(size_t)i * k + m] = sidx[m];
        st[m] = __longlong_as_double((long long)skey[m]) - dmin;     // each thread rewrites its own entries
    }
    __syncthreads();
    // the header's bracketing; every thread follows the same scalars
    double beta = 1.0, lo = -INFINITY, hi = INFINITY, s, a;
    for (int step = 0; step < TS_STEPS; ++step) {
        ts_row_sums(k, st, beta, red, s, a);
        const double h = log(s) + beta * (a / s);
        double nb;
        if (h == logpx) break;
        if (h > logpx) {
            lo = beta;
            nb = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0;
        } else {
            hi = beta;
            nb = lo == -INFINITY ? beta / 2.0 : (beta + lo) / 2.0;
        }
        if (nb == beta) break;
        beta = nb;
    }
    ts_row_sums(k, st, beta, red, s, a);
    for (int m = tid; m < k; m += TS_BLOCK) p[(size_t)i * k + m] = exp(-(beta * st[m])) / s;
    if (tid == 0) beta_out[i] = beta;
}

// ---- gradient

// joins the lanes of a wave, the same order on every call; every lane ends with the sum
__device__ __forceinline__ double ts_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o, 64);
    return v;
}

// joins the threads of a workgroup through red[TS_BLOCK]; thread 0 returns the sum
__device__ __forceinline__ double ts_block_sum(double v, double *red)
{
    const int tid = threadIdx.x;
    __syncthreads();
    red[tid] = v;
    for (int h = TS_BLOCK / 2; h > 0; h >>= 1) {
        __syncthreads();
        if (tid < h) red[tid] = red[tid] + red[tid + h];
    }
    __syncthreads();
    return red[0];
}

// pconst[i][0] = sum_j P_ij ln P_ij over P_ij > 0, pconst[i][1] = sum_j P_ij: a wave per row
__global__ void __launch_bounds__(TS_BLOCK)
nm_tsne_plogp_kernel(int n, const long long *__restrict__ rowptr, const double *__restrict__ val, double *__restrict__ pconst)
{
    const int i = blockIdx.x * (TS_BLOCK / 64) + (int)threadIdx.x / 64, lane = threadIdx.x & 63;
    if (i >= n) return;                                         // the whole wave
    double a = 0.0, s = 0.0;
    for (long long e = rowptr[i] + lane; e < rowptr[i + 1]; e += 64) {
        const double pij = val[e];
        if (pij > 0.0) a = a + pij * log(pij);
        s = s + pij;
    }
    a = ts_wave_sum(a);
    s = ts_wave_sum(s);
    if (lane == 0) { pconst[2 * (size_t)i] = a; pconst[2 * (size_t)i + 1] = s; }
}

template <int NC> __global__ void __launch_bounds__(TS_BLOCK)
nm_tsne_attract_kernel(int n, const long long *__restrict__ rowptr, const int *__restrict__ col, const double *__restrict__ val,
                       const double *__restrict__ y, double *__restrict__ att)
{
    const int i = blockIdx.x * (TS_BLOCK / 64) + (int)threadIdx.x / 64, lane = threadIdx.x & 63;
    if (i >= n) return;                                         // the whole wave
    double yi[NC], acc[NC], lq = 0.0;
#pragma unroll
    for (int c = 0; c < NC; ++c) { yi[c] = y[(size_t)i * NC + c]; acc[c] = 0.0; }
    for (long long e = rowptr[i] + lane; e < rowptr[i + 1]; e += 64) {
        const double pij = val[e];
        double yj[NC];
#pragma unroll
        for (int c = 0; c < NC; ++c) yj[c] = y[(size_t)col[e] * NC + c];
        const double q = 1.0 + ts_d2<NC>(yi, yj);
        const double pw = pij / q;
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[c] = acc[c] + pw * (yi[c] - yj[c]);
        if (pij > 0.0) lq = lq + pij * log(q);
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = ts_wave_sum(acc[c]);
    lq = ts_wave_sum(lq);
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < NC; ++c) att[(size_t)i * TS_ATT + c] = acc[c];
        att[(size_t)i * TS_ATT + 3] = lq;
    }
}

// 1 / q for 1 <= q < 2^1000: the hardware's estimate and two Newton steps, five instructions where the correctly rounded quotient
// takes eleven (it scales against overflow, which q cannot have, and corrects the last bit).  The estimate is good to 2^-26 at
// least, so the first step leaves 2^-52 and the second the roundings of its own two operations: within 2 u of 1 / q, the same bits
// on every call.
__device__ __forceinline__ double ts_rcp(double q)
{
    double r = __builtin_amdgcn_rcp(q);
    double e = __builtin_fma(-q, r, 1.0);
    r = __builtin_fma(r, e, r);
    e = __builtin_fma(-q, r, 1.0);
    return __builtin_fma(r, e, r);
}

// the all-pairs pass: part[slice][i][c] = sum over the slice's columns of w^2 (y_i[c] - y_j[c]), part[slice][i][3] of w, j != i
template <int NC> __global__ void __launch_bounds__(TS_BLOCK)
nm_tsne_pairs_kernel(int n, const double *__restrict__ y, double *__restrict__ part)
{
    int idx[TS_RPT];
    bool valid[TS_RPT];
    double row[TS_RPT][NC], rep[TS_RPT][NC], zr[TS_RPT];
    scan_rows<TsScan, NC>(y, nullptr, n, blockIdx.x, idx, valid, row);
#pragma unroll
    for (int r = 0; r < TS_RPT; ++r) {
        zr[r] = 0.0;
#pragma unroll
        for (int c = 0; c < NC; ++c) rep[r][c] = 0.0;
    }
    const int ntiles = (n + TS_TILE - 1) / TS_TILE;
    ts_scan<NC>(n, y, blockIdx.y, gridDim.y, ntiles, [&](int r, int j, const double (&col)[NC], auto own) {
        const double w = ts_rcp(1.0 + ts_d2<NC>(row[r], col));
        const double w2 = w * w;
        zr[r] = zr[r] + ((decltype(own)::value && j == idx[r]) ? 0.0 : w);
#pragma unroll
        for (int c = 0; c < NC; ++c) rep[r][c] = __builtin_fma(w2, row[r][c] - col[c], rep[r][c]);
    });
#pragma unroll
    for (int r = 0; r < TS_RPT; ++r)
        if (valid[r]) {
            double *dst = part + ((size_t)blockIdx.y * n + idx[r]) * TS_PART;
#pragma unroll
            for (int c = 0; c < NC; ++c) dst[c] = rep[r][c];
            dst[3] = zr[r];
        }
}

// rep[i][c] and Z's row from the slices in ascending order; bsum[block][0..3] = the block's sums of Z's rows, of sum P ln q, of
// sum P ln P and of sum P
__global__ void __launch_bounds__(TS_BLOCK)
nm_tsne_rows_kernel(int n, int ncomp, int slices, const double *__restrict__ part, const double *__restrict__ att,
                    const double *__restrict__ pconst, double *__restrict__ rep, double *__restrict__ bsum)
{
    __shared__ double red[TS_BLOCK];
    const int i = blockIdx.x * TS_BLOCK + threadIdx.x;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if (i < n) {
        double acc[TS_PART] = {0.0, 0.0, 0.0, 0.0};
        for (int s = 0; s < slices; ++s)
            for (int c = 0; c < TS_PART; ++c)
                if (c < ncomp || c == 3) acc[c] = acc[c] + part[((size_t)s * n + i) * TS_PART + c];
        for (int c = 0; c < TS_MAXCOMP; ++c) rep[(size_t)i * TS_MAXCOMP + c] = acc[c];
        v[0] = acc[3];
        v[1] = att[(size_t)i * TS_ATT + 3];
        v[2] = pconst[2 * (size_t)i];
        v[3] = pconst[2 * (size_t)i + 1];
    }
    for (int c = 0; c < 4; ++c) {
        const double s = ts_block_sum(v[c], red);
        if (threadIdx.x == 0) bsum[(size_t)blockIdx.x * 4 + c] = s;
    }
}

// one workgroup: tot[0] = Z, tot[1] = kl
__global__ void __launch_bounds__(TS_BLOCK) nm_tsne_total_kernel(int nblocks, const double *__restrict__ bsum, double *__restrict__ tot)
{
    __shared__ double red[TS_BLOCK];
    double s[4];
    for (int c = 0; c < 4; ++c) {
        double v = 0.0;
        for (int b = threadIdx.x; b < nblocks; b += TS_BLOCK) v = v + bsum[(size_t)b * 4 + c];
        s[c] = ts_block_sum(v, red);
    }
    if (threadIdx.x == 0) {
        tot[0] = s[0];
        tot[1] = (s[2] + s[1]) + log(s[0]) * s[3];
    }
}

// per element of y: the gradient, and the header's update where `descend`; bnorm[block] = the block's sum of g^2
__global__ void __launch_bounds__(TS_BLOCK)
nm_tsne_step_kernel(int n, int ncomp, double exaggeration, const double *__restrict__ att, const double *__restrict__ rep,
                    const double *__restrict__ tot, double *__restrict__ grad, int descend, double momentum, double rate,
                    double *__restrict__ y, double *__restrict__ update, double *__restrict__ gains, double *__restrict__ bnorm)
{
    __shared__ double red[TS_BLOCK];
    const int e = blockIdx.x * TS_BLOCK + threadIdx.x;
    double g2 = 0.0;
    if (e < n * ncomp) {
        const int i = e / ncomp, c = e - i * ncomp;
        const double g = 4.0 * (exaggeration * att[(size_t)i * TS_ATT + c] - rep[(size_t)i * TS_MAXCOMP + c] / tot[0]);
        grad[e] = g;
        g2 = g * g;
        if (descend) {
            double ga = gains[e];
            const double up = update[e];
            ga = up * g < 0.0 ? ga + 0.2 : ga * 0.8;
            ga = ga < 0.01 ? 0.01 : ga;
            const double nu = momentum * up - rate * (g * ga);
            gains[e] = ga;
            update[e] = nu;
            y[e] = y[e] + nu;
        }
    }
    const double s = ts_block_sum(g2, red);
    if (threadIdx.x == 0) bnorm[blockIdx.x] = s;
}

// one workgroup: the step's trace row: kl, Z, the gradient's 2-norm
__global__ void __launch_bounds__(TS_BLOCK)
nm_tsne_norm_kernel(int nblocks, const double *__restrict__ bnorm, const double *__restrict__ tot, double *__restrict__ trace)
{
    __shared__ double red[TS_BLOCK];
    double v = 0.0;
    for (int b = threadIdx.x; b < nblocks; b += TS_BLOCK) v = v + bnorm[b];
    const double s = ts_block_sum(v, red);
    if (threadIdx.x == 0) {
        trace[0] = tot[1];
        trace[1] = tot[0];
        trace[2] = sqrt(s);
    }
}

} // namespace nm
