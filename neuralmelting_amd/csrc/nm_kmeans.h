// nm_kmeans.h — the kernels of k-means (include/nm_distr.h, nm_cluster_kmeans: the definitions; the entry point stands in
// nm_distr_api.hip, the distance is nm_d2.h's, which DBSCAN shares): Lloyd's iteration of N points x[n][c], float64,
// row-major, for all restarts at once.  The device holds x, one byte of label per point and restart, the centres of every restart,
// the partial sums of a step (at most N ndim doubles: one set per KM_CHUNK = 4096 points, and restarts x clusters <= 4096) and a
// few ints per restart.  No N x k array of distances exists.
//
// A step is three launches, and the host looks at the restarts' states only every KM_LOOK steps: a step of restarts that have all
// finished does nothing.
//
//   nm_kmeans_assign_kernel   nm_scan.h's skeleton: the points are the rows (KM_ROWS of a workgroup in registers, scan_rows), the
//                             nrestarts * k centres are the columns, column q = r k + j, staged in LDS in tiles of KM_TILE and read
//                             as a broadcast.  x is read once for all restarts.  A row keeps the smallest cl_d2 of a restart's
//                             centres, the first j on equal bits (a strict <, j ascending); behind the restart's last centre it
//                             writes the label's byte and says whether it differs from the byte that stood there (one integer
//                             atomicOr per wave on changed[r]).  The columns of a finished restart are walked over.
//   nm_kmeans_sums_kernel     one workgroup per (chunk of KM_CHUNK points, restart that goes on): lane p of a wave sums the members
//                             of the wave's cluster among the KM_PIECE = 64 points of piece p, ascending (a point that is no member
//                             adds +0, which changes no bit), the 64 lanes are summed as a binary tree by __shfl_xor, and lane 0
//                             writes the chunk's sum and count of that cluster.  The four waves take clusters j, j + 1, j + 2, j + 3.
//   nm_kmeans_finish_kernel   one workgroup per restart: the steps 2 to 5 of the header.  A thread per (j, c) adds the chunks'
//                             sums ascending, divides once, writes the centre and leaves (C' - C)^2 in LDS; thread 0 adds those
//                             squares, j then c ascending, and decides.  It clears changed[r] for the next step.
//   nm_kmeans_inertia_kernel  behind the last step, one wave per (chunk, restart) with the restart's centres in LDS: the same pieces
//                             and the same tree over d2(i, centre of label[i]).  The host adds the chunks ascending.
//
// Nothing waits for anything inside a launch: no spin loop, no polled flag, no cooperative launch.  The only atomic is an integer
// atomicOr of 1.  No sum depends on the schedule: pieces, trees and chunks are fixed by the index alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nm_d2.h"
#include "nm_scan.h"

namespace nm {

constexpr int KM_BLOCK = 256;                       // threads of a workgroup
constexpr int KM_RPT = 2;                           // rows of a thread
constexpr int KM_ROWS = KM_RPT * KM_BLOCK;          // rows of a workgroup of the assignment
constexpr int KM_TILE = 256;                        // centres staged in LDS at a time: 32 KiB at ndim = 16
constexpr int KM_PIECE = 64;                        // points that one lane sums in ascending order
constexpr int KM_CHUNK = 64 * KM_PIECE;             // points of a wave's tree: the unit of the partial sums
constexpr int KM_MAXDIM = 16;
constexpr int64_t KM_MAXN = (int64_t)1 << 21;
constexpr int KM_MAXK = 256;
constexpr int KM_MAXR = 64;
constexpr int KM_MAXCOLS = 4096;                    // k * nrestarts at most
#ifndef KM_LOOK
#define KM_LOOK 4                                   // steps between two looks of the host at the restarts' states
#endif

enum { KM_RUN = 0, KM_LAST = 1, KM_DONE = 2 };      // a restart iterates; has its centres and waits for its last assignment; is frozen

using KmScan = ScanShape<KM_BLOCK, KM_RPT, KM_TILE, 1, 1>;
static_assert(KM_MAXR <= KM_BLOCK, "a restart's state is staged by one thread each");
static_assert(KM_MAXK <= 256, "a label is one byte");

template <int ND> __global__ void __launch_bounds__(KM_BLOCK)
nm_kmeans_assign_kernel(int n, const double *__restrict__ x, int k, int nr, const double *__restrict__ centre, const int *__restrict__ state,
                        size_t stride, uint8_t *lab, int *changed)
{
    __shared__ __align__(16) double sx[KM_TILE * ND];
    __shared__ int live[KM_MAXR];
    const int tid = threadIdx.x;
    bool mine = false;
    if (tid < nr) {
        mine = state[tid] != KM_DONE;
        live[tid] = mine;
    }
    if (!__syncthreads_or(mine)) return;                        // every restart is frozen: the same answer in every thread
    int idx[KM_RPT], arg[KM_RPT];
    bool valid[KM_RPT];
    double row[KM_RPT][ND], best[KM_RPT];
    scan_rows<KmScan, ND>(x, nullptr, n, blockIdx.x, idx, valid, row);
#pragma unroll
    for (int r = 0; r < KM_RPT; ++r) { arg[r] = 0; best[r] = 0.0; }
    const int ncols = nr * k;
    for (int j0 = 0; j0 < ncols; j0 += KM_TILE) {
        const int cnt = ncols - j0 < KM_TILE ? ncols - j0 : KM_TILE;
        __syncthreads();                                        // the tile before has been read by every wave
        const double *src = centre + (size_t)j0 * ND;
        for (int q = tid; q < cnt * ND; q += KM_BLOCK) sx[q] = src[q];
        __syncthreads();
        int r = j0 / k, j = j0 - r * k;                         // the restart and the cluster of the tile's first column
        for (int jj = 0; jj < cnt; ++jj) {
            if (live[r]) {                                      // the same in every thread
                double col[ND];
#pragma unroll
                for (int c = 0; c < ND; ++c) col[c] = sx[jj * ND + c];
#pragma unroll
                for (int s = 0; s < KM_RPT; ++s) {
                    const double d = cl_d2<ND>(row[s], col);
                    if (j == 0 || d < best[s]) { best[s] = d; arg[s] = j; }
                }
                if (j == k - 1) {                               // the restart's last centre: the label stands
                    bool differs = false;
#pragma unroll
                    for (int s = 0; s < KM_RPT; ++s)
                        if (valid[s]) {
                            uint8_t *p = lab + (size_t)r * stride + idx[s];
                            differs = differs || *p != (uint8_t)arg[s];
                            *p = (uint8_t)arg[s];
                        }
                    if (__any(differs) && (tid & 63) == 0) atomicOr(changed + r, 1);
                }
            }
            if (++j == k) { j = 0; ++r; }
        }
    }
}

// the binary tree over the 64 lanes: a[2 i] + a[2 i + 1], level by level (both lanes of a pair form the same sum: the order of
// the two terms changes no bit)
__device__ __forceinline__ double km_tree(double v)
{
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) v += __shfl_xor(v, s);
    return v;
}

template <int ND> __global__ void __launch_bounds__(KM_BLOCK)
nm_kmeans_sums_kernel(int n, const double *__restrict__ x, int k, int nr, int step, const int *__restrict__ state, const int *__restrict__ changed,
                      size_t stride, const uint8_t *__restrict__ lab, double *__restrict__ part, int *__restrict__ cntp)
{
    __shared__ uint8_t slab[KM_CHUNK];                          // the chunk's labels, [point of the piece][piece]
    const int b = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    if (state[r] != KM_RUN || (step > 1 && !changed[r])) return;            // finished, or at its fixed point: the same in every thread
    const int i0 = b * KM_CHUNK;
    for (int o = tid; o < KM_CHUNK; o += KM_BLOCK)
        slab[(o % KM_PIECE) * 64 + o / KM_PIECE] = i0 + o < n ? lab[(size_t)r * stride + i0 + o] : (uint8_t)0;
    __syncthreads();
    const int w = tid >> 6, p = tid & 63, base = i0 + p * KM_PIECE;
    for (int j = w; j < k; j += KM_BLOCK / 64) {                // the wave's clusters; no barrier inside
        double acc[ND];
        int members = 0;
#pragma unroll
        for (int c = 0; c < ND; ++c) acc[c] = 0.0;
#pragma unroll 4
        for (int q = 0; q < KM_PIECE; ++q) {
            const int i = base + q;
            const bool in = i < n && slab[q * 64 + p] == j;
            const double *src = x + (size_t)(i < n ? i : 0) * ND;
#pragma unroll
            for (int c = 0; c < ND; ++c) acc[c] += in ? src[c] : 0.0;
            members += in;
        }
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) members += __shfl_xor(members, s);
        const size_t at = ((size_t)b * nr + r) * k + j;
#pragma unroll
        for (int c = 0; c < ND; ++c) {
            const double v = km_tree(acc[c]);
            if (p == 0) part[at * ND + c] = v;
        }
        if (p == 0) cntp[at] = members;
    }
}

__global__ void __launch_bounds__(KM_BLOCK)
nm_kmeans_finish_kernel(int ndim, int k, int nr, int nchunks, int step, int max_iter, double tol, const double *__restrict__ part,
                        const int *__restrict__ cntp, double *centre, int *state, int *status, int *iters, int *changed)
{
    __shared__ double sq[KM_MAXK * KM_MAXDIM];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int st = state[r], ch = changed[r];
    __syncthreads();                                            // every thread has read them
    if (tid == 0) changed[r] = 0;
    if (st == KM_DONE) return;
    if (st == KM_LAST) {                                        // the assignment of this step was its last
        if (tid == 0) state[r] = KM_DONE;
        return;
    }
    if (step > 1 && !ch) {                                      // L_t == L_{t-1}: the fixed point
        if (tid == 0) { state[r] = KM_DONE; status[r] = 0; iters[r] = step - 1; }
        return;
    }
    for (int e = tid; e < k * ndim; e += KM_BLOCK) {
        const int j = e / ndim, c = e - j * ndim;
        double sum = 0.0;
        int members = 0;
        for (int b = 0; b < nchunks; ++b) {                     // the chunks ascending
            const size_t at = ((size_t)b * nr + r) * k + j;
            sum += part[at * ndim + c];
            members += cntp[at];
        }
        const size_t ce = ((size_t)r * k + j) * ndim + c;
        const double old = centre[ce], now = members ? sum / (double)members : old;     // a cluster without members keeps its centre
        centre[ce] = now;
        const double d = now - old;
        sq[e] = d * d;
    }
    __syncthreads();
    if (tid) return;
    double shift = 0.0;
    for (int e = 0; e < k * ndim; ++e) shift += sq[e];          // j then c ascending
    const int s = shift <= tol ? 1 : step == max_iter ? 2 : -1;
    if (s > 0) { state[r] = KM_LAST; status[r] = s; iters[r] = step; }
}

template <int ND> __global__ void __launch_bounds__(64)
nm_kmeans_inertia_kernel(int n, const double *__restrict__ x, int k, int nr, const double *__restrict__ centre, size_t stride,
                         const uint8_t *__restrict__ lab, double *__restrict__ ipart)
{
#pragma clang fp contract(off)                                  // a term is rounded as cl_d2 leaves it, then added
    __shared__ double sc[KM_MAXK * ND];                         // the restart's centres
    const int b = blockIdx.x, r = blockIdx.y, p = threadIdx.x, base = b * KM_CHUNK + p * KM_PIECE;
    for (int q = p; q < k * ND; q += 64) sc[q] = centre[(size_t)r * k * ND + q];
    __syncthreads();
    double acc = 0.0;
#pragma unroll 8
    for (int q = 0; q < KM_PIECE; ++q) {                        // the loads are unconditional: a point past the end is point 0 and adds +0
        const bool in = base + q < n;
        const int i = in ? base + q : 0;
        double row[ND], col[ND];
        const double *src = x + (size_t)i * ND, *cen = sc + (int)lab[(size_t)r * stride + i] * ND;
#pragma unroll
        for (int c = 0; c < ND; ++c) { row[c] = src[c]; col[c] = cen[c]; }
        const double d = cl_d2<ND>(row, col);
        acc = acc + (in ? d : 0.0);
    }
    acc = km_tree(acc);
    if (p == 0) ipart[(size_t)b * nr + r] = acc;
}

} // namespace nm
