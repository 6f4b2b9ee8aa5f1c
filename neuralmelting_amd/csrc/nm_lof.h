// nm_lof.h — the kernels of the outlier stage (include/nm_distr.h: the definitions of nm_distr_lof): the local outlier factor of
// many small sets at once, x[s][i][c], float64.  No npts x npts array exists: the device holds x, the lists (k ints and k doubles
// per point) and three doubles per point.
//
//   (nm_scan.h)                 the screen for values that are not finite, over all points of all sets.
//   nm_lof_neighbours_kernel    one workgroup per row block of one set, one thread per row, the row's coordinates in registers (their
//                               number is a template parameter).  The set's own columns are walked once, in ascending order, in tiles
//                               of LOF_TILE points that are copied into LDS as they lie; every thread reads the same column at the
//                               same time (a broadcast read).  A thread keeps its k best (bits of d2, j) in LDS, entry m of thread
//                               t at [m][t] (neighbouring threads, neighbouring banks), as a binary heap with the largest (key, j)
//                               at the root, and the root's key, the k-th, in a register: the heap is touched only when a column's
//                               key lies below that key, which after the first k columns happens about k ln(npts / k) times per
//                               row.  The column then replaces the root and sinks to its place: log2 k steps, each the reads of two
//                               children that do not wait for one another.  (At the production shape a list kept sorted by shifting
//                               took 17.5 ms, an unordered one whose largest was found again by k reads 15.8 ms, the heap 9.5 ms:
//                               64 lanes that each keep k of npts columns touch a list at nearly every column, so the wave pays for
//                               one at nearly every column and the steps that wait for LDS are what counts: DESIGN.md §9 f-10.)
//                               The columns come in ascending j, so a key that equals the k-th has the larger index and stays out:
//                               the kept set is the header's k smallest (d2, j).  A non-negative double orders
//                               like its bit pattern; the list starts as k entries of all ones, which lie behind every distance
//                               (+inf included).  A row past the end has the k-th key 0, which nothing lies below.  At the end the
//                               workgroup writes its rows' lists as one contiguous piece of nbr and of dist = sqrt(d2), each entry
//                               at its rank, the number of its row's entries with a smaller (key, j); kdist[i] = dist[i][k - 1].
//                               The lists of lof_rows(k) rows take lof_rows(k) k 10 bytes of LDS, at most 40 KiB, beside a tile of
//                               at most 16 KiB: the rows of a workgroup are halved above k = 16 and again above k = 32.
//   nm_lof_lrd_kernel           one thread per point: the sum of reach(i, m) over its list in list order, lrd.
//   nm_lof_lof_kernel           one thread per point: the sum of lrd[nbr[i][m]] / lrd[i] in list order, lof.
//
// lof_d2 is the header's distance: with contraction off inside it (the pragma in its body: the file that includes this one keeps
// its own setting) every difference, product and sum rounds on its own; negating every difference changes no bit, so
// d2(i, j) == d2(j, i).  No other expression here holds a product next to a sum.
//
// Bounds, u = 2^-53, to first order in u.  d2 is a sum of non-negative terms: a difference rounds once, its square carries two
// roundings and one of its own, the first square then passes through ndim - 1 additions: (ndim + 2) u d2.  The square root halves
// that, (ndim / 2 + 1) u, and rounds itself (the f64 quotient is the correctly rounded one, u; the f64 square root is an expansion
// around the hardware's estimate, for which 2 u are allowed): dist and kdist to (ndim / 2 + 3) u.  reach is the larger of two such
// numbers and carries the same.  The sum of k of them, all non-negative, in sequence: k - 1 more; the division by k one; adding
// 1e-10 to a non-negative number rounds once and lowers what the sum carried; the reciprocal one: lrd to (ndim / 2 + k + 5) u, below
// the header's (ndim / 2 + k + 8) u.  A term lrd[j] / lrd[i] carries both, 2 (ndim / 2 + k + 5) u, and its quotient's u; k positive
// terms in sequence k - 1, the last division one: lof to (ndim + 3 k + 11) u of itself, below the header's (ndim + 3 k + 16) u.  All
// this with the lists given: the selection itself is exact in the computed d2, which both sides of a comparison form with the same
// bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nm_scan.h"

namespace nm {

constexpr int LOF_ROWS = 256;                       // rows (threads) of a workgroup up to k = LOF_KFULL
constexpr int LOF_KFULL = 16;                       // above it the rows are halved, above twice it halved again
constexpr int LOF_TILE = 128;                       // columns staged in LDS at a time: 16 KiB of coordinates at ndim = 16
constexpr int LOF_BLOCK = 256;                      // threads of a workgroup of the two gathers
constexpr int LOF_MAXDIM = 16;
constexpr int LOF_MAXK = 64;
constexpr int LOF_MAXPTS = 4096;                    // a list holds its indices in 16 bits
constexpr int64_t LOF_MAXSETS = (int64_t)1 << 20;
constexpr int64_t LOF_MAXN = (int64_t)1 << 21;      // points of all sets together
constexpr double LOF_FLOOR = 1e-10;                 // sklearn's, added to the mean reach

static_assert(LOF_MAXK <= 4 * LOF_KFULL && LOF_ROWS % 256 == 0, "a workgroup keeps at least one whole wave of rows");
static_assert(LOF_MAXPTS <= 65535, "0xffff is no point");

// the rows of a workgroup of the neighbour pass, sized from k on the host: the lists of all of them stay within 40 KiB
inline int lof_rows(int k) { return k <= LOF_KFULL ? LOF_ROWS : k <= 2 * LOF_KFULL ? LOF_ROWS / 2 : LOF_ROWS / 4; }
using LofScreen = ScanShape<LOF_BLOCK, 1, LOF_TILE, 1, 1>;                      // for nm_scan.h's screen: one thread per point

inline size_t lof_list_bytes(int k) { return (size_t)lof_rows(k) * k * (sizeof(unsigned long long) + sizeof(unsigned short)); }

template <int ND> __device__ __forceinline__ double lof_d2(const double (&a)[ND], const double (&b)[ND])
{
#pragma clang fp contract(off)      // every product and sum of this body rounds on its own
    double d = a[0] - b[0];
    double acc = d * d;
#pragma unroll
    for (int c = 1; c < ND; ++c) {
        d = a[c] - b[c];
        acc = acc + d * d;
    }
    return acc;
}

// blockDim.x = lof_rows(k) threads and lof_list_bytes(k) of dynamic LDS; block b is row block b % blocks of set b / blocks
template <int ND> __global__ void __launch_bounds__(LOF_ROWS)
nm_lof_neighbours_kernel(int npts, int k, int blocks, const double *__restrict__ x, int *__restrict__ nbr, double *__restrict__ dist,
                         double *__restrict__ kdist)
{
    extern __shared__ __align__(16) unsigned char lof_lists[];
    __shared__ __align__(16) double sx[LOF_TILE * ND];
    const int rows = blockDim.x, tid = threadIdx.x;
    const int set = blockIdx.x / blocks, r0 = (blockIdx.x - set * blocks) * rows;
    const double *xs = x + (size_t)set * npts * ND;
    unsigned long long *lkey = (unsigned long long *)lof_lists;                 // [k][rows]
    unsigned short *lidx = (unsigned short *)(lkey + (size_t)k * rows);         // [k][rows]
    const int i = r0 + tid;
    const bool valid = i < npts;
    double row[ND];
    {
        const double *src = xs + (size_t)(valid ? i : 0) * ND;
#pragma unroll
        for (int c = 0; c < ND; ++c) row[c] = src[c];
    }
    for (int m = 0; m < k; ++m) {                                               // the thread's own entries: no barrier is needed
        lkey[m * rows + tid] = ~0ull;
        lidx[m * rows + tid] = 0xffff;
    }
    unsigned long long kth = valid ? ~0ull : 0ull;                              // the key at the root, the largest of the k
    for (int j0 = 0; j0 < npts; j0 += LOF_TILE) {
        const int cnt = npts - j0 < LOF_TILE ? npts - j0 : LOF_TILE;
        __syncthreads();                                                        // the tile before has been read by every wave
        const double *src = xs + (size_t)j0 * ND;
        for (int e = tid; e < cnt * ND; e += rows) sx[e] = src[e];
        __syncthreads();
        for (int jj = 0; jj < cnt; ++jj) {
            double col[ND];
#pragma unroll
            for (int c = 0; c < ND; ++c) col[c] = sx[jj * ND + c];
            const unsigned long long key = (unsigned long long)__double_as_longlong(lof_d2<ND>(row, col));
            if (key < kth && j0 + jj != i) {                                    // the root falls out: the column sinks in from there
                const int jn = j0 + jj;
                unsigned long long top = key;
                int p = 0;
                for (int c = 1; c < k; c = 2 * p + 1) {
                    unsigned long long kc = lkey[c * rows + tid];
                    int jc = lidx[c * rows + tid];
                    if (c + 1 < k) {                                            // the larger of the two children
                        const unsigned long long ks = lkey[(c + 1) * rows + tid];
                        const int js = lidx[(c + 1) * rows + tid];
                        if (ks > kc || (ks == kc && js > jc)) { kc = ks; jc = js; ++c; }
                    }
                    if (kc < key || (kc == key && jc < jn)) break;              // both lie before the column: it stays here
                    lkey[p * rows + tid] = kc;
                    lidx[p * rows + tid] = (unsigned short)jc;
                    if (p == 0) top = kc;
                    p = c;
                }
                lkey[p * rows + tid] = key;
                lidx[p * rows + tid] = (unsigned short)jn;
                kth = top;
            }
        }
    }
    __syncthreads();
    const int nval = npts - r0 < rows ? npts - r0 : rows;                       // the block's rows that exist, at least one
    const size_t base = ((size_t)set * npts + r0) * k;
    for (int e = tid; e < nval * k; e += rows) {                                // an entry's place in its row's order: the entries before it
        const int r = e / k, m = e - r * k;
        const unsigned long long key = lkey[m * rows + r];
        const int idx = lidx[m * rows + r];
        int rank = 0;
        for (int q = 0; q < k; ++q) {
            const unsigned long long kq = lkey[q * rows + r];
            rank += (kq < key || (kq == key && (int)lidx[q * rows + r] < idx)) ? 1 : 0;
        }
        nbr[base + (size_t)r * k + rank] = idx;
        dist[base + (size_t)r * k + rank] = sqrt(__longlong_as_double((long long)key));
    }
    if (valid) kdist[(size_t)set * npts + i] = sqrt(__longlong_as_double((long long)kth));
}

// one thread per point p of all sets; its set begins at point p - p % npts
__global__ void __launch_bounds__(LOF_BLOCK)
nm_lof_lrd_kernel(int n, int npts, int k, const int *__restrict__ nbr, const double *__restrict__ dist, const double *__restrict__ kdist,
                  double *__restrict__ lrd)
{
    const int p = blockIdx.x * LOF_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int s0 = p - p % npts;
    double sum = 0.0;
    for (int m = 0; m < k; ++m) {
        const double d = dist[(size_t)p * k + m], kd = kdist[s0 + nbr[(size_t)p * k + m]];
        sum = sum + (d > kd ? d : kd);
    }
    lrd[p] = 1.0 / (sum / (double)k + LOF_FLOOR);
}

__global__ void __launch_bounds__(LOF_BLOCK)
nm_lof_lof_kernel(int n, int npts, int k, const int *__restrict__ nbr, const double *__restrict__ lrd, double *__restrict__ lof)
{
    const int p = blockIdx.x * LOF_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int s0 = p - p % npts;
    const double mine = lrd[p];
    double sum = 0.0;
    for (int m = 0; m < k; ++m) sum = sum + lrd[s0 + nbr[(size_t)p * k + m]] / mine;
    lof[p] = sum / (double)k;
}

} // namespace nm
