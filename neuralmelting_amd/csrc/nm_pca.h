// nm_pca.h — the kernels of the principal component stage (include/nm_pca.h: the definitions).  The samples x[n][j] are float32,
// row-major, and reach the device in batches of PCA_BATCH samples; every kernel works on one batch and carries its result on to
// the next, so the arithmetic is the same whether x stays on the device or is uploaded again.
//
//   nm_pca_colsum_kernel   one workgroup per (64 columns, chunk of PCA_MCH samples of the batch): a thread owns one column and every
//                          fourth sample, sums them in float64 in order, keeps the smallest and largest value and the first sample
//                          that is not finite; the four threads of a column are joined in LDS in order: one partial per (chunk, column).
//   nm_pca_coljoin_kernel  one thread per column: the batch's chunks are added to the running column sum in chunk order; behind the
//                          last batch mean = sum / N.
//   nm_pca_gram_kernel     one workgroup (4 waves) per (tile of PCA_TILE x PCA_TILE entries of the upper triangle, slice s of the batch):
//                          slice s holds the samples s PCA_SL .. (s + 1) PCA_SL - 1 of every batch.  PCA_KC samples at a time, the
//                          tile's two column blocks are read, converted to float64, centred and written to LDS once (feature and
//                          sample positions past the end as exact zeros of the CENTRED value), the next PCA_KC are already on their
//                          way into registers, and each wave accumulates its 32 x 32 quarter as 2 x 2 blocks of
//                          v_mfma_f64_16x16x4_f64.  The accumulators start from the slice's partial of the batch before, so a
//                          slice is one chain of fused multiply-adds over all its samples in sample order.
//                          Operands: A[i = lane & 15][k = lane >> 4] and B[k = lane >> 4][j = lane & 15], one double per lane, both
//                          read from LDS as s[k][column].  Result: register r of a lane is entry (row = (lane >> 4) + 4 r, col =
//                          lane & 15) of the 16 x 16 block - not the float32 instruction's map.
//   nm_pca_gramsum_kernel  gram[i][j] = the slices' partials added in slice order, for i <= j, written to [i][j] and [j][i]: of a
//                          diagonal tile only the upper half is used, so the mirror holds bit for bit.
//   nm_pca_project_kernel  one wave per PCA_PS samples, lanes over features: y = (x - mean) inv_scale once per feature, PCA_PC
//                          components at a time as fused multiply-adds per lane in feature order, then a butterfly over the lanes.
//
// Nothing here depends on the device: the chunk, the slice, the batch and the tile are constants, every sum has one order, and
// the only atomic is an integer minimum (the first sample that is not finite).
//
// Error bound (u = 2^-53; sums below are over the exact values; k u stands for k u / (1 - k u)).  A float32 converts to float64
// exactly.  A value that passes through k roundings, each relative, is off by at most k u of itself; in a sum every term
// passes through the additions on its way to the result and through its own roundings before.
//   mean     a thread adds at most PCA_MCH / 4 samples (255 additions), the column's four threads 3, the chunks ceil(N / PCA_MCH)
//            (the first one to an exact 0), the division 1; no summation of N terms has a path of more than N - 1 additions:
//            |d mean[j]| <= (min(N - 1, 258 + ceil(N / PCA_MCH)) + 1) u (sum_n |x[n][j]|) / N            <= (N + 2) u (...) / N.
//   gram     a = x - mean: one rounding, so a_i a_j carries 2.  A slice is one chain of fused multiply-adds (one rounding each,
//            the instruction's four products enter in k order) over its M_s samples; the slices that hold samples are added
//            in order.  With M = the largest M_s <= min(N, ceil(N / PCA_BATCH) PCA_SL) and S = min(PCA_SLICES, ceil(N / PCA_SL)):
//            |d gram[i][j]| <= (M + S + 1) u sum_n |a_i a_j|                                                <= (N + 8) u (...),
//            about N / 8 + 9 at large N.  (`a` is centred on the returned mean, as the definition says: the mean's own error is no
//            part of this.)  A column of N <= 2^29 equal values c has mean == c exactly (m c fits the 53 bits for every m <= 2^29,
//            so every partial sum and the division are exact): its centred value, and with it its row of gram, is exactly 0.
//   z        y_j = (x - mean) inv_scale: 2 roundings.  A lane adds ceil(D / 64) products by fused multiply-add, the butterfly adds 6
//            (additions of exact zeros do not round, and no path has more than D roundings):
//            |d z[n][c]| <= (min(D, ceil(D / 64) + 6) + 2) u sum_j |y_j comp[c][j]|                         <= (D + 2) u (...).
//   norm2    y_j^2 carries 4: |d norm2[n]| <= (min(D, ceil(D / 64) + 6) + 4) u norm2[n]                     <= (D + 4) u norm2.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nm {

constexpr int PCA_BLOCK = 256;
constexpr int PCA_TILE = 64;                        // features per side of a Gram tile: 4 waves x (2 x 2 blocks of 16 x 16)
constexpr int PCA_KC = 16;                          // samples staged in LDS at a time: four steps of the instruction's K = 4
constexpr int PCA_LD = PCA_TILE + 16;               // doubles per staged sample: rows k and k + 1 of a half-wave's read fall on the two halves of the banks
constexpr int PCA_SL = 4096;                        // samples of a slice within one batch
constexpr int PCA_SLICES = 8;                       // slices: 231 tiles x 8 = 1848 workgroups at 1331 features
constexpr int PCA_BATCH = PCA_SL * PCA_SLICES;      // samples uploaded and processed at a time: 32768 (174 MB at 1331 features)
constexpr int PCA_MCH = 1024;                       // samples per chunk of the column sums
constexpr int PCA_MAXFEAT = 4096;
constexpr int PCA_MAXCOMP = 64;
constexpr int PCA_PS = 4;                           // samples a wave projects at a time
constexpr int PCA_PC = 8;                           // components per sweep over the features
constexpr unsigned long long PCA_NOBAD = ~0ull;     // no sample that is not finite

typedef double pca_d4 __attribute__((ext_vector_type(4)));

static_assert(PCA_BATCH % PCA_MCH == 0 && PCA_SL % PCA_KC == 0 && PCA_KC % 4 == 0 && PCA_TILE == 64 && PCA_BLOCK == 256, "the kernels' index arithmetic");

// x: the batch, nb samples, of which the first is sample `first` of the call.  part: [chunks of the batch][nfeat].
__global__ void __launch_bounds__(PCA_BLOCK)
nm_pca_colsum_kernel(const float *__restrict__ x, int nb, int nfeat, int64_t first, double *__restrict__ part, float *__restrict__ plo,
                     float *__restrict__ phi, unsigned long long *__restrict__ bad)
{
    __shared__ double ss[4][64];
    __shared__ float slo[4][64], shi[4][64];
    const int c = threadIdx.x & 63, r = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + c;
    const int n0 = blockIdx.y * PCA_MCH;
    const int n1 = (nb - n0) < PCA_MCH ? nb : n0 + PCA_MCH;
    double s = 0.0;
    float lo = INFINITY, hi = -INFINITY;
    unsigned long long firstbad = PCA_NOBAD;
    if (j < nfeat)
        for (int n = n0 + r; n < n1; n += 4) {
            const float v = x[(int64_t)n * nfeat + j];
            if (!isfinite(v) && firstbad == PCA_NOBAD) firstbad = (unsigned long long)(first + n);
            s += (double)v;
            lo = fminf(lo, v);
            hi = fmaxf(hi, v);
        }
    if (firstbad != PCA_NOBAD) atomicMin(bad, firstbad);
    ss[r][c] = s;
    slo[r][c] = lo;
    shi[r][c] = hi;
    __syncthreads();
    if (r == 0 && j < nfeat) {
        for (int q = 1; q < 4; ++q) {
            s += ss[q][c];
            lo = fminf(lo, slo[q][c]);
            hi = fmaxf(hi, shi[q][c]);
        }
        const int64_t o = (int64_t)blockIdx.y * nfeat + j;
        part[o] = s;
        plo[o] = lo;
        phi[o] = hi;
    }
}

// sum, lo, hi [nfeat]: the running values (start: 0, +inf, -inf); with n > 0 (the last batch) mean = sum / n
__global__ void __launch_bounds__(PCA_BLOCK)
nm_pca_coljoin_kernel(int nchunks, int nfeat, const double *__restrict__ part, const float *__restrict__ plo, const float *__restrict__ phi,
                      double *__restrict__ sum, double *__restrict__ lo, double *__restrict__ hi, int64_t n, double *__restrict__ mean)
{
    const int j = blockIdx.x * PCA_BLOCK + threadIdx.x;
    if (j >= nfeat) return;
    double s = sum[j], l = lo[j], h = hi[j];
    for (int q = 0; q < nchunks; ++q) {
        const int64_t o = (int64_t)q * nfeat + j;
        s += part[o];
        l = fmin(l, (double)plo[o]);
        h = fmax(h, (double)phi[o]);
    }
    sum[j] = s;
    lo[j] = l;
    hi[j] = h;
    if (n > 0) mean[j] = s / (double)n;
}

// tile t of the upper triangle of a tiles x tiles grid, row by row: (ti, tj), ti <= tj
__device__ __forceinline__ void pca_tile_of(int t, int tiles, int &ti, int &tj)
{
    ti = 0;
    while (t >= tiles - ti) {
        t -= tiles - ti;
        ++ti;
    }
    tj = ti + t;
}

// the centred float64 value of sample n (of the batch), feature j; an exact 0 past the slice's end n1 or the last feature
__device__ __forceinline__ double pca_centred(const float *__restrict__ x, int nfeat, int n, int n1, int j, double mean)
{
    return (n < n1 && j < nfeat) ? (double)x[(int64_t)n * nfeat + j] - mean : 0.0;
}

// part: [PCA_SLICES][tiles of the upper triangle][PCA_TILE][PCA_TILE], zero before the first batch; one workgroup per (tile, slice)
__global__ void __launch_bounds__(PCA_BLOCK)
nm_pca_gram_kernel(const float *__restrict__ x, int nb, int nfeat, const double *__restrict__ mean, double *__restrict__ part)
{
    __shared__ double sa[PCA_KC * PCA_LD], sb[PCA_KC * PCA_LD];
    // consecutive workgroups are dealt out over the dies in turn: with the slice as the fastest index a die's workgroups share
    // one slice's samples in its L2
    const int slice = blockIdx.x % PCA_SLICES, tile = blockIdx.x / PCA_SLICES, ntri = gridDim.x / PCA_SLICES;
    const int n0 = slice * PCA_SL;
    if (n0 >= nb) return;                                       // the slice holds nothing of this batch: its partial stays
    const int n1 = (nb - n0) < PCA_SL ? nb : n0 + PCA_SL;
    const int tiles = (nfeat + PCA_TILE - 1) / PCA_TILE;
    int ti, tj;
    pca_tile_of(tile, tiles, ti, tj);
    const bool diag = ti == tj;
    const double *__restrict__ sB = diag ? sa : sb;

    const int c = threadIdx.x & 63, r = threadIdx.x >> 6;       // staging: column c of both blocks, samples r, r + 4, r + 8, r + 12
    const int ja = ti * PCA_TILE + c, jb = tj * PCA_TILE + c;
    const double ma = ja < nfeat ? mean[ja] : 0.0, mb = jb < nfeat ? mean[jb] : 0.0;

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, lk = lane >> 4;
    const int ra = (wave >> 1) * 32 + lc, cb = (wave & 1) * 32 + lc; // the wave's quarter: rows of block A, columns of block B

    double *__restrict__ p = part + ((size_t)slice * ntri + tile) * (PCA_TILE * PCA_TILE);
    pca_d4 acc[2][2];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                acc[bi][bj][q] = p[((wave >> 1) * 32 + bi * 16 + lk + 4 * q) * PCA_TILE + (wave & 1) * 32 + bj * 16 + lc];

    double va[4], vb[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        va[q] = pca_centred(x, nfeat, n0 + r + 4 * q, n1, ja, ma);
        vb[q] = diag ? 0.0 : pca_centred(x, nfeat, n0 + r + 4 * q, n1, jb, mb);
    }
    for (int n = n0; n < n1; n += PCA_KC) {
        __syncthreads();                                        // the samples before these have been read
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            sa[(r + 4 * q) * PCA_LD + c] = va[q];
            if (!diag) sb[(r + 4 * q) * PCA_LD + c] = vb[q];
        }
        __syncthreads();
        if (n + PCA_KC < n1) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                va[q] = pca_centred(x, nfeat, n + PCA_KC + r + 4 * q, n1, ja, ma);
                vb[q] = diag ? 0.0 : pca_centred(x, nfeat, n + PCA_KC + r + 4 * q, n1, jb, mb);
            }
        }
#pragma unroll
        for (int kk = 0; kk < PCA_KC; kk += 4) {
            const double a0 = sa[(kk + lk) * PCA_LD + ra], a1 = sa[(kk + lk) * PCA_LD + ra + 16];
            const double b0 = sB[(kk + lk) * PCA_LD + cb], b1 = sB[(kk + lk) * PCA_LD + cb + 16];
            acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj)
#pragma unroll
            for (int q = 0; q < 4; ++q)
                p[((wave >> 1) * 32 + bi * 16 + lk + 4 * q) * PCA_TILE + (wave & 1) * 32 + bj * 16 + lc] = acc[bi][bj][q];
}

// one workgroup per tile of the upper triangle; gram [nfeat][nfeat]
__global__ void __launch_bounds__(PCA_BLOCK)
nm_pca_gramsum_kernel(int nfeat, const double *__restrict__ part, double *__restrict__ gram)
{
    const int tiles = (nfeat + PCA_TILE - 1) / PCA_TILE;
    int ti, tj;
    pca_tile_of(blockIdx.x, tiles, ti, tj);
    for (int e = threadIdx.x; e < PCA_TILE * PCA_TILE; e += PCA_BLOCK) {
        const int i = ti * PCA_TILE + e / PCA_TILE, j = tj * PCA_TILE + e % PCA_TILE;
        if (i > j || j >= nfeat) continue;                      // (i <= j < nfeat; below the diagonal only in a diagonal tile)
        double s = part[(size_t)blockIdx.x * (PCA_TILE * PCA_TILE) + e];
        for (int q = 1; q < PCA_SLICES; ++q) s += part[((size_t)q * gridDim.x + blockIdx.x) * (PCA_TILE * PCA_TILE) + e];
        gram[(size_t)i * nfeat + j] = s;
        gram[(size_t)j * nfeat + i] = s;
    }
}

// the same value in every lane, in a fixed order
__device__ __forceinline__ double pca_wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// x: the batch of nb samples (the first is sample `first` of the call); z [nb][ncomp] and norm2 [nb] (or null) are the batch's
__global__ void __launch_bounds__(PCA_BLOCK)
nm_pca_project_kernel(const float *__restrict__ x, int nb, int nfeat, int64_t first, const double *__restrict__ mean,
                      const double *__restrict__ inv_scale, int ncomp, const double *__restrict__ comp, double *__restrict__ z,
                      double *__restrict__ norm2, unsigned long long *__restrict__ bad)
{
    const int lane = threadIdx.x & 63;
    const int n0 = (blockIdx.x * (PCA_BLOCK / 64) + (threadIdx.x >> 6)) * PCA_PS;
    if (n0 >= nb) return;
    unsigned long long firstbad = PCA_NOBAD;
    for (int c0 = 0; c0 < ncomp; c0 += PCA_PC) {
        double acc[PCA_PC][PCA_PS], nn[PCA_PS];
#pragma unroll
        for (int s = 0; s < PCA_PS; ++s) {
            nn[s] = 0.0;
#pragma unroll
            for (int c = 0; c < PCA_PC; ++c) acc[c][s] = 0.0;
        }
        for (int j = lane; j < nfeat; j += 64) {
            const double m = mean[j], w = inv_scale[j];
            double y[PCA_PS];
#pragma unroll
            for (int s = 0; s < PCA_PS; ++s) {
                const float v = n0 + s < nb ? x[(int64_t)(n0 + s) * nfeat + j] : 0.0f;
                if (!isfinite(v) && firstbad == PCA_NOBAD) firstbad = (unsigned long long)(first + n0 + s);
                y[s] = ((double)v - m) * w;
                nn[s] = fma(y[s], y[s], nn[s]);
            }
#pragma unroll
            for (int c = 0; c < PCA_PC; ++c) {
                const double e = c0 + c < ncomp ? comp[(int64_t)(c0 + c) * nfeat + j] : 0.0;
#pragma unroll
                for (int s = 0; s < PCA_PS; ++s) acc[c][s] = fma(y[s], e, acc[c][s]);
            }
        }
#pragma unroll
        for (int s = 0; s < PCA_PS; ++s) {
            if (n0 + s >= nb) break;
#pragma unroll
            for (int c = 0; c < PCA_PC; ++c) {
                const double v = pca_wave_sum(acc[c][s]);
                if (lane == 0 && c0 + c < ncomp) z[(int64_t)(n0 + s) * ncomp + c0 + c] = v;
            }
            if (c0 == 0 && norm2) {
                const double v = pca_wave_sum(nn[s]);
                if (lane == 0) norm2[n0 + s] = v;
            }
        }
    }
    if (firstbad != PCA_NOBAD) atomicMin(bad, firstbad);
}

} // namespace nm
