// nm_distr.h — histogram kernels for lammps_distr.py's calculate_rdf / calculate_cdf (lammps_distr.py:123-171).
// One workgroup per (sample, periodic image): positions staged in LDS, float32 displacement arithmetic identical to
// numpy's (no contraction), float64 edge comparisons, integer counts in LDS, one float atomic (exact below 2^24) per non-empty bin
// at the end; the host refuses a result with a count of 2^24 or more.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "nm_math.h"

namespace nm {

constexpr int DISTR_BLOCK = 256;
constexpr int DISTR_MAXS = 256;  // most spherical bin edges
constexpr int DISTR_MAXC = 32;   // most cartesian bins per axis

// nm_distr_kernel's LDS: the positions and their shifted, padded copy (distr_pos_bytes, rounded up for the float64 edges behind
// them), the edges of both histograms, the counts
__host__ __device__ inline size_t distr_pos_bytes(int natoms)
{
    return ((size_t)3 * (natoms + ((natoms + 63) & ~63)) * sizeof(float) + 7) & ~(size_t)7;
}

__host__ __device__ inline size_t distr_lds_bytes(int natoms, int sbins, int cbins)
{
    return distr_pos_bytes(natoms) + (size_t)(sbins + cbins + 1) * sizeof(double)
         + ((size_t)sbins + (size_t)cbins * cbins * cbins) * sizeof(unsigned int);
}

// np.histogram with explicit edges: bin k holds e[k] <= d < e[k+1], the last bin also d == e[n-1]; -1 = outside
__device__ __forceinline__ int bin_of(const double *e, int n, double d)
{
    if (!(d >= e[0]) || !(d <= e[n - 1])) return -1;
    int lo = 0, hi = n - 1; // invariant: e[lo] <= d, d < e[hi] or hi == n-1
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (d >= e[mid]) lo = mid; else hi = mid;
    }
    return lo; // d == e[n-1] ends in the last bin n-2
}

// the same bin found from a guess: the reference's edges are np.linspace grids, so (d - e[0]) * inv lands on the right bin or
// next to it, and the walk below ends after zero or one step; it is exact for any increasing edges
__device__ __forceinline__ int bin_near(const double *e, int n, double d, double inv)
{
    const double e0 = e[0];
    if (!(d >= e0) || !(d <= e[n - 1])) return -1;
    int k = (int)((d - e0) * inv);
    k = k < 0 ? 0 : (k > n - 2 ? n - 2 : k);
    if (d < e[k]) { do --k; while (d < e[k]); } // stops at k >= 0: e[0] <= d
    else while (k < n - 2 && d >= e[k + 1]) ++k;
    return k;
}

// A pair contributes only if its displacement lies inside the cube |d| <= l/2 (the sphere r <= l/2 of the radial histogram
// sits inside it): 1/27 of all (pair, image) combinations.  The loop over b therefore runs a cheap float pre-test over 64
// candidates at a time, collecting the survivors of each lane in a bit mask, and only then walks the set bits through the exact
// path (float32 arithmetic as numpy, float64 edge searches, LDS atomics).  The pre-test is conservative: `cube` is a float
// strictly outside every edge of both histograms, so a rejected candidate is outside in the exact comparison too.
__global__ void __launch_bounds__(DISTR_BLOCK)
nm_distr_kernel(int natoms, const float *__restrict__ pos, const float *__restrict__ box, int sbins,
                const double *__restrict__ r_edges, int cbins, const double *__restrict__ rv_edges,
                float *__restrict__ rdf_cnt, float *__restrict__ cdf_cnt)
{
#pragma clang fp contract(off)
    extern __shared__ __align__(16) unsigned char smem[];
    const int s = blockIdx.x / 27, img = blockIdx.x % 27;
    const int tid = threadIdx.x;
    // br[j] = (b[i], b[j], b[k]) for i, j, k in range(3), b = [-1, 0, 1]  (lammps_distr.py:99-102)
    const float bx = (float)(img / 9 - 1), by = (float)((img / 3) % 3 - 1), bz = (float)(img % 3 - 1);
    const int npad = (natoms + 63) & ~63;
    float *px = (float *)smem, *py = px + natoms, *pz = py + natoms;
    float *qx = pz + natoms, *qy = qx + npad, *qz = qy + npad; // pos[b] + box*br, padded with far-away entries
    double *re = (double *)(smem + distr_pos_bytes(natoms));
    double *ve = re + sbins;
    unsigned int *hr = (unsigned int *)(ve + (cbins + 1));
    unsigned int *hc = hr + sbins;
    const int nc = cbins * cbins * cbins;
    const float L = box[s];
    const float *ps = pos + (size_t)s * natoms * 3;
    const float sx = L * bx, sy = L * by, sz = L * bz; // box*br[j]
    for (int a = tid; a < npad; a += DISTR_BLOCK) {
        if (a < natoms) {
            const float x = ps[3 * a], y = ps[3 * a + 1], z = ps[3 * a + 2];
            px[a] = x; py[a] = y; pz[a] = z;
            qx[a] = x + sx; qy[a] = y + sy; qz[a] = z + sz;
        } else { qx[a] = 3.0e38f; qy[a] = 3.0e38f; qz[a] = 3.0e38f; }
    }
    for (int k = tid; k < sbins; k += DISTR_BLOCK) { re[k] = r_edges[k]; hr[k] = 0u; }
    const bool do_r = rdf_cnt != nullptr, do_c = cdf_cnt != nullptr;
    // an rdf-only call passes cbins = 0 and no cdf edges: nothing to stage then (ve[0] would be read from a null pointer)
    if (do_c)
        for (int k = tid; k <= cbins; k += DISTR_BLOCK) ve[k] = rv_edges[k];
    for (int k = tid; k < nc; k += DISTR_BLOCK) hc[k] = 0u;
    __syncthreads();
    double far = 0.0;
    if (do_r) far = fmax(far, fmax(fabs(re[0]), fabs(re[sbins - 1])));
    if (do_c) far = fmax(far, fmax(fabs(ve[0]), fabs(ve[cbins])));
    const double rinv = do_r ? (double)(sbins - 1) / (re[sbins - 1] - re[0]) : 0.0;
    const double vinv = do_c ? (double)cbins / (ve[cbins] - ve[0]) : 0.0;
    const float cube = nextafterf(nextafterf((float)far, 3.0e38f), 3.0e38f); // > every edge in magnitude, also after the cast's rounding
    // dvm[b][a] = pos[a] - (pos[b] + box*br): thread = a, loop over b (LDS broadcast reads)
    for (int a = tid; a < natoms; a += DISTR_BLOCK) {
        const float xa = px[a], ya = py[a], za = pz[a];
        for (int b0 = 0; b0 < npad; b0 += 64) {
            unsigned long long mask = 0ull;
#pragma unroll
            for (int j = 0; j < 64; ++j) {
                const float dx = xa - qx[b0 + j], dy = ya - qy[b0 + j], dz = za - qz[b0 + j];
                const float m = fmaxf(fmaxf(fabsf(dx), fabsf(dy)), fabsf(dz));
                mask |= (m <= cube) ? (1ull << j) : 0ull;
            }
            while (mask) {
                const int b = b0 + __ffsll((long long)mask) - 1;
                mask &= mask - 1ull;
                const float dx = xa - qx[b], dy = ya - qy[b], dz = za - qz[b];
                if (do_r) {
                    float d2 = dx * dx;      // np.sum(np.square(dvm), -1): sequential float32 sum of three terms
                    d2 = d2 + dy * dy;
                    d2 = d2 + dz * dz;
                    // np.sqrt is correctly rounded; so is sqrtf under hipcc's default fp32 sqrt, while __fsqrt_rn is
                    // the bare v_sqrt_f32 (1 ulp), which moves a pair next to an edge into the neighbouring bin
                    const float d = sqrtf(d2);
                    const int k = bin_near(re, sbins, (double)d, rinv);
                    if (k >= 0) atomicAdd(&hr[k + 1], 1u);
                }
                if (do_c) {
                    // np.histogramdd: bin = (#edges <= x) - 1, a value on the last edge goes to the last bin, outside is dropped
                    const int kx = bin_near(ve, cbins + 1, (double)dx, vinv), ky = bin_near(ve, cbins + 1, (double)dy, vinv),
                              kz = bin_near(ve, cbins + 1, (double)dz, vinv);
                    if (kx >= 0 && ky >= 0 && kz >= 0) atomicAdd(&hc[(kx * cbins + ky) * cbins + kz], 1u);
                }
            }
        }
    }
    __syncthreads();
    // the 27 image blocks of a sample meet in global memory.  A block's own count is at most natoms^2 < 2^24 and exact as a
    // float; the float atomics are exact as long as the sum stays below 2^24, and the host refuses a result that reaches it
    // (displacements on +-l/2 count in two images per axis, so a bin can exceed natoms^2).  Below that, the result is what
    // the reference holds in its float32 `rd` / `cd` arrays before the division by natoms
    if (do_r)
        for (int k = tid; k < sbins; k += DISTR_BLOCK) if (hr[k]) atomicAdd(&rdf_cnt[(size_t)s * sbins + k], (float)hr[k]);
    if (do_c)
        for (int k = tid; k < nc; k += DISTR_BLOCK) if (hc[k]) atomicAdd(&cdf_cnt[(size_t)s * nc + k], (float)hc[k]);
}

// ---------------------------------------------------------------------------------------------------------------
// What the kernels over a neighbour shell share (nm_adf_kernel, nm_bo_moments_kernel, nm_bo_average_kernel).  A workgroup of
// SHELL_BLOCK threads takes SHELL_CPB consecutive centres of one sample and stages the sample's positions and their bounding box
// in LDS once (shell_stage, shell_bounds); each wave then works through its centres on its own and finds a centre's neighbours
// with shell_scan.  That scan is the one place where a neighbour is decided, so the entries of the bond order are those of the
// angular distribution by construction (include/nm_distr.h).
constexpr int SHELL_BLOCK = 256;
constexpr int SHELL_WAVES = SHELL_BLOCK / 64;
constexpr int SHELL_CPB = 32;   // centres per workgroup

// A wave's lanes exchange the neighbour tiles through LDS without a workgroup barrier: a wave's LDS operations complete in
// program order, and this keeps the compiler from moving them across the hand-over.
__device__ __forceinline__ void adf_wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// a wave-uniform value in a scalar register
__device__ __forceinline__ float wave_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// Staging, first part: the sample's positions go to LDS, and every wave writes the bounding box of the atoms it copied to
// part[wave][lo x, hi x, lo y, hi y, lo z, hi z].  A workgroup barrier belongs between this and shell_bounds.
__device__ __forceinline__ void shell_stage(const float *ps, int natoms, float *px, float *py, float *pz, float *part)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float lo[3] = {3.0e38f, 3.0e38f, 3.0e38f}, hi[3] = {-3.0e38f, -3.0e38f, -3.0e38f};
    for (int a = tid; a < natoms; a += SHELL_BLOCK) {
        const float x = ps[3 * a], y = ps[3 * a + 1], z = ps[3 * a + 2];
        px[a] = x; py[a] = y; pz[a] = z;
        lo[0] = fminf(lo[0], x); hi[0] = fmaxf(hi[0], x);
        lo[1] = fminf(lo[1], y); hi[1] = fmaxf(hi[1], y);
        lo[2] = fminf(lo[2], z); hi[2] = fmaxf(hi[2], z);
    }
    for (int d = 0; d < 3; ++d) {
        for (int o = 32; o > 0; o >>= 1) {
            lo[d] = fminf(lo[d], __shfl_xor(lo[d], o));
            hi[d] = fmaxf(hi[d], __shfl_xor(hi[d], o));
        }
        if (lane == 0) { part[wave * 6 + 2 * d] = lo[d]; part[wave * 6 + 2 * d + 1] = hi[d]; }
    }
}

// Staging, second part: the sample's bounding box from the waves' partials, in every thread's registers
__device__ __forceinline__ void shell_bounds(const float *part, float *bb)
{
    for (int d = 0; d < 3; ++d) {
        float l = part[2 * d], u = part[2 * d + 1];
        for (int w = 1; w < SHELL_WAVES; ++w) { l = fminf(l, part[w * 6 + 2 * d]); u = fmaxf(u, part[w * 6 + 2 * d + 1]); }
        bb[2 * d] = l; bb[2 * d + 1] = u;
    }
}

// The neighbour scan: the candidates of centre (cx, cy, cz) are the 27 images x natoms atoms, image-major, walked by a wave 64
// atoms at a time (lane = atom a0 + lane).  A candidate is a neighbour if its float32 displacement length d, numpy's arithmetic
// (no contraction, sequential sum, correctly rounded root), has r_lo < (double)d <= r_hi.  An image whose shift puts the whole
// sample outside the cube |component| <= cube around the centre is skipped.  After each 64 candidates the scan calls
// sink(a, in, vx, vy, vz, ballot): the lane's atom, whether it is a neighbour, its displacement, and the wave's ballot of `in`,
// whose set bits below the lane number the neighbours in scan order.  The scan goes on while sink returns true.
template <class F>
__device__ __forceinline__ void shell_scan(const float *px, const float *py, const float *pz, int natoms, float cx, float cy, float cz,
                                           float L, float cube, const float *bb, double r_lo, double r_hi, int lane, F &&sink)
{
#pragma clang fp contract(off)
    for (int img = 0; img < 27; ++img) {
        // br[j] = (b[i], b[j], b[k]) for i, j, k in range(3), b = [-1, 0, 1]  (lammps_distr.py:99-102)
        const float bx = (float)(img / 9 - 1), by = (float)((img / 3) % 3 - 1), bz = (float)(img % 3 - 1);
        const float qx = cx + L * bx, qy = cy + L * by, qz = cz + L * bz; // pos[c] + box*br[j]
        // float subtraction is monotone, so every atom's component lies between those of the bounding box; a component beyond
        // cube >= r_hi in magnitude gives d >= |component| > r_hi (sqrt(x*x) rounds to |x|, the further terms only add)
        if (bb[0] - qx > cube || bb[1] - qx < -cube || bb[2] - qy > cube || bb[3] - qy < -cube || bb[4] - qz > cube || bb[5] - qz < -cube)
            continue;
        for (int a0 = 0; a0 < natoms; a0 += 64) {
            const int a = a0 + lane;
            bool in = false;
            float vx = 0.0f, vy = 0.0f, vz = 0.0f;
            if (a < natoms) {
                vx = px[a] - qx; vy = py[a] - qy; vz = pz[a] - qz;
                float d2 = vx * vx;      // sequential float32 sum of three terms, as the rdf path
                d2 = d2 + vy * vy;
                d2 = d2 + vz * vz;
                const double d = (double)sqrtf(d2); // correctly rounded (see nm_distr_kernel)
                in = r_lo < d && d <= r_hi;
            }
            if (!sink(a, in, vx, vy, vz, __ballot(in))) return;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Angular distribution (include/nm_distr.h, nm_distr_angles): for every centre atom c the angle between every unordered
// pair of its neighbours, a neighbour being an (image, atom) whose float32 displacement length lies in (r_lo, r_hi].
//
// A workgroup takes SHELL_CPB consecutive centres of one sample; the sample's positions are staged in LDS once.  Each wave
// works through its centres on its own (no workgroup barrier after the staging):
//   scan   shell_scan's neighbours are appended to the wave's LDS neighbour list (ballot + prefix count): the float32
//          components and 1/|v| in float64.
//   pairs  every unordered pair of the list, spread evenly over the lanes (the numbering is given at the loop), binned in cosine
//          space into one of ADF_REP copies of the wave's LDS histogram (crystal frames put nearly all counts into four
//          bins; the copies cut that contention by ADF_REP).
//   tiles  a list longer than ADF_TILE is processed in tiles: tile A against itself, then against every later tile B,
//          which is produced by scanning again.  Any number of neighbours is handled.
// The LDS histograms are 32-bit; a wave adds them to the 64-bit global counts before they could overflow and at its end.
constexpr int ADF_TILE = 256;   // neighbours per LDS tile (two tiles per wave)
constexpr int ADF_REP = 4;      // copies of a wave's histogram, chosen by lane
constexpr int ADF_LUT = 4096;   // cells of the bin-guess table over cos(theta) in [-1, 1]
constexpr int ADF_MAXB = 256;   // most edges (a bin index fits the table's bytes)
static_assert(ADF_LUT % SHELL_BLOCK == 0 && ADF_MAXB <= 256, "each thread fills ADF_LUT / SHELL_BLOCK cells with byte-sized bins");

// The estimate est = dot * (r1 * r2), r_i = 1 / sqrt(n_i), against the definition's cth = clip(dot / sqrt(n1 * n2)):
// with u = 2^-53 and every operation correctly rounded, cth carries a relative error of at most (1/2 + 1 + 1) u = 2.5 u
// against the real quotient t (the product, its root, the division); r_i carries 2 u (root, reciprocal), r1 * r2 5 u and est
// 6 u.  No operand can underflow or overflow: the n_i are sums of squares of float32 values, not all zero, so they lie in
// [2^-298, 2^257].  |t| <= 1 up to the rounding of dot and n_i (a few u), so |est - cth| < 9 u (1 + 4 u) < 2^-49, and
// ADF_MARGIN = 2^-48 is twice that.  If no edge lies within the margin of est and |est| < 1 - margin (so that the clip is
// the identity), est and cth lie strictly between the same two edges, or outside on the same side: same bin.  Otherwise the
// definition's expression is evaluated.
constexpr double ADF_MARGIN = 0x1p-48;

__host__ __device__ inline size_t adf_lds_bytes(int natoms, int abins)
{
    return (size_t)(abins + 1 + SHELL_WAVES * 2 * ADF_TILE) * sizeof(double)                // edges and their sentinel, 1/|v| of the tiles
         + ((size_t)3 * natoms + (size_t)SHELL_WAVES * 2 * 3 * ADF_TILE + SHELL_WAVES * 6) * sizeof(float) // positions, tiles, bounding box partials
         + (size_t)SHELL_WAVES * ADF_REP * abins * sizeof(unsigned int) + ADF_LUT;           // histograms, guess table
}

// bin k (0 <= k <= n-2) holds e[k] >= c > e[k+1] for strictly decreasing e, the last bin also c == e[n-1]; -1 = outside.
// The walk starts from any k in [0, n-2] and is exact for every start.
__device__ __forceinline__ int adf_walk(const double *e, int n, double c, int k)
{
    if (!(c <= e[0]) || !(c >= e[n - 1])) return -1;
    while (k > 0 && c > e[k]) --k;            // now c <= e[k]
    while (k < n - 2 && c <= e[k + 1]) ++k;   // now k == n-2 or c > e[k+1]
    return k;
}

// The bin of one neighbour pair, -1 = dropped.  e holds one sentinel behind the last edge (e[n] = -inf), so the three edges
// around the guessed bin are read at once: the guess k0 = lut[cell of est] is the bin of the cell's largest value, and est lies in
// bin k0 or k0 + 1 unless the cell holds two edges.  If est is then inside its bin by more than the margin (see ADF_MARGIN), that
// is the definition's bin; everything else (an edge within the margin, a wrong guess, outside, |est| within the margin of 1)
// takes the general path: the walk, the margin test against the bin found, and the definition's own expression where it fails.
__device__ __forceinline__ int adf_bin(const double *e, int n, const unsigned char *lut, float x1, float y1, float z1, double r1,
                                       float x2, float y2, float z2, double r2)
{
    // float64 from the float32 components.  A product of two float32 is exact in float64, so the fma chain rounds exactly
    // where (x1*x2 + y1*y2) + z1*z2 does: the same bits.
    const double X1 = x1, Y1 = y1, Z1 = z1, X2 = x2, Y2 = y2, Z2 = z2;
    const double dot = fma(Z1, Z2, fma(Y1, Y2, X1 * X2));
    const double est = dot * (r1 * r2);
    int g = (int)((1.0 - est) * (double)(ADF_LUT / 2));
    g = g < 0 ? 0 : (g > ADF_LUT - 1 ? ADF_LUT - 1 : g);
    const int k0 = (int)lut[g];
    const double ea = e[k0], eb = e[k0 + 1], ec = e[k0 + 2];
    const bool up = est <= eb;
    const double hi = up ? eb : ea, lo = up ? ec : eb;
    int k = up ? k0 + 1 : k0;
    if (k <= n - 2 && hi - est > ADF_MARGIN && est - lo > ADF_MARGIN && fabs(est) < 1.0 - ADF_MARGIN) return k;
    k = adf_walk(e, n, est, k <= n - 2 ? k : n - 2);
    bool near = !(fabs(est) < 1.0 - ADF_MARGIN);
    if (k >= 0) near = near || e[k] - est <= ADF_MARGIN || est - e[k + 1] <= ADF_MARGIN;
    else near = near || (est > e[0] ? est - e[0] <= ADF_MARGIN : e[n - 1] - est <= ADF_MARGIN);
    if (near) {
        const double n1 = fma(Z1, Z1, fma(Y1, Y1, X1 * X1)), n2 = fma(Z2, Z2, fma(Y2, Y2, X2 * X2));
        double c = dot / sqrt(n1 * n2); // IEEE division and square root (hipcc's defaults for float64)
        c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
        k = adf_walk(e, n, c, k >= 0 ? k : (est > e[0] ? 0 : n - 2));
    }
    return k;
}

// One shell_scan of centre (cx, cy, cz): neighbours number t0 .. t0+ADF_TILE-1 (in scan order) go to the tile.
// Returns the number of neighbours seen; the scan ends early once that reaches `stop`.
__device__ __forceinline__ int adf_fill(const float *px, const float *py, const float *pz, int natoms, float cx, float cy, float cz,
                                        float L, float cube, const float *bb, double r_lo, double r_hi, int t0, int stop, float *tx,
                                        float *ty, float *tz, double *tr, int lane)
{
    int base = 0;
    shell_scan(px, py, pz, natoms, cx, cy, cz, L, cube, bb, r_lo, r_hi, lane,
               [&](int, bool in, float vx, float vy, float vz, unsigned long long m) {
        if (in) {
            const int o = base + __popcll(m & ((1ull << lane) - 1ull)) - t0;
            if (o >= 0 && o < ADF_TILE) {
                const double X = vx, Y = vy, Z = vz;
                tx[o] = vx; ty[o] = vy; tz[o] = vz;
                tr[o] = 1.0 / sqrt(fma(Z, Z, fma(Y, Y, X * X)));
            }
        }
        base += __popcll(m);
        return base < stop;
    });
    return base;
}

__global__ void __launch_bounds__(SHELL_BLOCK)
nm_adf_kernel(int natoms, const float *__restrict__ pos, const float *__restrict__ box, double r_lo, double r_hi, float cube,
              int abins, const double *__restrict__ cos_edges, unsigned long long *__restrict__ adf)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int groups = (natoms + SHELL_CPB - 1) / SHELL_CPB;
    const int s = blockIdx.x / groups, c0 = (blockIdx.x % groups) * SHELL_CPB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double *e = (double *)smem, *tr_all = e + abins + 1;
    float *px = (float *)(tr_all + SHELL_WAVES * 2 * ADF_TILE), *py = px + natoms, *pz = py + natoms;
    float *txyz_all = pz + natoms, *part = txyz_all + SHELL_WAVES * 2 * 3 * ADF_TILE;
    unsigned int *h_all = (unsigned int *)(part + SHELL_WAVES * 6);
    unsigned char *lut = (unsigned char *)(h_all + SHELL_WAVES * ADF_REP * abins);
    const float L = box[s];
    // stage the positions, their bounding box, the edges, the guess table; clear the histograms
    shell_stage(pos + (size_t)s * natoms * 3, natoms, px, py, pz, part);
    for (int k = tid; k <= abins; k += SHELL_BLOCK) e[k] = k < abins ? cos_edges[k] : -INFINITY;
    for (int k = tid; k < SHELL_WAVES * ADF_REP * abins; k += SHELL_BLOCK) h_all[k] = 0u;
    __syncthreads();
    {
        // the bin of each cell's largest value (cells in decreasing order of cos: the bin never decreases along a thread's
        // consecutive cells); a hint only, adf_bin is exact for any table
        int k = 0;
        for (int g = tid * (ADF_LUT / SHELL_BLOCK); g < (tid + 1) * (ADF_LUT / SHELL_BLOCK); ++g) {
            const double top = 1.0 - (double)g * (2.0 / ADF_LUT);
            while (k < abins - 2 && top <= e[k + 1]) ++k;
            lut[g] = (unsigned char)k;
        }
    }
    float bb[6];
    shell_bounds(part, bb);
    __syncthreads();
    // this wave's tiles and histogram copies
    float *ax = txyz_all + (size_t)wave * 2 * 3 * ADF_TILE, *ay = ax + ADF_TILE, *az = ay + ADF_TILE;
    float *bx = az + ADF_TILE, *by = bx + ADF_TILE, *bz = by + ADF_TILE;
    double *ar = tr_all + (size_t)wave * 2 * ADF_TILE, *br = ar + ADF_TILE;
    unsigned int *hw = h_all + (size_t)wave * ADF_REP * abins;
    unsigned int *h = hw + (lane & (ADF_REP - 1)) * abins;
    unsigned long long *out = adf + (size_t)s * abins;
    unsigned long long held = 0ull; // upper bound of the counts this wave's LDS histograms hold
    auto flush = [&]() {
        for (int k = lane; k < abins; k += 64) {
            unsigned long long t = 0ull;
            for (int r = 0; r < ADF_REP; ++r) { t += hw[r * abins + k]; hw[r * abins + k] = 0u; }
            if (t) atomicAdd(&out[k], t);
        }
        held = 0ull;
    };
    const int cend = c0 + SHELL_CPB < natoms ? c0 + SHELL_CPB : natoms;
    for (int c = c0 + wave; c < cend; c += SHELL_WAVES) {
        adf_wave_sync(); // the previous centre's pair loops are done with the tiles
        const float cx = wave_uniform(px[c]), cy = wave_uniform(py[c]), cz = wave_uniform(pz[c]);
        const int M = adf_fill(px, py, pz, natoms, cx, cy, cz, L, cube, bb, r_lo, r_hi, 0, 0x7fffffff, ax, ay, az, ar, lane);
        adf_wave_sync();
        const int nt = (M + ADF_TILE - 1) / ADF_TILE;
        for (int ta = 0; ta < nt; ++ta) {
            if (ta > 0) {
                adf_wave_sync(); // the pair loops of the previous tile are done with A
                adf_fill(px, py, pz, natoms, cx, cy, cz, L, cube, bb, r_lo, r_hi, ta * ADF_TILE, (ta + 1) * ADF_TILE, ax, ay, az, ar, lane);
                adf_wave_sync();
            }
            const int ma = M - ta * ADF_TILE < ADF_TILE ? M - ta * ADF_TILE : ADF_TILE;
            if (held + (unsigned long long)ADF_TILE * ADF_TILE > 0xffffffffull) flush();
            // all unordered pairs of the tile, each once: pair number q = (d - 1) * ma + i is (i, (i + d) mod ma) for the offsets
            // d = 1 .. ma/2 (for even ma the last offset only with i < ma/2): ma (ma - 1) / 2 pairs, lanes take q = lane, lane + 64, ..
            {
                const int Q = ma * (ma - 1) / 2;
                int d = 1 + lane / ma, i = lane % ma;
                for (int q = lane; q < Q; q += 64) {
                    const int j = i + d < ma ? i + d : i + d - ma;
                    const int k = adf_bin(e, abins, lut, ax[i], ay[i], az[i], ar[i], ax[j], ay[j], az[j], ar[j]);
                    if (k >= 0) atomicAdd(&h[k + 1], 1u);
                    i += 64;
                    while (i >= ma) { i -= ma; ++d; }
                }
                held += (unsigned long long)Q;
            }
            for (int tb = ta + 1; tb < nt; ++tb) {
                adf_wave_sync();
                adf_fill(px, py, pz, natoms, cx, cy, cz, L, cube, bb, r_lo, r_hi, tb * ADF_TILE, (tb + 1) * ADF_TILE, bx, by, bz, br, lane);
                adf_wave_sync();
                const int mb = M - tb * ADF_TILE < ADF_TILE ? M - tb * ADF_TILE : ADF_TILE;
                if (held + (unsigned long long)ADF_TILE * ADF_TILE > 0xffffffffull) flush();
                const int Q = ma * mb; // every pair (i of A, j of B)
                int j = lane / ma, i = lane % ma;
                for (int q = lane; q < Q; q += 64) {
                    const int k = adf_bin(e, abins, lut, ax[i], ay[i], az[i], ar[i], bx[j], by[j], bz[j], br[j]);
                    if (k >= 0) atomicAdd(&h[k + 1], 1u);
                    i += 64;
                    while (i >= ma) { i -= ma; ++j; }
                }
                held += (unsigned long long)Q;
            }
        }
    }
    flush();
}

// ---------------------------------------------------------------------------------------------------------------
// Static structure factor (include/nm_distr.h, nm_distr_sfactor): S(hkl) = |sum_a exp(-2 pi i (h, k, l) . u_a)|^2 / N on the
// reciprocal lattice of each sample's box, summed and maximised over the shells h^2 + k^2 + l^2 = n2.
//
// One workgroup takes one sample.  A work item is (h >= 0, k >= 0, l0): a thread owns the up to 4 * SF_LB vectors
// (h, +-k, +-l), l = l0 .. l0 + SF_LB - 1, that lie in the half space (h > 0, or h = 0 and k > 0, or h = k = 0 and l > 0) and
// inside the sphere; the host lists the items that hold at least one, l0 slowest, so that a wave's lanes share l0.  The atoms
// are walked in tiles of SF_TILE: for a tile the workgroup builds the per-axis tables E(m) = exp(-2 pi i m u), m = 0 .. qmax,
// in LDS (the phase m u reduced to [-1/2, 1/2] turns in float64 first; the z table holds (cos, sin) instead), then every
// thread adds the tile to its float64 accumulators.  With W = E_x(h) E_y(+-k) (negative k is the conjugate) the two sums
//   P(l) = sum_a W cos(2 pi l u_z),  Q(l) = sum_a W sin(2 pi l u_z)    give   rho(h, +-k, +l) = P - i Q,  rho(h, +-k, -l) = P + i Q:
// 8 real multiply-adds per atom for 4 vectors, where the direct product takes 8 for one.  The x and y factors are one LDS
// gather per atom and item, the z factors broadcasts.  A sample of 4095 atoms needs the LDS of one tile.
//
// Shell reduction: S < 2^12 is split into two integers, S 2^28 = hi + lo 2^-52 (lo truncated at 2^-80), which are added to the
// shell's two 64-bit LDS counters with integer atomics; the maximum is an integer maximum over the bit patterns (S >= 0).
// Integer addition is associative, so the sums are exact to 2^-80 per vector and the same bits in whatever order the lanes
// arrive: what a fixed reduction order gives, without one.  A shell of the sphere holds fewer than 2^10 vectors, so neither
// counter can overflow (hi < 2^40, lo < 2^52 per vector).  The outputs are written with ordinary stores.
constexpr int SF_BLOCK = 1024;
constexpr int SF_TILE = 16;     // atoms per table tile
constexpr int SF_LB = 4;        // consecutive l of a work item
constexpr int SF_QMAX = 32;

// table entries per atom and axis: m = 0 .. qmax, padded with zeros so that every item reads a whole chunk of l
__host__ __device__ inline int sf_row(int qmax) { return (qmax / SF_LB + 1) * SF_LB; }

__host__ __device__ inline size_t sf_lds_bytes(int qmax) // 52,632 B at qmax 32
{
    return (size_t)3 * SF_TILE * sf_row(qmax) * sizeof(double2) + (size_t)3 * SF_TILE * sizeof(double)
         + (size_t)3 * (qmax * qmax + 1) * sizeof(unsigned long long);
}

__host__ __device__ inline unsigned int sf_item(int h, int k, int l0) { return (unsigned int)h | (unsigned int)k << 8 | (unsigned int)l0 << 16; }

__device__ __forceinline__ void sf_add(unsigned long long *shi, unsigned long long *slo, unsigned long long *smx, int n2, double S)
{
    const double x = S * 0x1p28;
    const unsigned long long hi = (unsigned long long)x;
    const unsigned long long lo = (unsigned long long)((x - (double)hi) * 0x1p52); // x - hi is exact
    atomicAdd(&shi[n2], hi);
    atomicAdd(&slo[n2], lo);
    atomicMax(&smx[n2], (unsigned long long)__double_as_longlong(S));
}

__global__ void __launch_bounds__(SF_BLOCK)
nm_sfac_kernel(int natoms, const float *__restrict__ pos, const float *__restrict__ box, int qmax, int nitems,
               const unsigned int *__restrict__ items, double *__restrict__ sf_sum, double *__restrict__ sf_max)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int row = sf_row(qmax), q2 = qmax * qmax, nsh = q2 + 1;
    double2 *ex = (double2 *)smem, *ey = ex + SF_TILE * row, *ez = ey + SF_TILE * row;
    double *ut = (double *)(ez + SF_TILE * row);                       // reduced coordinates of the tile, [atom][axis]
    unsigned long long *shi = (unsigned long long *)(ut + 3 * SF_TILE), *slo = shi + nsh, *smx = slo + nsh;
    const double L = (double)box[s], dn = (double)natoms;
    const float *ps = pos + (size_t)s * natoms * 3;
    for (int k = tid; k < 3 * nsh; k += SF_BLOCK) shi[k] = 0ull;         // all three arrays; the first barrier below orders it
    for (int i0 = 0; i0 < nitems; i0 += SF_BLOCK) {
        const bool have = i0 + tid < nitems;
        const unsigned int it = have ? items[i0 + tid] : 0u;
        const int h = (int)(it & 255u), k = (int)((it >> 8) & 255u), l0 = (int)(it >> 16);
        const bool work = __ballot(have) != 0ull;                        // a wave without an item only builds tables
        double acc[2][SF_LB][4];                                         // [+k, -k][l - l0][Re P, Im P, Re Q, Im Q]
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int j = 0; j < SF_LB; ++j) { acc[g][j][0] = 0.0; acc[g][j][1] = 0.0; acc[g][j][2] = 0.0; acc[g][j][3] = 0.0; }
        for (int a0 = 0; a0 < natoms; a0 += SF_TILE) {
            const int na = natoms - a0 < SF_TILE ? natoms - a0 : SF_TILE;
            __syncthreads();                                             // the previous tile's readers are done
            if (tid < 3 * na) ut[tid] = (double)ps[3 * a0 + tid] / L;
            __syncthreads();
            for (int e = tid; e < 3 * na * row; e += SF_BLOCK) {         // consecutive lanes, consecutive m: conflict-free stores
                const int ad = e / row, m = e - ad * row;                // ad = 3 * atom + axis
                const int ai = ad / 3, d = ad - 3 * ai;
                double2 v = make_double2(0.0, 0.0);
                if (m <= qmax) {
                    const double x = (double)m * ut[ad];
                    double sn, cs;
                    sincos_turn(x - rint(x), sn, cs);                    // the difference is exact
                    v = d == 2 ? make_double2(cs, sn) : make_double2(cs, -sn);
                }
                (d == 0 ? ex : d == 1 ? ey : ez)[ai * row + m] = v;
            }
            __syncthreads();
            if (!work) continue;
            for (int ai = 0; ai < na; ++ai) {
                const double2 X = ex[ai * row + h], Y = ey[ai * row + k];
                const double A = X.x * Y.x, B = X.y * Y.y, C = X.x * Y.y, D = X.y * Y.x;
                const double wr0 = A - B, wi0 = C + D;                   // E_x(h) E_y(k)
                const double wr1 = A + B, wi1 = D - C;                   // E_x(h) E_y(-k)
                const double2 *zr = ez + ai * row + l0;
#pragma unroll
                for (int j = 0; j < SF_LB; ++j) {
                    const double2 Z = zr[j];
                    acc[0][j][0] = fma(wr0, Z.x, acc[0][j][0]); acc[0][j][1] = fma(wi0, Z.x, acc[0][j][1]);
                    acc[0][j][2] = fma(wr0, Z.y, acc[0][j][2]); acc[0][j][3] = fma(wi0, Z.y, acc[0][j][3]);
                    acc[1][j][0] = fma(wr1, Z.x, acc[1][j][0]); acc[1][j][1] = fma(wi1, Z.x, acc[1][j][1]);
                    acc[1][j][2] = fma(wr1, Z.y, acc[1][j][2]); acc[1][j][3] = fma(wi1, Z.y, acc[1][j][3]);
                }
            }
        }
        if (have) {
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                if (g == 1 && !(h > 0 && k > 0)) continue;               // (h, -k, l): not for k = 0; for h = 0 it mirrors (0, k, -l)
#pragma unroll
                for (int j = 0; j < SF_LB; ++j) {
                    const int l = l0 + j, n2 = h * h + k * k + l * l;
                    if (n2 < 1 || n2 > q2) continue;
                    const double pr = acc[g][j][0], pi = acc[g][j][1], qr = acc[g][j][2], qi = acc[g][j][3];
                    double re = pr + qi, im = pi - qr;                   // rho(+l) = P - i Q
                    sf_add(shi, slo, smx, n2, (re * re + im * im) / dn);
                    if (l > 0 && (h | k)) {                              // rho(-l) = P + i Q; (0, 0, -l) mirrors (0, 0, l)
                        re = pr - qi; im = pi + qr;
                        sf_add(shi, slo, smx, n2, (re * re + im * im) / dn);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int n2 = tid; n2 < nsh; n2 += SF_BLOCK) {                       // S(-q) = S(q): the full shell's sum is twice the half's
        if (sf_sum) sf_sum[(size_t)s * nsh + n2] = 2.0 * ((double)shi[n2] * 0x1p-28 + (double)slo[n2] * 0x1p-80);
        if (sf_max) sf_max[(size_t)s * nsh + n2] = __longlong_as_double((long long)smx[n2]);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Steinhardt bond-order parameters (include/nm_distr.h, nm_distr_bondorder): per centre c the moments
// q_lm(c) = (1/Nb) sum over the neighbour entries of Y_lm(n), n = v/|v| in float64 from the float32 displacement, the
// neighbour entries being exactly those of nm_adf_kernel; from them q2 (per atom), qbar2 (the moments averaged over the centre
// and its entries) and Q2 (the moments of all bonds of the frame).
//
// Harmonics without an azimuth and without a division by sin(theta): Y_lm(n) = N_l^m(n_z) (n_x + i n_y)^m for m >= 0, where
// N_l^m = (normalisation) P_l^m / sin^m(theta) is a polynomial in n_z that obeys the three-term recurrence of the normalised
// functions at fixed m,
//   N_m^m = c_m = (-1)^m sqrt((2m+1)!! / (4 pi (2m)!!)),   N_l^m = A_lm (n_z N_(l-1)^m - B_lm N_(l-2)^m),   N_(m-1)^m = 0,
//   A_lm = sqrt((4 l^2 - 1) / (l^2 - m^2)),   B_lm = sqrt(((l-1)^2 - m^2) / (4 (l-1)^2 - 1)),
// so a bond along the z axis is no special case.  The host computes c, A and B for l <= 12 (long double, rounded once) into the
// table the kernels read with wave-uniform indices.  Y_l,-m = (-1)^m conj(Y_lm): only m >= 0 is formed, and the invariant
// 4 pi / (2l+1) sum_m |q_lm|^2 counts m > 0 twice.
//
// Pass 1 (nm_bo_moments_kernel): a workgroup takes SHELL_CPB consecutive centres of one sample, positions and bounding box
// staged by shell_stage and shell_bounds; each wave works through its centres alone.  bo_scan is a sink of shell_scan, as
// adf_fill is: both see the same neighbours in the same order, whatever the scan does to find them.  bo_scan also records the
// atom index and hands the wave's list on in batches of 64 entries as it fills, so any number of neighbours is handled with one
// scan.  For a batch, lane = bond: the lane runs the recurrence (m outer, l inner) and puts the Y_lm of the requested l into
// the wave's LDS staging rows [component][bond]; when the rows are full, lane = component: each lane adds its row's bonds in
// list order to the centre's accumulator in LDS.  No accumulator is indexed at run time in registers, so nothing goes to
// scratch memory.  At the centre's end the wave writes q_lm(c) to the global scratch [sample][atom][component], q2 and nnb, and
// keeps the unnormalised sums for Q2; the workgroup's partial sums and bond count go to [sample][group].
// Pass 2 (nm_bo_average_kernel, only if qbar2 is asked for): the same scan, indices only; lane = component gathers q_lm(a) of
// the batch's entries in list order (one coalesced read of the atom's moments per entry, the reads of up to eight entries in
// flight), then qbar_lm and its invariant.  The pass is bo_average_centres with the invariant as its finish; nm_distr_w.h runs the
// same centres with the cubic invariant beside it.
// nm_bo_global_kernel adds the partials of a sample's groups in order (bo_global_moments, shared with nm_distr_w.h) and forms Q2.
// Every sum runs in a fixed order (entries in scan order, centres in order per wave, waves in order, groups in order): the
// result is the same bits on every call, without a floating-point atomic.
//
// Error bound (u = 2^-53), per bond, of the computed vector y = (Y_lm)_m against the exact one, relative to |y| = sqrt((2l+1)/4 pi):
//   direction   each component of n = v * (1 / sqrt(|v|^2)) carries at most 3 u relative (sum of squares 1.5 u, halved by the
//               root, the root, the reciprocal, the product), so n is off by at most 3 u in length and 3 u in direction.  y
//               transforms under the (2l+1)-dimensional unitary representation, whose generators have norm l: a rotation by
//               3 u moves y by at most 3 l u |y|.  The length error scales (n_x + i n_y)^m by (1 + 3u)^m and moves n_z in a
//               polynomial of degree l - m whose derivative is at most (l - m)^2 times its maximum (Markov): together at
//               most 3 (m + (l-m)^2) u <= 3 l^2 u for l >= 1, taken against the same norm.
//   recurrence  l - m steps of three roundings each on the dominant solution of the recurrence (forward in l at fixed m is
//               the stable direction), m complex products for the power (at most 3 u each), the table's roundings (one per
//               step), the final product: at most (4 (l - m) + 3 m + 2) u <= (4 l + 2) u on each component, against its own
//               envelope sqrt((2l+1)/4 pi).
//   together    e(l) = (3 l^2 + 7 l + 8) u, the 6 u left over for the invariant's own sum and the division by Nb: 524 u =
//               5.8e-14 at l = 12.
// Sums: a fixed-order float64 sum of n terms of norm <= |y| adds at most (n - 1) u |y|.  So with M = the largest Nb:
//   q      e_q = e(l) + M u;             qbar    e_q + (M + 1) u;             Q    e(l) + (M + 12 + ceil(natoms / 32)) u
// (Q: the entries of a centre, then a wave's 8 centres, the 4 waves and the groups of 32 centres), and for each invariant
// x = |.|^2, |dx| <= 2 e sqrt(x) + e^2.  tests/bondorder_ref.py holds the same expressions; the tests allow twice that.
constexpr int BO_LIST = 128;    // list entries per wave: a batch of 64 and what one scan step can add to 63
constexpr int BO_SC = 16;       // staging rows (real components) per wave
constexpr int BO_ROW = 65;      // doubles per staging row: 64 bonds, padded so that lane = component reads spread over the banks
constexpr int BO_LMAX = 12;
constexpr int BO_MAXL = 6;      // most l values per call
constexpr int BO_TAB = (BO_LMAX + 1) * (2 * (BO_LMAX + 1) + 1); // c[m], A[l][m], B[l][m]

// what the kernels need to know of the requested l: bit l of lmask, the component offset of l (sum of l' + 1 over the
// requested l' < l) in 8 bits each (l = 1..8 in off_lo, 9..12 in off_hi), nc = sum of l + 1: scalar arithmetic only
struct BoSet { int nl, nc, lmax; unsigned int lmask; unsigned long long off_lo; unsigned int off_hi; };

__host__ __device__ __forceinline__ int bo_off(const BoSet &b, int l)
{
    return l <= 8 ? (int)((b.off_lo >> (8 * (l - 1))) & 255ull) : (int)((b.off_hi >> (8 * (l - 9))) & 255u);
}

__host__ __device__ inline size_t bo_lds_bytes(int natoms, int nc, bool moments)
{
    const size_t wave = (size_t)((moments ? BO_SC * BO_ROW + 4 * nc : 2 * nc)) * sizeof(double) // staging, acc and frame sums | qbar
                      + (size_t)(moments ? 4 : 1) * BO_LIST * 4 + (size_t)(BO_SC / 2 + 2) * 4; // list (vectors, index), row map, count
    return (size_t)SHELL_WAVES * wave + ((size_t)3 * natoms + SHELL_WAVES * 6) * sizeof(float);
}

// the l of the i-th requested value
__device__ __forceinline__ int bo_l_of(const BoSet &b, int i)
{
    int l = 0, k = -1;
    while (k < i && l < BO_LMAX) { ++l; if ((b.lmask >> l) & 1u) ++k; }
    return l;
}

// 4 pi / (2l+1) sum_{m=-l..l} |q_lm|^2 from the m >= 0 components q[2m], q[2m+1]
__device__ __forceinline__ double bo_invariant(const double *q, int l)
{
    double t = 0.0;
    for (int m = 1; m <= l; ++m) t += q[2 * m] * q[2 * m] + q[2 * m + 1] * q[2 * m + 1];
    return (4.0 * 3.14159265358979323846 / (double)(2 * l + 1)) * (q[0] * q[0] + q[1] * q[1] + 2.0 * t);
}

// One shell_scan of centre (cx, cy, cz) with the atom index recorded: the neighbour entries in scan order go to the wave's
// list (VEC: with their float32 components), and batch(n) is called with the list's first n entries whenever 64 are there, and
// with the rest at the end; entries beyond 64 move to the front.  Returns the number of entries.
template <bool VEC, class F>
__device__ __forceinline__ int bo_scan(const float *px, const float *py, const float *pz, int natoms, float cx, float cy, float cz,
                                       float L, float cube, const float *bb, double r_lo, double r_hi, float *lx, float *ly,
                                       float *lz, int *li, int lane, F &&batch)
{
    int cnt = 0, total = 0;
    shell_scan(px, py, pz, natoms, cx, cy, cz, L, cube, bb, r_lo, r_hi, lane,
               [&](int a, bool in, float vx, float vy, float vz, unsigned long long m) {
        if (in) {
            const int o = cnt + __popcll(m & ((1ull << lane) - 1ull)); // cnt <= 63 here: o <= 126 < BO_LIST
            if (VEC) { lx[o] = vx; ly[o] = vy; lz[o] = vz; }
            li[o] = a;
        }
        cnt += __popcll(m);
        total += __popcll(m);
        if (cnt >= 64) {
            adf_wave_sync();
            batch(64);
            adf_wave_sync();
            const int rest = cnt - 64;
            float tx = 0.0f, ty = 0.0f, tz = 0.0f;
            if (VEC) { tx = lx[64 + lane]; ty = ly[64 + lane]; tz = lz[64 + lane]; }
            const int ti = li[64 + lane];
            adf_wave_sync();
            if (lane < rest) {
                if (VEC) { lx[lane] = tx; ly[lane] = ty; lz[lane] = tz; }
                li[lane] = ti;
            }
            adf_wave_sync();
            cnt = rest;
        }
        return true;
    });
    if (cnt > 0) {
        adf_wave_sync();
        batch(cnt);
        adf_wave_sync();
    }
    return total;
}

__global__ void __launch_bounds__(SHELL_BLOCK)
nm_bo_moments_kernel(int natoms, const float *__restrict__ pos, const float *__restrict__ box, double r_lo, double r_hi, float cube,
                     BoSet set, const double *__restrict__ tab, double *__restrict__ qlm, double *__restrict__ q2,
                     int *__restrict__ nnb, double *__restrict__ partial, int *__restrict__ pcount)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int groups = (natoms + SHELL_CPB - 1) / SHELL_CPB;
    const int s = blockIdx.x / groups, grp = blockIdx.x % groups, c0 = grp * SHELL_CPB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nc2 = 2 * set.nc;
    double *stage_all = (double *)smem, *acc_all = stage_all + SHELL_WAVES * BO_SC * BO_ROW, *gacc_all = acc_all + SHELL_WAVES * nc2;
    float *lv_all = (float *)(gacc_all + SHELL_WAVES * nc2);
    int *li_all = (int *)(lv_all + SHELL_WAVES * 3 * BO_LIST), *rowc_all = li_all + SHELL_WAVES * BO_LIST;
    int *wcount = rowc_all + SHELL_WAVES * (BO_SC / 2);
    float *px = (float *)(wcount + SHELL_WAVES * 2), *py = px + natoms, *pz = py + natoms, *part = pz + natoms;
    const float L = box[s];
    float bb[6];
    shell_stage(pos + (size_t)s * natoms * 3, natoms, px, py, pz, part);
    __syncthreads();
    shell_bounds(part, bb);
    double *stage = stage_all + wave * BO_SC * BO_ROW, *acc = acc_all + wave * nc2, *gacc = gacc_all + wave * nc2;
    float *lx = lv_all + wave * 3 * BO_LIST, *ly = lx + BO_LIST, *lz = ly + BO_LIST;
    int *li = li_all + wave * BO_LIST, *rowc = rowc_all + wave * (BO_SC / 2);
    const double *tc = tab, *tA = tab + (BO_LMAX + 1), *tB = tA + (BO_LMAX + 1) * (BO_LMAX + 1);
    for (int j = lane; j < nc2; j += 64) gacc[j] = 0.0;
    int gcount = 0;
    const int cend = c0 + SHELL_CPB < natoms ? c0 + SHELL_CPB : natoms;
    for (int c = c0 + wave; c < cend; c += SHELL_WAVES) {
        for (int j = lane; j < nc2; j += 64) acc[j] = 0.0;
        adf_wave_sync();
        const float cx = wave_uniform(px[c]), cy = wave_uniform(py[c]), cz = wave_uniform(pz[c]);
        const int nb = bo_scan<true>(px, py, pz, natoms, cx, cy, cz, L, cube, bb, r_lo, r_hi, lx, ly, lz, li, lane, [&](int mb) {
            // lane = bond: the unit vector in float64 from the float32 components
            const bool act = lane < mb;
            const double X = act ? (double)lx[lane] : 0.0, Y = act ? (double)ly[lane] : 0.0, Z = act ? (double)lz[lane] : 1.0;
            const double rinv = 1.0 / sqrt(fma(Z, Z, fma(Y, Y, X * X)));
            const double nx = X * rinv, ny = Y * rinv, nz = Z * rinv;
            int nst = 0;
            // lane = component: add the staged rows' bonds in list order to the centre's accumulators
            auto flush = [&]() {
                adf_wave_sync();
                if (lane < nst) {
                    const double *r = stage + lane * BO_ROW;
                    double t = 0.0;
                    for (int b = 0; b < mb; ++b) t += r[b];
                    acc[2 * rowc[lane >> 1] + (lane & 1)] += t;
                }
                adf_wave_sync();
                nst = 0;
            };
            double pr = 1.0, pi = 0.0; // (n_x + i n_y)^m
            for (int m = 0; m <= set.lmax; ++m) {
                if (m > 0) { const double t = pr * nx - pi * ny; pi = pr * ny + pi * nx; pr = t; }
                double p0 = tc[m], p1 = 0.0; // N_l^m, N_(l-1)^m
                for (int l = m; l <= set.lmax; ++l) {
                    if (l > m) {
                        const double p = tA[l * (BO_LMAX + 1) + m] * (nz * p0 - tB[l * (BO_LMAX + 1) + m] * p1);
                        p1 = p0; p0 = p;
                    }
                    if ((set.lmask >> l) & 1u) {
                        if (nst + 2 > BO_SC) flush();
                        stage[nst * BO_ROW + lane] = p0 * pr;
                        stage[(nst + 1) * BO_ROW + lane] = p0 * pi;
                        if (lane == 0) rowc[nst >> 1] = bo_off(set, l) + m;
                        nst += 2;
                    }
                }
            }
            flush();
        });
        // q_lm(c), the frame's sums, q2 and nnb
        const size_t at = (size_t)s * natoms + c;
        for (int j = lane; j < nc2; j += 64) {
            const double a = acc[j];
            gacc[j] += a;
            const double q = nb > 0 ? a / (double)nb : 0.0;
            acc[j] = q;
            qlm[at * nc2 + j] = q;
        }
        gcount += nb;
        adf_wave_sync();
        if (q2 && lane < set.nl) {
            const int l = bo_l_of(set, lane);
            q2[at * set.nl + lane] = bo_invariant(acc + 2 * bo_off(set, l), l);
        }
        if (nnb && lane == 0) nnb[at] = nb;
        adf_wave_sync();
    }
    if (lane == 0) wcount[wave] = gcount;
    __syncthreads();
    if (tid < nc2) {
        double t = gacc_all[tid];
        for (int w = 1; w < SHELL_WAVES; ++w) t += gacc_all[w * nc2 + tid];
        partial[((size_t)s * groups + grp) * nc2 + tid] = t;
    }
    if (tid == 0) {
        int t = 0;
        for (int w = 0; w < SHELL_WAVES; ++w) t += wcount[w];
        pcount[(size_t)s * groups + grp] = t;
    }
}

// pass 2's gather: the components lane and lane + 64 of the moments of K list entries, all reads issued before the first sum,
// added in list order
template <int K>
__device__ __forceinline__ void bo_gather(const double *__restrict__ qs, const int *li, int nc2, int lane, bool own0, bool own1,
                                          double &a0, double &a1)
{
    double v0[K], v1[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double *r = qs + (size_t)li[k] * nc2;
        v0[k] = own0 ? r[lane] : 0.0;
        v1[k] = own1 ? r[lane + 64] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        if (own0) a0 += v0[k];
        if (own1) a1 += v1[k];
    }
}

// Pass 2's centres: the staging, the scan and the gather of the workgroup's centres.  Where qbar_lm(c) stands in the wave's LDS row
// (m >= 0, real and imaginary parts in turn, the l in the set's order), finish(s, c, qbar, lane) is called by the whole wave: what is
// formed from the averaged moments (nm_bo_average_kernel's invariant, nm_distr_w.h's cubic one) reads the same bits.
template <class E>
__device__ __forceinline__ void bo_average_centres(int natoms, const float *__restrict__ pos, const float *__restrict__ box, double r_lo,
                                                   double r_hi, float cube, const BoSet &set, const double *__restrict__ qlm, E &&finish)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int groups = (natoms + SHELL_CPB - 1) / SHELL_CPB;
    const int s = blockIdx.x / groups, c0 = (blockIdx.x % groups) * SHELL_CPB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nc2 = 2 * set.nc; // at most 126: a lane owns the components lane and lane + 64
    double *acc_all = (double *)smem;
    int *li_all = (int *)(acc_all + SHELL_WAVES * nc2);
    float *px = (float *)(li_all + SHELL_WAVES * BO_LIST + SHELL_WAVES * (BO_SC / 2 + 2)), *py = px + natoms, *pz = py + natoms, *part = pz + natoms;
    const float L = box[s];
    float bb[6];
    shell_stage(pos + (size_t)s * natoms * 3, natoms, px, py, pz, part);
    __syncthreads();
    shell_bounds(part, bb);
    double *acc = acc_all + wave * nc2;
    int *li = li_all + wave * BO_LIST;
    const double *qs = qlm + (size_t)s * natoms * nc2;
    const bool own0 = lane < nc2, own1 = lane + 64 < nc2;
    const int cend = c0 + SHELL_CPB < natoms ? c0 + SHELL_CPB : natoms;
    for (int c = c0 + wave; c < cend; c += SHELL_WAVES) {
        const float cx = wave_uniform(px[c]), cy = wave_uniform(py[c]), cz = wave_uniform(pz[c]);
        double a0 = 0.0, a1 = 0.0;
        const int nb = bo_scan<false>(px, py, pz, natoms, cx, cy, cz, L, cube, bb, r_lo, r_hi, nullptr, nullptr, nullptr, li, lane, [&](int mb) {
            // up to eight entries' reads in flight at a time (one entry's reads after the other leave the wave waiting for L2 four
            // fifths of its cycles at 126 neighbours); the sums keep the list order
            int b = 0;
            for (; b + 8 <= mb; b += 8) bo_gather<8>(qs, li + b, nc2, lane, own0, own1, a0, a1);
            if (b + 4 <= mb) { bo_gather<4>(qs, li + b, nc2, lane, own0, own1, a0, a1); b += 4; }
            for (; b < mb; ++b) bo_gather<1>(qs, li + b, nc2, lane, own0, own1, a0, a1);
        });
        const double *rc = qs + (size_t)c * nc2;
        const double den = (double)(nb + 1);
        if (own0) acc[lane] = (rc[lane] + a0) / den;
        if (own1) acc[lane + 64] = (rc[lane + 64] + a1) / den;
        adf_wave_sync();
        finish(s, c, acc, lane);
        adf_wave_sync();
    }
}

// qbar2 of a centre from its averaged moments in LDS: lane = requested l
__device__ __forceinline__ void bo_average_invariant(const BoSet &set, int natoms, int s, int c, const double *qbar, int lane,
                                                     double *__restrict__ qbar2)
{
    if (lane < set.nl) {
        const int l = bo_l_of(set, lane);
        qbar2[((size_t)s * natoms + c) * set.nl + lane] = bo_invariant(qbar + 2 * bo_off(set, l), l);
    }
}

__global__ void __launch_bounds__(SHELL_BLOCK)
nm_bo_average_kernel(int natoms, const float *__restrict__ pos, const float *__restrict__ box, double r_lo, double r_hi, float cube,
                     BoSet set, const double *__restrict__ qlm, double *__restrict__ qbar2)
{
    bo_average_centres(natoms, pos, box, r_lo, r_hi, cube, set, qlm,
                       [&](int s, int c, const double *qbar, int lane) { bo_average_invariant(set, natoms, s, c, qbar, lane, qbar2); });
}

// the moments of all bonds of sample s in q (LDS, 2 nc doubles): the groups' partial sums in order, divided by the groups' bonds; a
// workgroup barrier stands behind them
__device__ __forceinline__ void bo_global_moments(int groups, const BoSet &set, const double *__restrict__ partial,
                                                  const int *__restrict__ pcount, int s, double *q)
{
    const int tid = threadIdx.x, nc2 = 2 * set.nc;
    if (tid < nc2) {
        double t = 0.0;
        long long n = 0;
        for (int g = 0; g < groups; ++g) {
            t += partial[((size_t)s * groups + g) * nc2 + tid];
            n += pcount[(size_t)s * groups + g];
        }
        q[tid] = n > 0 ? t / (double)n : 0.0;
    }
    __syncthreads();
}

// one workgroup of 128 threads per sample: the groups' partial sums in order, the moments of all bonds, Q2
__global__ void __launch_bounds__(128)
nm_bo_global_kernel(int groups, BoSet set, const double *__restrict__ partial, const int *__restrict__ pcount, double *__restrict__ Q2)
{
    __shared__ double q[2 * BO_MAXL * (BO_LMAX + 1)];
    const int s = blockIdx.x, tid = threadIdx.x;
    bo_global_moments(groups, set, partial, pcount, s, q);
    if (tid < set.nl) {
        const int l = bo_l_of(set, tid);
        Q2[(size_t)s * set.nl + tid] = bo_invariant(q + 2 * bo_off(set, l), l);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Solid-like atoms and crystal clusters (include/nm_distr.h, nm_distr_solid): ten Wolde, Ruiz-Montero and Frenkel's criterion on
// the normalised dot products of the q_lm vectors of neighbouring atoms, then the connected components of the solid-like atoms.
// The moments come from nm_bo_moments_kernel, launched for the single l and unchanged; three kernels follow, each a kernel
// boundary behind what it reads:
//   connect  (nm_solid_connect_kernel) the grid and staging of the average pass, bo_scan<false>.  For a batch, lane = entry: the
//            lane walks the moments' rows of the centre (the same address in every lane) and of its entry's atom (l + 1 reads of
//            16 B from a row of at most 208 B that L2 holds) and forms the dot product and both norms with m ascending, a fixed
//            order: the same bits on every call.  The connections are counted by ballot and popcount.  The wave writes nconn[c]
//            (an atom is solid-like where nconn >= n_min: the later kernels read the flag off that array) and parent[c] = c.
//   union    (nm_solid_union_kernel) the same grid; a centre that is not solid-like is skipped, a solid-like one is scanned
//            again, indices only, and every entry whose atom is solid-like is united with the centre in the sample's parent
//            array.  An edge that only one of its two ends sees as an entry (the float32 test on the cutoff itself) is united
//            from that end: both ends are scanned, being solid-like.
//   label    (nm_solid_label_kernel) one workgroup per sample: label = root or -1, the cluster sizes by LDS integer atomics on
//            the root, then nsolid, nclus, largest.
// The union-find is lock-free and no thread ever waits for another: no spin loop, no polled flag, no cooperative launch.
// Invariants of parent[] (one int per atom, indices within the sample):
//   (1) parent[x] <= x always: it starts as x, and every write stores a smaller value;
//   (2) every write lowers a value: a hook is atomicCAS(parent[r], r, smaller root), a compression is atomicMin(parent[x],
//       grandparent); so a value read earlier is still an ancestor, and a root (parent[r] == r) is never written by a compression;
//   (3) the atomicCAS of a hook fails only if r is no longer a root, which only another hook's success can cause: a sample sees at
//       most natoms - 1 successful hooks, so all threads together retry at most that often per root they aimed at;
//   (4) a find terminates: along parent[] the indices decrease strictly until a root, at most natoms - 1 steps.
// The smaller root always wins, so the root of a finished cluster is its smallest index: the label is canonical, whatever the
// order of execution.  Reads of parent[] that race with other workgroups are relaxed atomic loads at agent scope (they pass the
// caches that are not coherent across the device); the label kernel runs behind a kernel boundary and reads plainly.
// Integer atomics only.
constexpr int SOLID_BLOCK = 256;    // threads of the label kernel
constexpr int SOLID_MAXN = 4096;    // its LDS counters: natoms <= 4095

__host__ __device__ inline size_t solid_lds_bytes(int natoms) // 51,284 B at 4095 atoms
{
    return (size_t)SHELL_WAVES * BO_LIST * sizeof(int) + ((size_t)3 * natoms + SHELL_WAVES * 6) * sizeof(float);
}

__global__ void __launch_bounds__(SHELL_BLOCK)
nm_solid_connect_kernel(int natoms, const float *__restrict__ pos, const float *__restrict__ box, double r_lo, double r_hi, float cube,
                        int l, double s_min, const double *__restrict__ qlm, int *__restrict__ nconn, int *__restrict__ parent)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int groups = (natoms + SHELL_CPB - 1) / SHELL_CPB;
    const int s = blockIdx.x / groups, c0 = (blockIdx.x % groups) * SHELL_CPB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int *li_all = (int *)smem;
    float *px = (float *)(li_all + SHELL_WAVES * BO_LIST), *py = px + natoms, *pz = py + natoms, *part = pz + natoms;
    const float L = box[s];
    float bb[6];
    shell_stage(pos + (size_t)s * natoms * 3, natoms, px, py, pz, part);
    __syncthreads();
    shell_bounds(part, bb);
    int *li = li_all + wave * BO_LIST;
    const int nc2 = 2 * (l + 1); // a row is 16 (l + 1) bytes: every (Re, Im) pair is one aligned 16-byte read
    const double *qs = qlm + (size_t)s * natoms * nc2;
    const int cend = c0 + SHELL_CPB < natoms ? c0 + SHELL_CPB : natoms;
    for (int c = c0 + wave; c < cend; c += SHELL_WAVES) {
        const float cx = wave_uniform(px[c]), cy = wave_uniform(py[c]), cz = wave_uniform(pz[c]);
        const double2 *rc = (const double2 *)(qs + (size_t)c * nc2);
        int conn = 0;
        bo_scan<false>(px, py, pz, natoms, cx, cy, cz, L, cube, bb, r_lo, r_hi, nullptr, nullptr, nullptr, li, lane, [&](int mb) {
            const bool act = lane < mb;
            const double2 *ra = (const double2 *)(qs + (size_t)(act ? li[lane] : c) * nc2);
            const double2 C0 = rc[0], A0 = ra[0];
            double dm = 0.0, cm = 0.0, am = 0.0; // the sums over m > 0, m ascending
            for (int m = 1; m <= l; ++m) {
                const double2 C = rc[m], A = ra[m];
                dm = fma(C.y, A.y, fma(C.x, A.x, dm));
                cm = fma(C.y, C.y, fma(C.x, C.x, cm));
                am = fma(A.y, A.y, fma(A.x, A.x, am));
            }
            const double dot = fma(C0.y, A0.y, C0.x * A0.x) + 2.0 * dm;
            const double n2c = fma(C0.y, C0.y, C0.x * C0.x) + 2.0 * cm, n2a = fma(A0.y, A0.y, A0.x * A0.x) + 2.0 * am;
            const double den = sqrt(n2c) * sqrt(n2a);
            const double sv = den > 0.0 ? dot / den : 0.0;
            conn += __popcll(__ballot(act && sv > s_min));
        });
        if (lane == 0) {
            nconn[(size_t)s * natoms + c] = conn;
            parent[(size_t)s * natoms + c] = c;
        }
    }
}

__device__ __forceinline__ int solid_peek(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x, halving the path on the way: x's parent is lowered to its grandparent (invariant 2), then the walk goes on from
// the grandparent.  Every step lowers x or ends the walk (invariant 4).
__device__ __forceinline__ int solid_find(int *parent, int x)
{
    for (;;) {
        const int p = solid_peek(parent + x);
        if (p == x) return x;
        const int g = solid_peek(parent + p);
        if (g < p) atomicMin(parent + x, g);
        x = g;
    }
}

// unites the clusters of x and y: the larger of the two roots is hooked under the smaller with one atomicCAS.  A failure means
// that the larger one has been hooked by someone else in the meantime (invariant 3): find again from where we are, nothing to
// wait for.
__device__ __forceinline__ void solid_union(int *parent, int x, int y)
{
    for (;;) {
        x = solid_find(parent, x);
        y = solid_find(parent, y);
        if (x == y) return;
        const int hi = x > y ? x : y, lo = x > y ? y : x;
        if (atomicCAS(parent + hi, hi, lo) == hi) return;
        x = hi; y = lo;
    }
}

__global__ void __launch_bounds__(SHELL_BLOCK)
nm_solid_union_kernel(int natoms, const float *__restrict__ pos, const float *__restrict__ box, double r_lo, double r_hi, float cube,
                      int n_min, const int *__restrict__ nconn, int *parent)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int groups = (natoms + SHELL_CPB - 1) / SHELL_CPB;
    const int s = blockIdx.x / groups, c0 = (blockIdx.x % groups) * SHELL_CPB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int *nc = nconn + (size_t)s * natoms;
    const int cend = c0 + SHELL_CPB < natoms ? c0 + SHELL_CPB : natoms;
    {
        // a workgroup without a solid-like centre has nothing to unite (the same answer in every thread: no barrier is skipped
        // by a part of the workgroup)
        bool any = false;
        for (int c = c0; c < cend; ++c) any = any || nc[c] >= n_min;
        if (!any) return;
    }
    int *li_all = (int *)smem;
    float *px = (float *)(li_all + SHELL_WAVES * BO_LIST), *py = px + natoms, *pz = py + natoms, *part = pz + natoms;
    const float L = box[s];
    float bb[6];
    shell_stage(pos + (size_t)s * natoms * 3, natoms, px, py, pz, part);
    __syncthreads();
    shell_bounds(part, bb);
    int *li = li_all + wave * BO_LIST;
    int *par = parent + (size_t)s * natoms;
    for (int c = c0 + wave; c < cend; c += SHELL_WAVES) {
        if (nc[c] < n_min) continue; // wave-uniform
        const float cx = wave_uniform(px[c]), cy = wave_uniform(py[c]), cz = wave_uniform(pz[c]);
        bo_scan<false>(px, py, pz, natoms, cx, cy, cz, L, cube, bb, r_lo, r_hi, nullptr, nullptr, nullptr, li, lane, [&](int mb) {
            if (lane < mb) {
                const int a = li[lane];
                if (a != c && nc[a] >= n_min) solid_union(par, c, a);
            }
        });
    }
}

__global__ void __launch_bounds__(SOLID_BLOCK)
nm_solid_label_kernel(int natoms, int n_min, const int *__restrict__ nconn, const int *__restrict__ parent, int *__restrict__ label,
                      int *__restrict__ nsolid, int *__restrict__ nclus, int *__restrict__ largest)
{
    __shared__ int size[SOLID_MAXN];
    __shared__ int red[SOLID_BLOCK / 64][3];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int *nc = nconn + (size_t)s * natoms, *par = parent + (size_t)s * natoms;
    for (int c = tid; c < natoms; c += SOLID_BLOCK) size[c] = 0;
    __syncthreads();
    for (int c = tid; c < natoms; c += SOLID_BLOCK) {
        int r = -1;
        if (nc[c] >= n_min) {
            r = c;
            for (int p = par[r]; p != r; p = par[r]) r = p; // invariant 4
            atomicAdd(&size[r], 1);
        }
        label[(size_t)s * natoms + c] = r;
    }
    __syncthreads();
    int ns = 0, ncl = 0, big = 0;
    for (int c = tid; c < natoms; c += SOLID_BLOCK) {
        const int v = size[c];
        ns += v; ncl += v > 0 ? 1 : 0; big = v > big ? v : big;
    }
    for (int o = 32; o > 0; o >>= 1) {
        ns += __shfl_xor(ns, o); ncl += __shfl_xor(ncl, o);
        const int t = __shfl_xor(big, o);
        big = t > big ? t : big;
    }
    if ((tid & 63) == 0) { red[tid >> 6][0] = ns; red[tid >> 6][1] = ncl; red[tid >> 6][2] = big; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < SOLID_BLOCK / 64; ++w) {
            ns += red[w][0]; ncl += red[w][1]; big = red[w][2] > big ? red[w][2] : big;
        }
        nsolid[s] = ns; nclus[s] = ncl; largest[s] = big;
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Common neighbour analysis (include/nm_distr.h, nm_distr_cna): per centre the graph of bonds among its own neighbour vectors, per
// neighbour the signature (common neighbours, bonds among them, bonds of their largest component), from the signatures' counts the
// structure type.  The grid and staging of the other shell kernels; each wave works through its centres alone:
//   scan       shell_scan, one pass.  FIXED: the entries are counted and the first CNA_MAXV vectors go to the wave's LDS list in scan
//              order.  ADAPTIVE: the wave keeps the CNA_KEEP smallest entries by (d, scan order) sorted in its lanes' registers (lane
//              k holds entry k).  A scan step's candidates are the lanes whose d lies below the list's last (a tie loses: the list's
//              entries come earlier in the scan); where there is none, which is nearly every step once the list is full, the step
//              costs one ballot.  Otherwise the step is merged in: every held entry and every candidate counts the keys before its
//              own (the candidates' d arrive by one cross-lane read per candidate, the held d by one per held entry), which is its
//              rank in the union, a total order; the ranks below CNA_KEEP are scattered to LDS slots, each written once, and read
//              back by the lanes.  Any number of entries is handled; the list is never longer than CNA_KEEP.
//   cutoffs    ADAPTIVE: rc12 and rc14 in float64 from the sorted d, every lane the same sum in the stated order (cna_rc), no
//              contraction.
//   adjacency  the nv <= 32 vertices' nv (nv - 1) / 2 pairs spread over the lanes (adf's numbering), at most 8 steps; a bond sets the
//              two bits of the vertices' 32-bit masks in the wave's LDS (integer OR: the order does not matter).
//   signature  lane k = vertex k, integer registers: cn = adj[k]; the bonds among cn are half the sum of popcount(adj[m] & cn) over
//              the m in cn; the components of cn by a flood fill over the masks, the bonds of each counted the same way.
//   counts     the column counts of a centre by eight ballots (wave-uniform: the type follows without a further exchange); lane
//              k < 8 keeps the wave's sum of column k, lane 8 + t the wave's number of atoms of type t; at the end LDS integer
//              atomics per workgroup, then one global integer atomic per column and type.
// Integer atomics only: the same bits on every call.
constexpr int CNA_MAXV = 32;    // most vertices of a graph: one mask word per vertex
constexpr int CNA_KEEP = 14;    // entries the adaptive mode keeps: the bcc test's
constexpr int CNA_NSIG = 8;     // signature columns: 421 422 444 666 555 544 433 other
constexpr int CNA_NTYPE = 5;    // other fcc hcp bcc ico
constexpr int CNA_WAVE = 4 * CNA_MAXV + 16;                 // a wave's LDS words: list vectors, masks, merge slots' d
constexpr int CNA_TOT = 16;                                 // the workgroup's sums: CNA_NSIG columns, CNA_NTYPE types, padding
static_assert(CNA_NSIG + CNA_NTYPE <= CNA_TOT && CNA_KEEP <= 16 && CNA_KEEP <= CNA_MAXV, "the sums and merge slots fit their arrays");

__host__ __device__ inline size_t cna_lds_bytes(int natoms) // 51,604 B at 4095 atoms
{
    return (size_t)(SHELL_WAVES * CNA_WAVE + CNA_TOT) * 4 + ((size_t)3 * natoms + SHELL_WAVES * 6) * sizeof(float);
}

// the float32 length of the definition: sequential sum, correctly rounded root (see nm_distr_kernel), no contraction
__device__ __forceinline__ float cna_len(float x, float y, float z)
{
#pragma clang fp contract(off)
    float d2 = x * x;
    d2 = d2 + y * y;
    d2 = d2 + z * z;
    return sqrtf(d2);
}

// the adaptive cutoff over the first nv = 12 or 14 sorted entries (lane k holds d_k): float64, added in order, one rounding per
// operation; at 14 the first 8 are scaled by 2 / sqrt 3 (the bcc shells' ratio)
__device__ __forceinline__ double cna_rc(float hd, int nv)
{
#pragma clang fp contract(off)
    double sum = 0.0;
    for (int k = 0; k < nv; ++k) {
        const double dk = (double)__shfl(hd, k);
        const double term = (nv == 14 && k < 8) ? dk * 1.1547005383792517 : dk;
        sum = sum + term;
    }
    const double scaled = 1.2071067811865475 * sum;
    return scaled / (double)nv;
}

__device__ __forceinline__ int cna_column(int ncn, int nb, int nlc)
{
    if (ncn == 4 && nb == 2 && nlc == 1) return 0;
    if (ncn == 4 && nb == 2 && nlc == 2) return 1;
    if (ncn == 4 && nb == 4 && nlc == 4) return 2;
    if (ncn == 6 && nb == 6 && nlc == 6) return 3;
    if (ncn == 5 && nb == 5 && nlc == 5) return 4;
    if (ncn == 5 && nb == 4 && nlc == 4) return 5;
    if (ncn == 4 && nb == 3 && nlc == 3) return 6;
    return 7;
}

// fcc, hcp or ico from the column counts of 12 vertices, else other
__device__ __forceinline__ int cna_close_packed(const int (&n)[CNA_NSIG])
{
    return n[0] == 12 ? 1 : (n[0] == 6 && n[1] == 6) ? 2 : n[4] == 12 ? 4 : 0;
}

// The graph on the first nv <= CNA_MAXV vectors of the wave's list with the cutoff rc, and every vertex's signature column: n[] are
// the column counts, the same in every lane.
__device__ __forceinline__ void cna_columns(const float *lx, const float *ly, const float *lz, unsigned int *adj, int nv, double r_lo,
                                            double rc, int lane, int (&n)[CNA_NSIG])
{
    if (lane < CNA_MAXV) adj[lane] = 0u;
    adf_wave_sync(); // the list and the cleared masks are in place
    if (nv >= 2) {
        // pair number q = (dd - 1) * nv + i is (i, (i + dd) mod nv) for the offsets dd = 1 .. nv/2 (for even nv the last offset only
        // with i < nv/2): nv (nv - 1) / 2 pairs, each once
        const int Q = nv * (nv - 1) / 2;
        int dd = 1 + lane / nv, i = lane % nv;
        for (int q = lane; q < Q; q += 64) {
            const int j = i + dd < nv ? i + dd : i + dd - nv;
            const double dw = (double)cna_len(lx[j] - lx[i], ly[j] - ly[i], lz[j] - lz[i]);
            if (r_lo < dw && dw <= rc) {
                atomicOr(&adj[i], 1u << j);
                atomicOr(&adj[j], 1u << i);
            }
            i += 64;
            while (i >= nv) { i -= nv; ++dd; }
        }
    }
    adf_wave_sync();
    int col = -1;
    if (lane < nv) {
        const unsigned int cn = adj[lane];
        int nb2 = 0, nlc = 0;
        for (unsigned int t = cn; t; t &= t - 1u) nb2 += __popc(adj[__ffs((int)t) - 1] & cn);
        for (unsigned int rem = cn; rem;) {
            unsigned int comp = rem & (0u - rem), front = comp; // the component of the lowest vertex left
            while (front) {
                unsigned int grow = 0u;
                for (unsigned int t = front; t; t &= t - 1u) grow |= adj[__ffs((int)t) - 1] & cn;
                front = grow & ~comp;
                comp |= front;
            }
            int b2 = 0;
            for (unsigned int t = comp; t; t &= t - 1u) b2 += __popc(adj[__ffs((int)t) - 1] & comp);
            nlc = b2 >> 1 > nlc ? b2 >> 1 : nlc;
            rem &= ~comp;
        }
        col = cna_column(__popc(cn), nb2 >> 1, nlc);
    }
#pragma unroll
    for (int k = 0; k < CNA_NSIG; ++k) n[k] = __popcll(__ballot(col == k));
}

__global__ void __launch_bounds__(SHELL_BLOCK)
nm_cna_kernel(int natoms, const float *__restrict__ pos, const float *__restrict__ box, double r_lo, double r_hi, float cube,
              bool adaptive, int *__restrict__ type, int *__restrict__ sig, int *__restrict__ ntype, int *__restrict__ nsig)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int groups = (natoms + SHELL_CPB - 1) / SHELL_CPB;
    const int s = blockIdx.x / groups, c0 = (blockIdx.x % groups) * SHELL_CPB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float *wave_all = (float *)smem;
    int *tot = (int *)(wave_all + SHELL_WAVES * CNA_WAVE);
    float *px = (float *)(tot + CNA_TOT), *py = px + natoms, *pz = py + natoms, *part = pz + natoms;
    const float L = box[s];
    float bb[6];
    shell_stage(pos + (size_t)s * natoms * 3, natoms, px, py, pz, part);
    if (tid < CNA_TOT) tot[tid] = 0;
    __syncthreads();
    shell_bounds(part, bb);
    float *lx = wave_all + wave * CNA_WAVE, *ly = lx + CNA_MAXV, *lz = ly + CNA_MAXV;
    unsigned int *adj = (unsigned int *)(lz + CNA_MAXV);
    float *sd = (float *)(adj + CNA_MAXV);
    int wsum = 0; // lane k < 8: column k over this wave's centres; lane 8 + t: its atoms of type t
    const int cend = c0 + SHELL_CPB < natoms ? c0 + SHELL_CPB : natoms;
    for (int c = c0 + wave; c < cend; c += SHELL_WAVES) {
        adf_wave_sync(); // the previous centre is done with the list
        const float cx = wave_uniform(px[c]), cy = wave_uniform(py[c]), cz = wave_uniform(pz[c]);
        int n[CNA_NSIG] = {0, 0, 0, 0, 0, 0, 0, 0};
        int typ = 0;
        if (!adaptive) {
            int cnt = 0;
            shell_scan(px, py, pz, natoms, cx, cy, cz, L, cube, bb, r_lo, r_hi, lane,
                       [&](int, bool in, float vx, float vy, float vz, unsigned long long m) {
                if (in) {
                    const int o = cnt + __popcll(m & ((1ull << lane) - 1ull));
                    if (o < CNA_MAXV) { lx[o] = vx; ly[o] = vy; lz[o] = vz; }
                }
                cnt += __popcll(m);
                return true;
            });
            if (cnt > CNA_MAXV) n[CNA_NSIG - 1] = cnt;
            else {
                cna_columns(lx, ly, lz, adj, cnt, r_lo, r_hi, lane, n);
                if (cnt == 12) typ = cna_close_packed(n);
                else if (cnt == 14 && n[2] == 6 && n[3] == 8) typ = 3;
            }
        } else {
            float hd = 0.0f, hx = 0.0f, hy = 0.0f, hz = 0.0f; // lane k < nh: the k-th smallest entry so far
            float thr = INFINITY;                              // the last one's d once CNA_KEEP are held
            int nh = 0;
            shell_scan(px, py, pz, natoms, cx, cy, cz, L, cube, bb, r_lo, r_hi, lane,
                       [&](int, bool in, float vx, float vy, float vz, unsigned long long) {
                const float d = cna_len(vx, vy, vz); // the scan's own d
                const bool cand = in && d < thr;
                const unsigned long long cm = __ballot(cand);
                if (cm == 0ull) return true;
                // the entries before this lane's held one (rh) and before its candidate (rk) in the order (d, scan order): held
                // entries precede every candidate of this step in the scan, the candidates follow the lanes
                int rh = lane, rk = 0;
                for (unsigned long long t = cm; t; t &= t - 1ull) {
                    const int b = __ffsll((long long)t) - 1;
                    const float db = __shfl(d, b);
                    rh += db < hd ? 1 : 0;
                    rk += (db < d || (db == d && b < lane)) ? 1 : 0;
                }
                for (int k = 0; k < nh; ++k) rk += __shfl(hd, k) <= d ? 1 : 0;
                if (lane < nh && rh < CNA_KEEP) { sd[rh] = hd; lx[rh] = hx; ly[rh] = hy; lz[rh] = hz; }
                if (cand && rk < CNA_KEEP) { sd[rk] = d; lx[rk] = vx; ly[rk] = vy; lz[rk] = vz; }
                adf_wave_sync();
                nh += __popcll(cm);
                nh = nh < CNA_KEEP ? nh : CNA_KEEP;
                if (lane < nh) { hd = sd[lane]; hx = lx[lane]; hy = ly[lane]; hz = lz[lane]; }
                adf_wave_sync();
                if (nh == CNA_KEEP) thr = __shfl(hd, CNA_KEEP - 1);
                return true;
            });
            // the list's slots 0 .. nh - 1 hold the sorted entries: the last merge left them there
            if (nh >= 12) {
                cna_columns(lx, ly, lz, adj, 12, r_lo, cna_rc(hd, 12), lane, n);
                typ = cna_close_packed(n);
                if (typ == 0 && nh >= 14) {
                    int n14[CNA_NSIG];
                    cna_columns(lx, ly, lz, adj, 14, r_lo, cna_rc(hd, 14), lane, n14);
                    if (n14[2] == 6 && n14[3] == 8) {
                        typ = 3;
#pragma unroll
                        for (int k = 0; k < CNA_NSIG; ++k) n[k] = n14[k];
                    }
                }
            }
        }
        int mine = 0;
#pragma unroll
        for (int k = 0; k < CNA_NSIG; ++k) mine = lane == k ? n[k] : mine;
        mine = lane == CNA_NSIG + typ ? 1 : mine;
        const size_t at = (size_t)s * natoms + c;
        if (sig && lane < CNA_NSIG) sig[at * CNA_NSIG + lane] = mine;
        if (type && lane == 0) type[at] = typ;
        wsum += mine;
    }
    if (lane < CNA_NSIG + CNA_NTYPE && wsum) atomicAdd(&tot[lane], wsum);
    __syncthreads();
    if (tid < CNA_NSIG) {
        if (nsig && tot[tid]) atomicAdd(&nsig[(size_t)s * CNA_NSIG + tid], tot[tid]);
    } else if (tid < CNA_NSIG + CNA_NTYPE) {
        if (ntype && tot[tid]) atomicAdd(&ntype[(size_t)s * CNA_NTYPE + tid - CNA_NSIG], tot[tid]);
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Pair entropy per atom (include/nm_distr.h, nm_distr_entropy): Piaggi and Parrinello's projection of the two-body excess entropy
// on each atom, s(c) = -2 pi rho integral over (0, r_m] of (g_m ln g_m - g_m + 1) r^2 dr with g_m the Gaussian-smeared radial
// density around c, on the grid r_k = k D, D = r_m / nbins, by the trapezoid rule; then its neighbour average sbar.
//
// Pass 1 (nm_ent_local_kernel<NA>): the grid and staging of the other shell kernels (SHELL_CPB centres per workgroup, shell_stage /
// shell_bounds, then a wave per centre in turn) and one shell_scan per centre with r_lo = 0, r_hi = r_m.  lane = grid point: a lane
// owns the points k = lane + 64 j, j < NA = ceil((nbins + 1) / 64), each with a float64 accumulator in a register (NA is a template
// argument, 1 2 4 8 or 17, so that no accumulator is indexed at run time; a point beyond nbins sits at r = infinity and never gets
// a term).  The sink sees 64 candidates at a time; it walks the set bits of the step's ballot in ascending order, that is the
// entries in scan order, takes each entry's float32 d out of its lane with v_readlane (no neighbour list is stored anywhere, so
// there is no cap on the entries), and every lane adds exp(-(r_k - d)^2 / (2 sigma^2)) to its accumulators.  A term is left out
// iff its computed exponent is below -ENT_EMAX; a block of 64 grid points that lies more than ENT_REACH sigma from d as a whole is
// skipped by a wave-uniform branch (every term of it would be left out anyway: ENT_REACH^2 / 2 exceeds ENT_EMAX by 1e-6 of it,
// the exponent's rounding is 1e-14 of it).  After the scan h_k = pref * acc, the integrand per lane, the lanes' sums over j
// ascending, then an xor butterfly over the wave (floating-point addition commutes, so all lanes hold the same bits).
// Pass 2 (nm_ent_average_kernel): the same staging, bo_scan<false> with r_hi = r_avg (indices only); for a batch, lane = entry reads
// s(a) of its entry from the global array that pass 1 wrote for the whole chunk, a butterfly adds the batch, the batches are added in
// order.  sbar(c) = (s(c) + sum) / (1 + entries).
// Both passes leave their workgroup's sum of s / sbar over its centres (a wave's centres in order, then the waves in order), and
// pass 2 its count of sbar < s_cut, in [sample][group]; nm_ent_mean_kernel adds a sample's groups in order.  No atomic of any
// kind: the result is the same bits on every call.
//
// Error bound (u = 2^-53; E = ENT_EMAX = 50; M the largest number of entries of a centre; the grid r_k = k D is the float64 product
// and belongs to the definition, so it carries no error).  For one centre let
//   A = 2 pi rho D sum' (h_k |ln(h_k / r_k^2)| + h_k + r_k^2)        (sum' the trapezoid sum over k >= 1; A >= |s|).
//   term      t = r_k - d is one rounding (d is a float32, exact in float64); the exponent -(t t) * (1 / (2 sigma^2)) carries the
//             rounding of t twice, of the square, of the constant (3 roundings) and of the product: at most 7 u relative, so at most
//             7 E u absolute, which is the relative error of the exponential; the exponential itself at most 2 ulp = 4 u:
//             (7 E + 4) u per term, all terms positive;
//   h_k       the fixed-order sum of at most M positive terms adds (M - 1) u; the prefactor 1 / (4 pi rho sigma sqrt(2 pi)) with
//             rho = natoms / L^3 at most 10 u; the product 1 u: eta = (7 E + M + 14) u relative;
//   integrand d/dh (h ln(h / r^2) - h + r^2) = ln(h / r^2), so eta moves I_k by eta h_k (|ln(h_k / r_k^2)| + eta); its own evaluation
//             (quotient, logarithm at 2 ulp, two products, two sums) at most 8 u (h_k |ln| + h_k + r_k^2);
//   sums      any order of adding the nbins + 1 weighted terms at most (nbins + 1) u sum' |I_k|; -2 pi rho D and its product 6 u;
//   together  e_s = (7 E + M + nbins + 30) u A + omitted = (M + nbins + 380) u A + omitted;
//   omitted   every term left out is below exp(-E) (1 + 1e-12), so h_k is short by at most om = M exp(-E) pref (1 + 1e-12), and with
//             phi(h) = h ln(h / r^2) - h convex, |phi(h + om) - phi(h)| <= om (1 + |ln(om / r_k^2)| + |ln(h_k / r_k^2)|) (the last
//             term only where h_k > 0): omitted = 2 pi rho D sum' of that, about 1e-19 A for M = 2200.
//   sbar      the mean of 1 + n <= 1 + M_a values (M_a the largest number of entries within r_avg), each within e_s: the largest e_s of
//             the sample plus (M_a + 2) u max |s| for the butterflies, the batches and the division;
//   means     the largest e_s (e_sbar) of the sample plus (natoms + 1) u max |s|.
// tests/entropy_ref.py holds the same expressions; the tests allow exactly that.
constexpr int ENT_MAXBINS = 1024;
constexpr int ENT_MAXACC = (ENT_MAXBINS + 1 + 63) / 64; // 17
constexpr double ENT_EMAX = 50.0;
constexpr double ENT_REACH = 10.00001;                 // sqrt(2 ENT_EMAX) and a margin

__host__ __device__ inline size_t ent_lds_bytes(int natoms, bool average) // 51,332 B at 4095 atoms for the average pass
{
    return (size_t)SHELL_WAVES * (sizeof(double) + sizeof(int)) + (average ? (size_t)SHELL_WAVES * BO_LIST * sizeof(int) : 0)
         + ((size_t)3 * natoms + SHELL_WAVES * 6) * sizeof(float);
}

template <int NA>
__global__ void __launch_bounds__(SHELL_BLOCK)
nm_ent_local_kernel(int natoms, const float *__restrict__ pos, const float *__restrict__ box, double r_m, float cube, double sigma,
                    double inv2s2, int nbins, double D, double *__restrict__ sl, int *__restrict__ nnb, double *__restrict__ psum)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int groups = (natoms + SHELL_CPB - 1) / SHELL_CPB;
    const int s = blockIdx.x / groups, grp = blockIdx.x % groups, c0 = grp * SHELL_CPB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double *wsum = (double *)smem;
    float *px = (float *)((int *)(wsum + SHELL_WAVES) + SHELL_WAVES), *py = px + natoms, *pz = py + natoms, *part = pz + natoms;
    const float L = box[s];
    float bb[6];
    shell_stage(pos + (size_t)s * natoms * 3, natoms, px, py, pz, part);
    __syncthreads();
    shell_bounds(part, bb);
    const double PI = 3.14159265358979323846, Ld = (double)L, rho = (double)natoms / (Ld * Ld * Ld);
    const double pref = 1.0 / (4.0 * PI * rho * sigma * 2.50662827463100050242); // sqrt(2 pi)
    const double reach = ENT_REACH * sigma;
    double rk[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) rk[j] = lane + 64 * j <= nbins ? (double)(lane + 64 * j) * D : INFINITY;
    double wtot = 0.0;
    const int cend = c0 + SHELL_CPB < natoms ? c0 + SHELL_CPB : natoms;
    for (int c = c0 + wave; c < cend; c += SHELL_WAVES) {
        const float cx = wave_uniform(px[c]), cy = wave_uniform(py[c]), cz = wave_uniform(pz[c]);
        double acc[NA];
#pragma unroll
        for (int j = 0; j < NA; ++j) acc[j] = 0.0;
        int nb = 0;
        shell_scan(px, py, pz, natoms, cx, cy, cz, L, cube, bb, 0.0, r_m, lane,
                   [&](int, bool, float vx, float vy, float vz, unsigned long long m) {
            nb += __popcll(m);
            const int df = __float_as_int(cna_len(vx, vy, vz)); // the scan's own d
            for (; m; m &= m - 1ull) {
                const int src = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
                const double d = (double)__int_as_float(__builtin_amdgcn_readlane(df, src));
#pragma unroll
                for (int j = 0; j < NA; ++j) {
                    if (NA > 1 && (d < (double)(64 * j) * D - reach || d > (double)(64 * j + 63) * D + reach)) continue; // wave-uniform
                    const double t = rk[j] - d, e = -(t * t) * inv2s2;
                    if (e >= -ENT_EMAX) acc[j] += exp(e);
                }
            }
            return true;
        });
        double sum = 0.0;
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            const int k = lane + 64 * j;
            if (k >= 1 && k <= nbins) {
                const double r2 = rk[j] * rk[j], h = pref * acc[j];
                const double I = h > 0.0 ? h * log(h / r2) - h + r2 : r2;
                sum += k == nbins ? 0.5 * I : I;
            }
        }
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        const double sv = -(2.0 * PI * rho * D) * sum;
        const size_t at = (size_t)s * natoms + c;
        if (lane == 0) {
            sl[at] = sv;
            if (nnb) nnb[at] = nb;
        }
        wtot += sv;
    }
    if (lane == 0) wsum[wave] = wtot;
    __syncthreads();
    if (tid == 0) {
        double t = wsum[0];
        for (int w = 1; w < SHELL_WAVES; ++w) t += wsum[w];
        psum[(size_t)s * groups + grp] = t;
    }
}

__global__ void __launch_bounds__(SHELL_BLOCK)
nm_ent_average_kernel(int natoms, const float *__restrict__ pos, const float *__restrict__ box, double r_avg, float cube, double s_cut,
                      const double *__restrict__ sl, double *__restrict__ sbar, double *__restrict__ psum, int *__restrict__ plow)
{
    extern __shared__ __align__(16) unsigned char smem[];
    const int groups = (natoms + SHELL_CPB - 1) / SHELL_CPB;
    const int s = blockIdx.x / groups, grp = blockIdx.x % groups, c0 = grp * SHELL_CPB;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double *wsum = (double *)smem;
    int *wlow = (int *)(wsum + SHELL_WAVES), *li_all = wlow + SHELL_WAVES;
    float *px = (float *)(li_all + SHELL_WAVES * BO_LIST), *py = px + natoms, *pz = py + natoms, *part = pz + natoms;
    const float L = box[s];
    float bb[6];
    shell_stage(pos + (size_t)s * natoms * 3, natoms, px, py, pz, part);
    __syncthreads();
    shell_bounds(part, bb);
    int *li = li_all + wave * BO_LIST;
    const double *ss = sl + (size_t)s * natoms;
    double wtot = 0.0;
    int low = 0;
    const int cend = c0 + SHELL_CPB < natoms ? c0 + SHELL_CPB : natoms;
    for (int c = c0 + wave; c < cend; c += SHELL_WAVES) {
        const float cx = wave_uniform(px[c]), cy = wave_uniform(py[c]), cz = wave_uniform(pz[c]);
        double a = 0.0;
        const int nb = bo_scan<false>(px, py, pz, natoms, cx, cy, cz, L, cube, bb, 0.0, r_avg, nullptr, nullptr, nullptr, li, lane, [&](int mb) {
            double v = lane < mb ? ss[li[lane]] : 0.0; // lane = entry
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            a += v;
        });
        const double b = (ss[c] + a) / (double)(nb + 1);
        if (sbar && lane == 0) sbar[(size_t)s * natoms + c] = b;
        wtot += b;
        low += b < s_cut ? 1 : 0;
    }
    if (lane == 0) { wsum[wave] = wtot; wlow[wave] = low; }
    __syncthreads();
    if (tid == 0) {
        double t = wsum[0];
        int n = wlow[0];
        for (int w = 1; w < SHELL_WAVES; ++w) { t += wsum[w]; n += wlow[w]; }
        psum[(size_t)s * groups + grp] = t;
        plow[(size_t)s * groups + grp] = n;
    }
}

// one thread per sample: the groups' sums in order, the means over the atoms and the count below the cut
__global__ void __launch_bounds__(64)
nm_ent_mean_kernel(int ns, int natoms, int groups, const double *__restrict__ ps, const double *__restrict__ pb, const int *__restrict__ pl,
                   double *__restrict__ smean, double *__restrict__ sbarmean, int *__restrict__ nlow)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= ns) return;
    double ts = 0.0, tb = 0.0;
    int n = 0;
    for (int g = 0; g < groups; ++g) {
        ts += ps[(size_t)s * groups + g];
        if (pb) { tb += pb[(size_t)s * groups + g]; n += pl[(size_t)s * groups + g]; }
    }
    if (smean) smean[s] = ts / (double)natoms;
    if (sbarmean) sbarmean[s] = tb / (double)natoms;
    if (nlow) nlow[s] = n;
}

} // namespace nm
