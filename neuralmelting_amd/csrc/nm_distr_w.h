// nm_distr_w.h — the third-order Steinhardt invariants (include/nm_distr.h, nm_distr_bondorder_w) over the moments of nm_distr.h:
//   T_l(a) = (4 pi / (2l+1))^(3/2) Re sum_{m1+m2+m3=0} (l l l; m1 m2 m3) a_m1 a_m2 a_m3,   a_-m = (-1)^m conj(a_m),
// for a = q_lm(c) (w3), a = qbar_lm(c) (wbar3) and a = Q_lm (W3), even l only (for odd l the symbol changes its sign under the exchange
// of two columns, so the sum vanishes).  Included by nm_distr_api.hip behind nm_distr.h.
//
// The table (built on the host, nm_distr_api.hip: bo_w_table): for l = 2, 4, .., 12 in turn the terms (m1, m2) with m1 = -l..l
// ascending (outer), m2 = -l..l ascending (inner) and |m1 + m2| <= l, m3 = -m1 - m2, without the symbols that vanish (the integer sum
// of Racah's formula is 0: twelve at l = 8, none elsewhere): n_l = 19, 61, 127, 205, 331, 469 terms, 1212 in all.  A term is its
// coefficient (4 pi / (2l+1))^(3/2) (l l l; m1 m2 m3), formed in long double and rounded once, and the three positions m + l in one
// int (8 bits each).  That order is part of the definition of the returned bits.
//
// The contraction (bo_w_contract), one wave per vector: the stored half m >= 0 is expanded to the 2l+1 complex components in the
// wave's LDS row; then lane = term k0 + lane for k0 = 0, 64, ..: the lane multiplies its three components, keeps the real part
// ((ab)_r c_r - (ab)_i c_i) and scales it by the coefficient; the 64 lanes meet in the butterfly of xor 32, 16, .., 1 (an addition
// commutes, so every lane ends with the same bits), and the ceil(n_l / 64) <= 8 steps add in order.  Every sum runs in a fixed
// order: the same bits on every call, no atomics.
//
// Where the vectors come from:
//   w3     nm_bo_w_kernel: a wave reads q_lm(c) as nm_bo_moments_kernel (launched unchanged) left it in the scratch;
//   wbar3  nm_bo_w_average_kernel: bo_average_centres, the scan and gather of nm_bo_average_kernel itself, leaves qbar_lm(c) in LDS;
//          the finish forms qbar2 with nm_bo_average_kernel's own expression (the same bits) and the cubic invariant beside it;
//   W3     nm_bo_w_global_kernel: bo_global_moments, the ordered partial sums of nm_bo_global_kernel itself, then Q2 and W3.
//
// Error bound (u = 2^-53).  Write b = sqrt(4 pi / (2l+1)) a for the scaled vector, |b|^2 = x the matching square (q2, qbar2, Q2), and
// T_l(a) = F(b, b, b) with the trilinear F(b, c, d) = sum (3j) b_m1 c_m2 d_m3.  The symbols obey sum_{m1, m2} (3j)^2 = 1, so by
// Cauchy-Schwarz |F(b, c, d)| <= sqrt(sum_{m1, m2} |b_m1|^2 |c_m2|^2 |d_m3|^2) <= |b| |c| |d|, and likewise sum |(3j) b_m1 c_m2 d_m3|
// <= |b| |c| |d|.
//   vector   nm_distr.h bounds the computed b' against the exact b: |b' - b| <= e, an absolute error of the scaled vector (e = e_q,
//            e_qbar, e_Q; it is what gives |dx| <= 2 e sqrt(x) + e^2).  Trilinearity: |F(b', b', b') - F(b, b, b)| <=
//            3 e x + 3 e^2 sqrt(x) + e^3.
//   terms    a coefficient carries 2 u (long double arithmetic of some 60 operations at 2^-64 each, one rounding), the two complex
//            products and the scaling at most 10 u more against |coef| |b_m1| |b_m2| |b_m3| (each component of a complex product
//            is two products and a sum: 2 u of |b| |c| up to second order, with or without a fused multiply-add): 12 u per term.
//   sum      any order of n_l terms adds at most (n_l - 1) u sum |term|.
//   together |w3 - exact| <= 3 e x + 3 e^2 sqrt(x) + e^3 + (n_l + 12) u (sqrt(x) + e)^3, the last factor being the bound of
//            sum |term| for the computed vector.  Up to M = 529 neighbours and 4095 atoms (e_Q = 1193 u at l = 12) that is below 5e-13.
// tests/bondorder_w_ref.py holds the same expression; the tests allow exactly that.
#pragma once
#include "nm_distr.h"

namespace nm {

constexpr int BO_W_TERMS = 1212; // 19 + 61 + 127 + 205 + 331 + 469

// terms of l (3 l^2 + 3 l + 1 triples, twelve vanishing symbols at l = 8 left out), and where they start in the table
__host__ __device__ __forceinline__ int bo_w_terms(int l) { return 3 * l * l + 3 * l + 1 - (l == 8 ? 12 : 0); }
__host__ __device__ __forceinline__ int bo_w_off(int l)
{
    int off = 0;
    for (int j = 2; j < l; j += 2) off += bo_w_terms(j);
    return off;
}

// the table on the device
struct BoW { const double *coef; const int *idx; };

// T_l of the vector whose stored half (m >= 0: re, im in turn) lies at `half` in LDS, written and made visible to the wave before the
// call; `full` is the wave's own 2 (2l+1) doubles of LDS.  Every lane returns the same value.
__device__ __forceinline__ double bo_w_contract(const double *half, int l, double *full, const BoW &w, int lane)
{
    if (lane < 2 * l + 1) {
        const int m = lane - l, k = m < 0 ? -m : m;
        const double re = half[2 * k], im = half[2 * k + 1];
        const double sg = (m < 0 && (k & 1)) ? -1.0 : 1.0;   // a_-k = (-1)^k conj(a_k)
        full[2 * lane] = sg * re;
        full[2 * lane + 1] = m < 0 ? -(sg * im) : im;
    }
    adf_wave_sync();
    const int n = bo_w_terms(l);
    const double *coef = w.coef + bo_w_off(l);
    const int *idx = w.idx + bo_w_off(l);
    double t = 0.0;
    for (int k0 = 0; k0 < n; k0 += 64) {
        const int k = k0 + lane;
        double v = 0.0;
        if (k < n) {
            const int p = idx[k];
            const double *a = full + 2 * (p & 255), *b = full + 2 * ((p >> 8) & 255), *c = full + 2 * ((p >> 16) & 255);
            const double pr = a[0] * b[0] - a[1] * b[1], pi = a[0] * b[1] + a[1] * b[0];
            v = coef[k] * (pr * c[0] - pi * c[1]);
        }
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        t += v;
    }
    adf_wave_sync(); // the next call writes `full` again
    return t;
}

// the cubic invariants of the set's l for one vector set (all l, layout of the moments) at `vec` in LDS: lane 0 writes out[i]
__device__ __forceinline__ void bo_w_all(const BoSet &set, const double *vec, double *full, const BoW &w, int lane, double *__restrict__ out)
{
    for (int i = 0; i < set.nl; ++i) {
        const int l = bo_l_of(set, i);
        const double t = bo_w_contract(vec + 2 * bo_off(set, l), l, full, w, lane);
        if (lane == 0) out[i] = t;
    }
}

constexpr int BO_W_FULL = 2 * (2 * BO_LMAX + 1);          // doubles of a wave's expanded vector
constexpr int BO_W_ROW = 2 * BO_MAXL * (BO_LMAX + 1);     // doubles of one atom's moments at the most (as nm_bo_global_kernel's)

// w3: one wave per atom of the chunk; nvec = samples x atoms
__global__ void __launch_bounds__(SHELL_BLOCK)
nm_bo_w_kernel(int nvec, BoSet set, const double *__restrict__ qlm, BoW w, double *__restrict__ w3)
{
    __shared__ double row_all[SHELL_WAVES * BO_W_ROW], full_all[SHELL_WAVES * BO_W_FULL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nc2 = 2 * set.nc;
    const long long v = (long long)blockIdx.x * SHELL_WAVES + wave;
    if (v >= nvec) return; // the whole wave; no workgroup barrier follows
    double *row = row_all + wave * BO_W_ROW;
    for (int j = lane; j < nc2; j += 64) row[j] = qlm[(size_t)v * nc2 + j];
    adf_wave_sync();
    bo_w_all(set, row, full_all + wave * BO_W_FULL, w, lane, w3 + (size_t)v * set.nl);
}

// where the waves' expanded vectors start in the dynamic LDS of nm_bo_w_average_kernel: behind nm_bo_average_kernel's layout
__host__ __device__ inline size_t bo_w_full_at(int natoms, int nc) { return (bo_lds_bytes(natoms, nc, false) + 15) & ~(size_t)15; }
__host__ __device__ inline size_t bo_w_lds_bytes(int natoms, int nc) { return bo_w_full_at(natoms, nc) + (size_t)SHELL_WAVES * BO_W_FULL * sizeof(double); }

// wbar3, and qbar2 where it is asked for: nm_bo_average_kernel's centres with the cubic invariant in the finish
__global__ void __launch_bounds__(SHELL_BLOCK)
nm_bo_w_average_kernel(int natoms, const float *__restrict__ pos, const float *__restrict__ box, double r_lo, double r_hi, float cube,
                       BoSet set, const double *__restrict__ qlm, BoW w, double *__restrict__ qbar2, double *__restrict__ wbar3)
{
    extern __shared__ __align__(16) unsigned char smem[];
    double *full = (double *)(smem + bo_w_full_at(natoms, set.nc)) + (threadIdx.x >> 6) * BO_W_FULL;
    bo_average_centres(natoms, pos, box, r_lo, r_hi, cube, set, qlm, [&](int s, int c, const double *qbar, int lane) {
        if (qbar2) bo_average_invariant(set, natoms, s, c, qbar, lane, qbar2);
        bo_w_all(set, qbar, full, w, lane, wbar3 + ((size_t)s * natoms + c) * set.nl);
    });
}

// W3, and Q2 where it is asked for: nm_bo_global_kernel's moments; the first wave contracts
__global__ void __launch_bounds__(128)
nm_bo_w_global_kernel(int groups, BoSet set, const double *__restrict__ partial, const int *__restrict__ pcount, BoW w,
                      double *__restrict__ Q2, double *__restrict__ W3)
{
    __shared__ double q[BO_W_ROW], full[BO_W_FULL];
    const int s = blockIdx.x, tid = threadIdx.x;
    bo_global_moments(groups, set, partial, pcount, s, q);
    if (Q2 && tid < set.nl) {
        const int l = bo_l_of(set, tid);
        Q2[(size_t)s * set.nl + tid] = bo_invariant(q + 2 * bo_off(set, l), l);
    }
    if (tid < 64) bo_w_all(set, q, full, w, tid, W3 + (size_t)s * set.nl);
}

} // namespace nm
