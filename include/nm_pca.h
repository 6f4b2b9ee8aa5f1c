/*
 * nm_pca.h — C-ABI of the principal component stage: the moments of a set of feature vectors and their
 * projections on given components.  The reference embeds distr's histograms with a VAE and applies PCA to the latents
 * (lammps_vae.py); this is the linear form of that stage, and the definitions below are the build's own.
 *
 * Samples.  x[n][j], n = 0..N-1 samples of j = 0..D-1 features, float32, row-major, in host memory.
 * Moments (nm_pca_moments).
 *   mean[j]    = (sum_n x[n][j]) / N
 *   lo[j], hi[j] = the smallest and the largest x[n][j] over n, exact
 *   gram[i][j] = sum_n a[n][i] a[n][j],  a[n][j] = x[n][j] - mean[j] with the RETURNED mean, the difference taken in float64;
 *                all D x D entries, gram[i][j] == gram[j][i] bit for bit.
 *   The covariance under a scaling s_j of the features is gram[i][j] / (s_i s_j (N - 1)): the caller's arithmetic.
 * Projections (nm_pca_project), for components comp[c][j], c = 0..ncomp-1:
 *   y[n][j]  = (x[n][j] - mean[j]) * inv_scale[j]
 *   z[n][c]  = sum_j y[n][j] comp[c][j]
 *   norm2[n] = sum_j y[n][j]^2            (norm2 - sum_c z^2 is the squared distance to the components' span, if they are orthonormal)
 * Arithmetic.  float64 throughout: a float32 converts exactly, the Gram products are accumulated by the float64 matrix
 *   instruction (fused multiply-adds).  Every sum runs in a fixed order that depends on N and D alone: the same bits on every
 *   call and on every device, no floating-point atomics, nothing depends on the number of compute units.  x need not fit the
 *   device: it is processed in batches of 32768 samples and kept on the device between the two passes of nm_pca_moments when it fits.
 * Error bound, u = 2^-53, k u short for k u / (1 - k u) (derivation: csrc/nm_pca.h):
 *   mean:  (min(N - 1, 258 + ceil(N / 1024)) + 1) u (sum_n |x[n][j]|) / N
 *   gram:  (M + S + 1) u sum_n |a[n][i] a[n][j]|,  M = min(N, ceil(N / 32768) 4096),  S = min(8, ceil(N / 4096))
 *   z:     (min(D, ceil(D / 64) + 6) + 2) u sum_j |y[n][j] comp[c][j]|
 *   norm2: (min(D, ceil(D / 64) + 6) + 4) u norm2[n]
 *   These lie below (N + 2) u, (N + 8) u, (D + 4) u and (D + 4) u of the same sums, the bounds of a summation in sample order.
 *   A column of N <= 2^29 equal values has an exact mean, and its row and column of gram are exactly 0.
 *
 * Both functions return 0 or a negative NM_ERR_* code (include/nm.h); message via nm_pca_last_error(), starting with the
 * function's name.  NM_ERR_ARG, checked before the device is looked for and with every output left untouched, for: nfeat
 * outside 1..4096, nsamples < 2, nsamples * nfeat > 2^40, ncomp outside 1..64 or above nfeat, a non-finite value in mean,
 * inv_scale or comp, a needed pointer that is null (norm2 may be), a negative device ordinal.  A value of x that is not finite
 * is found on the device by the first pass over x: NM_ERR_ARG, the message names the first such sample, the outputs are left
 * untouched.  NM_ERR_HIP without a device or when a HIP call fails.
 */
#ifndef NM_PCA_H
#define NM_PCA_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* x [nsamples][nfeat]; mean, lo, hi [nfeat]; gram [nfeat][nfeat]. */
int nm_pca_moments(int device, int64_t nsamples, int nfeat, const float *x, double *mean, double *lo, double *hi, double *gram);

/* x [nsamples][nfeat]; mean, inv_scale [nfeat]; comp [ncomp][nfeat]; z [nsamples][ncomp]; norm2 [nsamples] or NULL. */
int nm_pca_project(int device, int64_t nsamples, int nfeat, const float *x, const double *mean, const double *inv_scale, int ncomp,
                   const double *comp, double *z, double *norm2);

/* Where the device time of the calling thread's last successful call went, in milliseconds between device events: ms[0] the
 * uploads of x (and of the small arguments), ms[1] the first pass of nm_pca_moments (column sums, extremes, screen), ms[2] its Gram
 * pass, ms[3] the kernels of nm_pca_project.  The downloads of the results are not in it. */
int nm_pca_last_timing(double *ms);

const char *nm_pca_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
