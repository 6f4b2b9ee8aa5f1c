/*
 * nm_tsne.h — C-ABI of the manifold stage: t-SNE of a set of points, the default manifold (-mf) that the
 * reference applies to its PCA projections before it clusters them (lammps_vae.py).  The definitions below are the build's own;
 * they are sklearn.manifold.TSNE's quantities (_binary_search_perplexity, _kl_divergence at one degree of freedom,
 * _gradient_descent) with the exact all-pairs sum in place of the Barnes-Hut tree: no angle parameter, no approximation.
 * Every array lives in host memory, float64 unless said otherwise; calls are stateless.  u = 2^-53 below.
 *
 * Points.  x[n][c], n = 0..N-1 points of c = 0..ndim-1 coordinates, row-major.
 * Distance.  d2(i, j) = sum_c (x[i][c] - x[j][c])^2 in float64, c ascending, every difference, product and sum rounded on its own
 *   (no fused multiply-add): the value of include/nm_cluster.h's definition evaluated without contraction, the same bits wherever
 *   a pair is formed and d2(i, j) == d2(j, i).  Error at most (ndim + 2) u d2.
 * Neighbours.  nbr[i][0..k-1] (int32) are the k points j != i with the smallest (d2(i, j), j) in lexicographic order, stored in
 *   that order: duplicates and ties are decided by the index.  The selection is exact (a radix select on the bits of d2 over
 *   repeated all-pairs scans, then a gather and a sort of the survivors).
 * Conditional probabilities.  With d_m = d2(i, nbr[i][m]), t_m = d_m - dmin and dmin = d_0:
 *     e_m = exp(-(beta_i t_m)),  S_i = sum_m e_m,  p[i][m] = e_m / S_i,  H_i = ln S_i + beta_i ((sum_m t_m e_m) / S_i).
 *   beta_i is the root of H_i = ln(perplexity), found by sklearn's bracketing: beta = 1; where H > ln(perplexity) the lower end
 *   becomes beta and beta is doubled while the upper end is unbounded, else set to the mean of beta and the upper end; where
 *   H < ln(perplexity) the same downwards (halved while the lower end is unbounded).  It ends where H == ln(perplexity), where the
 *   next iterate equals the present one, or after 200 evaluations; beta_i is the last iterate formed, and p is evaluated at it.
 *   There is no entropy tolerance.  A row whose perplexity cannot be met because its entries at dmin outnumber it (all k distances
 *   equal, for instance) is doubled 200 times: beta_i = 2^200, p uniform over the entries at dmin and 0 elsewhere.  Defined
 *   behaviour, no error.
 *   Bounds.  The sums run over non-negative terms in a fixed order (a thread adds every 256th term, a binary tree joins the 256).
 *   With B = ceil(k / 256) + 32:  |sum_m p[i][m] - 1| <= B u;  p[i][m] differs from exp(-(beta_i t_m)) / S by at most
 *   (B + beta_i t_m) u of itself; and |H_i(beta_i) - ln(perplexity)| <= B u (1 + ln k + M2_i) for every row that has a root, with
 *   M2_i = sum_m (beta_i t_m)^2 p[i][m]  (csrc/nm_tsne.h derives them).
 * Symmetric affinities.  P_ij = (p_{j|i} + p_{i|j}) / (2 N), a direction that is in no list counting 0.  The library builds them
 *   from the directed lists itself, once per call; the in-degree of a point is not bounded (a hub in every list has N - 1).
 * Embedding.  y[n][c], c = 0..ncomp-1, ncomp in 1..3.  d2_y as d2 above.
 *     w_ij = 1 / (1 + d2_y(i, j)) (within 2 u in the all-pairs pass: csrc/nm_tsne.h, ts_rcp),  Z = sum_{i != j} w_ij,
 *     grad_i = 4 sum_j (exaggeration P_ij - w_ij / Z) w_ij (y_i - y_j),
 *     kl = sum_{P_ij > 0} P_ij ln(P_ij Z / w_ij), always with the P that is not exaggerated.
 *   The repulsive sum runs over all pairs, exactly; one all-pairs pass gives its row sums and Z.
 *   Bound, per component c of grad_i:  (3 N + k + 64) u times 4 sum_j (exaggeration P_ij + w_ij / Z) w_ij |y_i[c] - y_j[c]|; Z to
 *   (N + 64) u of itself; kl to (3 N + k + 64) u times sum P_ij (|ln P_ij| + ln(1 + d2_y) + |ln Z|)  (csrc/nm_tsne.h).
 * Descent.  One step, element by element, every operation rounded on its own, g the gradient at the y before the step:
 *     inc = update * g < 0;  gains = inc ? gains + 0.2 : gains * 0.8;  gains = max(gains, 0.01);
 *     update = momentum * update - learning_rate * (g * gains);  y = y + update.
 *   niter steps run on the device without a way to the host between them.  No early stopping: the caller composes the schedule.
 * Determinism.  Every sum runs in an order that depends on the sizes alone; there are no floating-point atomics (integer atomics
 *   join the counts of the selection).  Every output is the same bytes on every call.
 * Memory.  O(npoints (ndim + k)) on the device; no N x N array exists at any time.
 *
 * Returns 0 or a negative NM_ERR_* code (include/nm.h); message via nm_tsne_last_error(), starting with the function's name.
 * NM_ERR_ARG is checked before the device is looked for and leaves every output untouched; the order is the one given at each
 * function.  A value of x that is not finite is found on the device by a first screen, as nm_cluster_dbscan finds it; a value of
 * y, update or gains that is not finite, an entry of nbr that is the row itself or no point, and a p that is negative or not finite
 * are found on the host while the symmetric lists are built, before a device is looked for: NM_ERR_ARG, the message names the
 * first such point, the outputs are left untouched.  NM_ERR_HIP without a device or when a HIP call fails.
 */
#ifndef NM_TSNE_H
#define NM_TSNE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* x [npoints][ndim]; nbr (int32), p [npoints][k]; beta [npoints].  NM_ERR_ARG for, in this order: npoints outside 2..2^20, ndim
 * outside 1..16, k outside 1..min(npoints - 1, 4096), a perplexity that is not finite or not in (1, k), a pointer that is null, a
 * negative device ordinal. */
int nm_tsne_affinities(int device, int64_t npoints, int ndim, const double *x, double perplexity, int k, int32_t *nbr, double *p,
                       double *beta);

/* nbr, p [npoints][k] as above (any directed lists: an entry may be any point but the row's own, a row's entries are distinct);
 * y, grad [npoints][ncomp]; kl, z [1].  NM_ERR_ARG for, in this order: npoints outside 2..2^20, k outside 1..min(npoints - 1,
 * 4096), ncomp outside 1..3, an exaggeration that is not finite or not > 0, a pointer that is null, a negative device ordinal. */
int nm_tsne_gradient(int device, int64_t npoints, int k, const int32_t *nbr, const double *p, int ncomp, const double *y,
                     double exaggeration, double *grad, double *kl, double *z);

/* y, update, gains [npoints][ncomp], read and written in place; trace [niter][3]: kl, Z and the 2-norm of the gradient of each
 * step (at the y before it).  NM_ERR_ARG for, in this order: npoints, k, ncomp as above, niter outside 1..2^20, an exaggeration
 * that is not finite or not > 0, a momentum that is not finite or not in [0, 1), a learning rate that is not finite or not > 0, a
 * pointer that is null, a negative device ordinal. */
int nm_tsne_descend(int device, int64_t npoints, int k, const int32_t *nbr, const double *p, int ncomp, double *y, double *update,
                    double *gains, int niter, double exaggeration, double momentum, double learning_rate, double *trace);

/* Where the device time of the calling thread's last successful call went, in milliseconds between device events.  After
 * nm_tsne_affinities: ms[0] the upload of x and the screen, ms[1] the radix select (64 counting scans), ms[2] the gather, ms[3] the
 * sort and the search for beta; ms[4] = 0.  After nm_tsne_gradient and nm_tsne_descend: ms[0] the uploads and the sums over P that
 * do not change with y (the symmetric lists are built on the host before them and are not in it); of the first step ms[1] the
 * attractive sums, ms[2] the all-pairs pass, ms[3] the joins, the gradient and the update; ms[4] all steps together.  The downloads
 * of the results are not in it. */
int nm_tsne_last_timing(double *ms);

const char *nm_tsne_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
