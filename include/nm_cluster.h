/*
 * nm_cluster.h — C-ABI of the cluster stage: DBSCAN of a set of points, the default clustering (-cl) that the
 * reference applies to its embedding (lammps_vae.py).  The definitions below are the build's own; off ties they give the labels of
 * sklearn.cluster.DBSCAN(eps, min_samples=min_pts, algorithm='brute').
 *
 * Points.  x[n][c], n = 0..N-1 points of c = 0..ndim-1 coordinates, float64, row-major, in host memory.
 * Distance.  d2(i, j) = sum_c (x[i][c] - x[j][c])^2 in float64, c ascending, one device function for every pass: a pair has the
 *   same bits wherever it is formed, and d2(i, j) == d2(j, i) bit for bit (the differences are negated, the squares and their order
 *   are the same).  Error at most (ndim + 2) u d2, u = 2^-53.  i and j are neighbours iff d2(i, j) <= eps * eps, the bound
 *   included, the product rounded once on the host.
 * Degree.  degree[i] = the number of neighbours of i, i itself among them (sklearn's convention).  i is a core point iff
 *   degree[i] >= min_pts.
 * Clusters.  The connected components of the core points under the neighbour relation, numbered 0, 1, ... in ascending order of
 *   their smallest core index; nclusters is their number.
 * Borders and noise.  A point that is not core and has a core neighbour is a border point and takes the lowest cluster number
 *   among its core neighbours.  Every other point that is not core is noise: label -1.
 *   (sklearn expands the clusters in index order, each completely before the next: the same numbering and the same border rule.)
 * Determinism.  Every output is an integer and a property of the input alone: the same bytes on every call and on every device,
 *   whatever the schedule.  Integer atomics only.
 * Memory.  O(npoints ndim) on the device; no N x N array exists at any time.  The work is N^2 distance tests per pass, three passes.
 *
 * Returns 0 or a negative NM_ERR_* code (include/nm.h); message via nm_cluster_last_error(), starting with the function's name.
 * NM_ERR_ARG, checked before the device is looked for and with every output left untouched, for, in this order: npoints outside
 * 1..2^21, ndim outside 1..16, an eps that is not finite or not > 0, min_pts < 1, a pointer that is null, a negative device
 * ordinal.  A value of x that is not finite is found on the device by a first screen: NM_ERR_ARG, the message names the first
 * such point, the outputs are left untouched.  NM_ERR_HIP without a device or when a HIP call fails.
 */
#ifndef NM_CLUSTER_H
#define NM_CLUSTER_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* x [npoints][ndim]; label, degree [npoints]; nclusters [1]. */
int nm_cluster_dbscan(int device, int64_t npoints, int ndim, const double *x, double eps, int min_pts, int32_t *label, int32_t *degree,
                      int32_t *nclusters);

/* Where the device time of the calling thread's last successful call went, in milliseconds between device events: ms[0] the upload
 * of x and the screen, ms[1] the degree pass, ms[2] the union pass and the flattening of the roots, ms[3] the numbering (the roots'
 * way to the host, the pass over them there and the numbers' way back), ms[4] the border pass.  The downloads of the results are not
 * in it. */
int nm_cluster_last_timing(double *ms);

const char *nm_cluster_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
