/*
 * nm_distr.h — C-ABI of the structural-histogram kernels, the step right after the sampler:
 * walkernr/neuralMelting's scripts/lammps_distr.py computes, for every recorded sample, the radial distribution over the
 * 27 periodic images (calculate_rdf, lammps_distr.py:123-135) and a 3-D histogram of pair displacement vectors
 * (calculate_cdf, lammps_distr.py:161-171) with np.histogram / np.histogramdd on float32 coordinates.
 *
 * nm_distr_histograms replaces both per-sample functions for a batch of samples.  It returns the raw integer counts the
 * reference accumulates before its division by natoms (bit-exact: same float32 arithmetic for the displacements, same
 * float64 edge comparisons and edge-inclusion rules as numpy), as float32 like the reference's `rd` / `cd` arrays.
 */
#ifndef NM_DISTR_H
#define NM_DISTR_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* pos[ns][natoms][3], box[ns] float32 (lammps_parse.py's .pos.npy / .box.npy);
 * r_edges[sbins] float64 = R of calculate_spatial (lammps_distr.py:84-95): sbins-1 bins, result written to rdf[s][1..sbins-1],
 *   rdf[s][0] = 0 (rd[1:] += np.histogram(d, r)[0]);
 * rv_edges[cbins+1] float64 = RV[0] of calculate_spatial (lammps_distr.py:111-113), the same edges in x, y and z;
 * rdf[ns][sbins], cdf[ns][cbins][cbins][cbins] float32 counts summed over the 27 images, NOT yet divided by natoms.
 * Either output may be NULL: that histogram is neither computed nor written, and its edges and bin count are not read.
 * Returns 0 or a negative NM_ERR_* code (include/nm.h); message via nm_distr_last_error().  NM_ERR_ARG for bad arguments
 * (natoms outside 1..4095, sbins outside 2..256, cbins outside 1..32, a working set beyond 160 KiB of LDS, a bad device
 * ordinal): the outputs are left untouched.  NM_ERR_ARG also when a returned count reaches 2^24 (a bin can hold more than
 * natoms^2 counts, because a displacement on +-l/2 lies in two periodic images per axis): float32 counts are no longer
 * exact there, and the outputs hold unspecified values. */
int nm_distr_histograms(int device, int ns, int natoms, const float *pos, const float *box, int sbins,
                        const double *r_edges, int cbins, const double *rv_edges, float *rdf, float *cdf);
const char *nm_distr_last_error(void);

/* Angular (bond-angle) distribution: the quantity lammps_distr.py names .a.npy / .adf.npy but leaves switched off.
 * Definition (the build's own; the reference's disabled code is not well-defined), for sample s and centre atom c:
 *   neighbours  (j, a) over the 27 image shifts br[j] (lammps_distr.py:99-102) and all atoms a, with
 *               v = pos[a] - (pos[c] + box*br[j]) in float32, d = float32 sqrt of the sequential float32 sum of the three
 *               squares (as the rdf), and r_lo < (double)d <= r_hi;
 *   triplets    every unordered pair of distinct neighbours (v1, v2) of the same centre; in float64 from the float32
 *               components n_i = (x_i*x_i + y_i*y_i) + z_i*z_i, dot = (x1*x2 + y1*y2) + z1*z2,
 *               cth = clip(dot / sqrt(n1*n2), -1, 1);
 *   bins        in cosine space: cos_edges[abins] = cos(a[k]) for the angle edges a, strictly decreasing; bin k
 *               (0 <= k <= abins-2) holds cos_edges[k] >= cth > cos_edges[k+1], the last bin also cth == cos_edges[abins-1]
 *               (np.histogram(theta, a) without an acos); outside is dropped;
 *   result      adf[s][k+1] += 1, adf[s][0] = 0 (ad[1:] += histogram, lammps_distr.py:107): raw counts, each unordered pair
 *               once, NOT divided by natoms.
 * pos[ns][natoms][3], box[ns] float32; adf[ns][abins] unsigned 64-bit (one bin can hold natoms * M^2 / 2 counts for M
 * neighbours per centre).  Any number of neighbours per centre is handled.
 * Returns 0 or a negative NM_ERR_* code; message via nm_distr_last_error(), starting with "nm_distr_angles:".  NM_ERR_ARG,
 * checked before the device is looked for and with adf left untouched, for: ns < 0, natoms outside 1..4095, abins outside
 * 2..256, edges not strictly decreasing, not 0 <= r_lo < r_hi, r_hi > min(box)/2 over the batch (an atom could neighbour its
 * own image), a null pointer, a bad device ordinal.  ns == 0 is NM_OK. */
int nm_distr_angles(int device, int ns, int natoms, const float *pos, const float *box, double r_lo, double r_hi, int abins,
                    const double *cos_edges, uint64_t *adf);

/* Static structure factor on the reciprocal lattice of each sample's box: the quantity lammps_distr.py names .q.npy / .sf.npy
 * but leaves switched off (its Fourier transform of g(r) ends at r = l/2 and cannot resolve a Bragg peak).  Definition (the
 * build's own), for sample s with N = natoms atoms and the cubic box L = box[s]:
 *   coordinates  u_a = (double)pos[a] / (double)L per component, in float64; the caller need not wrap them;
 *   vectors      every integer triple (h, k, l) with 1 <= n2 = h*h + k*k + l*l <= qmax*qmax  (q = 2 pi (h, k, l) / L);
 *   density mode rho(hkl) = sum_a exp(-2 pi i (h u_ax + k u_ay + l u_az)), the phases h u, k u, l u each reduced in turns (the
 *                nearest integer subtracted, in float64) before any sine or cosine, so that the accuracy depends on neither
 *                qmax nor unwrapped coordinates beyond the bound below;
 *   S(hkl)       = |rho(hkl)|^2 / N in float64; S(-q) = S(q), so one half space is evaluated;
 *   sf_sum[s][n2] the sum of S(hkl) over all vectors of the full shell h*h + k*k + l*l = n2 (twice the half-space sum);
 *   sf_max[s][n2] the maximum of S(hkl) over the shell: N on a Bragg peak of a perfect crystal, O(1) in a liquid;
 *   empty        index 0 and the shells without a vector (n2 = 4^a (8 b + 7)) hold 0 in both.
 * Error bound: every unit-magnitude term carries at most e = (6 pi qmax max|u| + 16) 2^-53 (the rounded products h u; the 16
 * covers the three sines and cosines and the two complex products), so |S - exact| <= 2 N e for every vector.
 * The result is the same bit for bit on every call: float64 accumulators in a fixed order, integer shell sums, no
 * floating-point atomics.
 * pos[ns][natoms][3], box[ns] float32; sf_sum, sf_max [ns][qmax*qmax + 1] float64.  Either output may be NULL (it is then not
 * written), but not both.
 * Returns 0 or a negative NM_ERR_* code; message via nm_distr_last_error(), starting with "nm_distr_sfactor:".  NM_ERR_ARG,
 * checked before the device is looked for and with the outputs left untouched, for: ns < 0, natoms outside 1..4095, qmax
 * outside 1..32, a box that is not finite and positive, a null pos or box, both outputs null, a bad device ordinal.
 * ns == 0 is NM_OK. */
int nm_distr_sfactor(int device, int ns, int natoms, const float *pos, const float *box, int qmax, double *sf_sum, double *sf_max);

#ifdef __cplusplus
}
#endif
#endif
