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

/* Steinhardt bond-orientational order parameters: per atom q_l, its neighbour-averaged form (Lechner and Dellago) and the
 * global Q_l of a frame, all returned as SQUARES.  Definition (the build's own), for sample s and centre atom c:
 *   entries     exactly the neighbours of nm_distr_angles: (j, a) over the 27 image shifts br[j] (lammps_distr.py:99-102) and all
 *               atoms a, with v = pos[a] - (pos[c] + box*br[j]) in float32, d = float32 sqrt of the sequential float32 sum of the
 *               three squares, and r_lo < (double)d <= r_hi.  r_lo >= 0 excludes the atom itself and coincident atoms; an atom
 *               that qualifies in two images counts as two entries.  Nb(c) is the number of entries;
 *   directions  n = v / |v| in float64 from the float32 components;
 *   moments     q_lm(c) = (1 / Nb(c)) sum over the entries of Y_lm(n), m = -l..l, with the orthonormal spherical harmonics in the
 *               Condon-Shortley phase (Y_l,-m = (-1)^m conj(Y_lm)); q_lm(c) = 0 if Nb(c) = 0;
 *   q2[s][c][i]    = 4 pi / (2l+1) sum_m |q_lm(c)|^2 for l = ls[i]: the square of Steinhardt's q_l, in [0, 1].  Squares, because
 *               where q_l vanishes (l = 2 on any cubic lattice) a 1e-16 error of the square is 1e-8 in the root;
 *   qbar2[s][c][i] the same invariant of qbar_lm(c) = (q_lm(c) + sum over the entries (j, a) of c of q_lm(a)) / (Nb(c) + 1);
 *   Q2[s][i]       the same invariant of (sum_c sum over the entries of c of Y_lm(n)) / (sum_c Nb(c)); 0 if the frame has no bond;
 *   nnb[s][c]      = Nb(c).
 * Error bound, u = 2^-53, M the largest Nb of the call (derivation: csrc/nm_distr.h): per bond the vector (Y_lm)_m is off by at
 * most e(l) = (3 l^2 + 7 l + 8) u of its norm; e_q = e(l) + M u, e_qbar = e_q + (M + 1) u, e_Q = e(l) + (M + 12 + ceil(natoms/32)) u,
 * and each returned square x is off by at most 2 e sqrt(x) + e^2.
 * The result is the same bit for bit on every call: float64 sums in a fixed order, no floating-point atomics.
 * ls[nl]: 1 to 6 strictly increasing values in 1..12.  pos[ns][natoms][3], box[ns] float32; q2, qbar2 [ns][natoms][nl] and
 * Q2[ns][nl] float64, nnb[ns][natoms] int32.  Any output may be NULL (it is then not written), but not all four.
 * Returns 0 or a negative NM_ERR_* code; message via nm_distr_last_error(), starting with "nm_distr_bondorder:".  NM_ERR_ARG,
 * checked before the device is looked for and with the outputs left untouched, for: ns < 0, natoms outside 1..4095, nl outside
 * 1..6, ls not strictly increasing within 1..12, not 0 <= r_lo < r_hi, r_hi > min(box)/2 over the batch, a box that is not finite
 * and positive, a null pos, box or ls, all outputs null, a bad device ordinal.  ns == 0 is NM_OK where a device is found (the
 * device is looked for first, as in nm_distr_sfactor: NM_ERR_HIP without one). */
int nm_distr_bondorder(int device, int ns, int natoms, const float *pos, const float *box, double r_lo, double r_hi, int nl,
                       const int *ls, double *q2, double *qbar2, double *Q2, int32_t *nnb);

/* Steinhardt's third-order invariants: per atom w_l, its neighbour-averaged form and the global W_l of a frame, all returned as the
 * UNNORMALISED cubic forms, beside the squares of nm_distr_bondorder.  Definition (the build's own), for sample s and centre atom c:
 *   entries, directions, moments   q_lm(c), qbar_lm(c) and the frame's Q_lm exactly those of nm_distr_bondorder;
 *   T_l(a)      for a vector a_m, m = -l..l, with a_-m = (-1)^m conj(a_m):
 *               T_l(a) = (4 pi / (2l+1))^(3/2) Re sum_{m1+m2+m3=0} (l l l; m1 m2 m3) a_m1 a_m2 a_m3, with Wigner's 3j symbol; the sum is real
 *               in exact arithmetic, so only the real part is formed;
 *   w3[s][c][i]    = T_l(q_lm(c)) for l = ls[i];   wbar3[s][c][i] = T_l(qbar_lm(c));   W3[s][i] = T_l(Q_lm); each 0 where the vector is 0;
 *   q2, qbar2, Q2, nnb   as in nm_distr_bondorder, and bit for bit what that function returns for the same arguments.
 * Steinhardt's w_l (hat) = w3 / q2^(3/2) lies in [-1, 1]: sum_{m1,m2} (3j)^2 = 1, so by Cauchy-Schwarz |T_l(a)| <= (4 pi / (2l+1) sum |a_m|^2)^(3/2).
 * The ratio is left to the caller, for the reason the squares are returned: it is ill-conditioned wherever q_l vanishes (l = 2 on a
 * cubic lattice, l = 4 on the icosahedron), while w3 itself is a polynomial in the moments with an absolute error bound.
 * Even l only: for odd 3l the symbol changes its sign under the exchange of two columns, so T_l vanishes identically.
 * Error bound, u = 2^-53 (derivation: csrc/nm_distr_w.h): with x the matching square (q2, qbar2, Q2), e the matching e_q, e_qbar, e_Q of
 * nm_distr_bondorder and n_l the number of symbols that do not vanish (19, 61, 127, 205, 331, 469 for l = 2, 4, .., 12), each returned
 * cubic form is off by at most 3 e x + 3 e^2 sqrt(x) + e^3 + (n_l + 12) u (sqrt(x) + e)^3: below 5e-13 up to M = 529 neighbours.
 * The result is the same bit for bit on every call: the terms in a fixed order (m1 ascending, then m2, 64 at a time through a fixed
 * tree), float64 sums in a fixed order, no floating-point atomics.
 * ls[nl]: 1 to 6 strictly increasing EVEN values in 2..12.  pos[ns][natoms][3], box[ns] float32; w3, wbar3, q2, qbar2 [ns][natoms][nl]
 * and W3, Q2 [ns][nl] float64, nnb[ns][natoms] int32.  Any output may be NULL (it is then not written), but not all seven.
 * Returns 0 or a negative NM_ERR_* code; message via nm_distr_last_error(), starting with "nm_distr_bondorder_w:".  NM_ERR_ARG, checked
 * before the device is looked for and with the outputs left untouched, for everything nm_distr_bondorder refuses, in its order, and
 * for an odd l (the message says why).  ns == 0 as in nm_distr_bondorder. */
int nm_distr_bondorder_w(int device, int ns, int natoms, const float *pos, const float *box, double r_lo, double r_hi,
                         int nl, const int *ls, double *w3, double *wbar3, double *W3,
                         double *q2, double *qbar2, double *Q2, int32_t *nnb);

/* Solid-like atoms and crystal clusters: ten Wolde, Ruiz-Montero and Frenkel's criterion on the normalised dot products of the
 * q_lm vectors of neighbouring atoms, and the connected components of the solid-like atoms.  Definition (the build's own), for
 * sample s, one l and centre atom c:
 *   entries     exactly those of nm_distr_bondorder: (j, a) over the 27 image shifts br[j] and all atoms a, the float32
 *               displacement and its float32 length d, r_lo < (double)d <= r_hi; an atom that qualifies in two images is two
 *               entries;
 *   moments     q_lm(c) exactly those of nm_distr_bondorder: float64, m >= 0 stored, 0 if c has no entry;
 *   norm        |q(c)|^2 = |q_l0|^2 + 2 sum_{m>0} |q_lm|^2;
 *   bond value  for the entry (j, a) of c: s(c, a) = (Re q_l0(c) conj q_l0(a) + 2 sum_{m>0} Re q_lm(c) conj q_lm(a)) / (|q(c)| |q(a)|)
 *               in float64, the sums with m ascending; s = 0 where the product of the norms is exactly 0;
 *   connection  the entry is connected iff s(c, a) > s_min;
 *   nconn[s][c] the number of connected entries of c;
 *   solid-like  nconn[s][c] >= n_min;
 *   clusters    the connected components of the undirected graph on the solid-like atoms that has the edge {c, a} whenever a is an
 *               entry of c or c is an entry of a.  The edge does not ask for a connection (the usual convention).  The float32 test
 *               is not guaranteed to be symmetric on the cutoff itself, hence the "or";
 *   label[s][c] the smallest atom index in c's cluster, -1 for an atom that is not solid-like: canonical, independent of the
 *               order of execution;
 *   nsolid[s]   the number of solid-like atoms, nclus[s] the number of clusters, largest[s] the size of the largest cluster (0 if
 *               there is none).
 * The bond value carries the error of the moments (nm_distr_bondorder: e_q per vector, relative to the harmonics' norm), so an
 * entry whose value lies within about 4 (e_q / |q(c)| + e_q / |q(a)|) + 16 u of s_min can fall on either side; everything else is
 * integer and exact.  The result is the same bit for bit on every call: fixed summation orders, integer atomics only.
 * pos[ns][natoms][3], box[ns] float32; nconn, label [ns][natoms] and nsolid, nclus, largest [ns] int32.  Any output may be NULL (it
 * is then not written), but not all five.
 * Returns 0 or a negative NM_ERR_* code; message via nm_distr_last_error(), starting with "nm_distr_solid:".  NM_ERR_ARG, checked
 * before the device is looked for and with the outputs left untouched, for: ns < 0, natoms outside 1..4095, l outside 1..12, s_min
 * not within [-1, 1), n_min < 1, not 0 <= r_lo < r_hi, r_hi > min(box)/2 over the batch, a box that is not finite and positive, a
 * null pos or box, all outputs null, a bad device ordinal.  ns == 0 as in nm_distr_bondorder. */
int nm_distr_solid(int device, int ns, int natoms, const float *pos, const float *box, double r_lo, double r_hi, int l, double s_min,
                   int n_min, int32_t *nconn, int32_t *label, int32_t *nsolid, int32_t *nclus, int32_t *largest);

/* Common neighbour analysis (Honeycutt and Andersen; Faken and Jonsson; the adaptive form of Stukowski, Modelling Simul. Mater. Sci.
 * Eng. 20 (2012) 045021): the structure type of every atom (fcc, hcp, bcc, icosahedral, other) from the bonds among its own
 * neighbours, in integers.  Definition (the build's own), for sample s and centre atom c:
 *   entries     exactly those of nm_distr_bondorder: (j, a) over the 27 image shifts br[j] and all atoms a, the float32 displacement v
 *               and its float32 length d (sequential sum, correctly rounded root, no contraction), r_lo < (double)d <= r_hi; an atom
 *               that qualifies in two images is two entries.  Scan order: image-major, then atom index;
 *   graph       on a set of entries (the vertices) with a local cutoff rc: the entries k and m are bonded iff the float32 difference
 *               w = v_m - v_k (componentwise) has a float32 length dw (the arithmetic of d) with r_lo < (double)dw <= rc.  The graph
 *               is local to the centre, bonds among the centre's own neighbour vectors (as OVITO defines them), not a lookup in the
 *               other atoms' entries: it needs no image bookkeeping, and an atom present in two images is two vertices;
 *   signature   of the entry k, the triple (ncn, nb, nlc): ncn the number of vertices bonded to k (the common neighbours of c and k),
 *               nb the number of bonds among those, nlc the largest number of bonds that one connected component of those bonds
 *               holds.  That is OVITO's definition.  It equals the "longest chain" of bonds of the original method wherever the
 *               largest component is a path or a ring, which it is for every signature of the columns below as the fcc, hcp, bcc and
 *               icosahedral environments produce them; no longest path is searched, and a star of three bonds has nlc = 3;
 *   columns     8, in this order: (4,2,1) (4,2,2) (4,4,4) (6,6,6) (5,5,5) (5,4,4) (4,3,3) and `other`;
 *   types       0 other, 1 fcc, 2 hcp, 3 bcc, 4 ico.  From the column counts n of a graph of Nv vertices:
 *               fcc if Nv = 12 and n421 = 12; hcp if Nv = 12, n421 = 6 and n422 = 6; ico if Nv = 12 and n555 = 12;
 *               bcc if Nv = 14, n444 = 6 and n666 = 8; else other;
 *   mode NM_CNA_FIXED     the vertices are all Nb entries of c and rc = r_hi: the conventional analysis, whose column sums are the
 *               Honeycutt-Andersen pair statistics of a liquid.  sig[s][c] = the column counts (they add up to Nb) and the type as
 *               above with Nv = Nb.  If Nb > 32: type other, and all Nb entries are counted in the column `other`;
 *   mode NM_CNA_ADAPTIVE  r_hi is only the search radius.  The entries are sorted by (d as float32, scan order).  With fewer than 12
 *               entries: type other, sig[s][c] all zero.  Otherwise the first 12 are the vertices, with
 *                 rc12 = 1.2071067811865475 * (d_0 + ... + d_11) / 12.0          ((1 + sqrt 2) / 2 times the mean)
 *               in float64: the d converted from float32 and added in sorted order, then the product, then the quotient, one rounding
 *               per operation, no contraction; fcc, hcp or ico as above.  If none of them holds and there are at least 14 entries,
 *               the first 14 are the vertices, with
 *                 rc14 = 1.2071067811865475 * S / 14.0,   S = sum_{k<8} (d_k * 1.1547005383792517) + sum_{8<=k<14} d_k
 *               (2 / sqrt 3 scales the first bcc shell onto the second; each product rounded, all terms added in that order); bcc
 *               if n444 = 6 and n666 = 8.  sig[s][c] = the column counts of the graph that decided the type, for type other those
 *               of the 12-vertex graph;
 *   per sample  ntype[s][t] the number of atoms of type t, nsig[s][k] the sum of sig[s][c][k] over the atoms (below 2^31 for every
 *               accepted call).
 * Everything returned is an integer, and every comparison is the stated float32 or float64 one: the result is the same bit for bit
 * on every call (integer atomics only) and equals a restatement of the text above exactly.
 * pos[ns][natoms][3], box[ns] float32; type[ns][natoms], sig[ns][natoms][8], ntype[ns][5], nsig[ns][8] int32.  Any output may be NULL
 * (it is then not written), but not all four.
 * Returns 0 or a negative NM_ERR_* code; message via nm_distr_last_error(), starting with "nm_distr_cna:".  NM_ERR_ARG, checked before
 * the device is looked for and with the outputs left untouched, for: ns < 0, natoms outside 1..4095, mode neither of the two, not
 * 0 <= r_lo < r_hi, r_hi > min(box)/2 over the batch, a box that is not finite and positive, a null pos or box, all outputs null, a
 * working set beyond the LDS, a bad device ordinal.  ns == 0 as in nm_distr_bondorder. */
#define NM_CNA_FIXED 0
#define NM_CNA_ADAPTIVE 1
int nm_distr_cna(int device, int ns, int natoms, const float *pos, const float *box, double r_lo, double r_hi, int mode,
                 int32_t *type, int32_t *sig, int32_t *ntype, int32_t *nsig);

/* Pair entropy per atom: Piaggi and Parrinello's local-entropy fingerprint (J. Chem. Phys. 147, 114112 (2017); Phys. Rev. Lett. 119,
 * 015701 (2017)), the projection of the two-body excess entropy -2 pi rho int (g ln g - g + 1) r^2 dr on each atom, in units of k_B, and
 * its average over the neighbours.  The papers define the quantity; the discretisation is the build's own.  For sample s and centre c:
 *   entries     exactly those of nm_distr_bondorder with r_lo = 0 and r_hi = r_m: (j, a) over the 27 image shifts br[j] and all atoms a,
 *               the float32 displacement and its float32 length d, 0 < (double)d <= r_m; an atom that qualifies in two images is two
 *               entries.  nnb[s][c] is their number;
 *   density     rho = natoms / L^3 with L = (double)box[s];
 *   grid        D = r_m / nbins and r_k = k * D for k = 0..nbins, each the float64 result of that one operation;
 *   smeared radial density   h_k = (1 / (4 pi rho sigma sqrt(2 pi))) * sum over the entries of exp(-(r_k - d)^2 / (2 sigma^2)), which
 *               is r_k^2 g_m(r_k) of the papers.  A term whose computed exponent is below -50 is left out;
 *   integrand   I_0 = 0; for k >= 1, I_k = r_k^2 where h_k == 0, otherwise I_k = h_k ln(h_k / r_k^2) - h_k + r_k^2;
 *   s[s][c]     = -2 pi rho D (I_0 / 2 + I_1 + ... + I_(nbins-1) + I_nbins / 2), the trapezoid rule.  An atom without entries has
 *               exactly -2 pi rho D (r_1^2 + ... + r_(nbins-1)^2 + r_nbins^2 / 2) up to the rounding of that sum;
 *   sbar[s][c]  = (s(c) + sum over the entries (j, a) of c with (double)d <= r_avg of s(a)) / (1 + their number): the plain-cutoff
 *               neighbour average, the shape of qbar_lm of nm_distr_bondorder.  r_avg is independent of r_m;
 *   smean[s], sbarmean[s]   the means of s and sbar over the atoms of the sample;
 *   nlow[s]     the number of atoms with sbar < s_cut (s_cut may be infinite; -infinity counts none).
 * Error bound, u = 2^-53, E = 50 the largest |exponent| kept, M the largest nnb of the call, M_a the largest number of entries within
 * r_avg (derivation: csrc/nm_distr.h).  With A(c) = 2 pi rho D sum' (h_k |ln(h_k / r_k^2)| + h_k + r_k^2) >= |s(c)|, sum' the
 * trapezoid sum over k >= 1:
 *   |s - exact| <= e_s = (7 E + M + nbins + 30) u A + omitted,
 *   omitted = 2 pi rho D sum' om (1 + |ln(om / r_k^2)| + |ln(h_k / r_k^2)|), om = M exp(-E) (1 + 1e-12) / (4 pi rho sigma sqrt(2 pi)),
 *   the last logarithm only where h_k > 0 (the allowance for the terms left out: about 1e-19 A);
 *   |sbar - exact| <= max e_s + (M_a + 2) u max |s|,   |smean - exact| <= max e_s + (natoms + 1) u max |s|,
 *   |sbarmean - exact| <= max e_s + (M_a + natoms + 3) u max |s|, the maxima over the atoms of the sample.
 * For M <= 2200 and nbins <= 1024 that is below 4e-13 A.  nlow is exact unless an sbar lies within its bound of s_cut.
 * The result is the same bit for bit on every call: float64 sums in a fixed order, no atomics.
 * pos[ns][natoms][3], box[ns] float32; s, sbar [ns][natoms] and smean, sbarmean [ns] float64; nnb [ns][natoms] and nlow [ns] int32.
 * Any output may be NULL (it is then not written), but not all six.
 * Returns 0 or a negative NM_ERR_* code; message via nm_distr_last_error(), starting with "nm_distr_entropy:".  NM_ERR_ARG, checked
 * before the device is looked for and with the outputs left untouched, for: ns < 0, natoms outside 1..4095, nbins outside 1..1024,
 * sigma or r_m not positive and finite, r_m or r_avg above min(box)/2 over the batch, r_avg <= 0, s_cut NaN, a box that is not finite
 * and positive, a null pos or box, all outputs null, a bad device ordinal.  ns == 0 as in nm_distr_bondorder. */
int nm_distr_entropy(int device, int ns, int natoms, const float *pos, const float *box, double r_m, double sigma, int nbins,
                     double r_avg, double s_cut, double *s, double *sbar, int32_t *nnb, double *smean, double *sbarmean,
                     int32_t *nlow);

/* nm_cluster_spectral — the spectral embedding of a set of points for the cluster stage: the leading
 * eigenvectors of the normalised affinity of a Gaussian kernel, which nm_cluster_kmeans then clusters (lammps_vae.py -cl spectral).
 * It is declared and built here for the reason nm_cluster_kmeans is.  The definitions are the build's own; off ties they are
 * sklearn.cluster.SpectralClustering(n_clusters=K, affinity='rbf', gamma=gamma, assign_labels='kmeans'), that is
 * sklearn.manifold.spectral_embedding(norm_laplacian=True, drop_first=False) followed by k-means.  No random number is drawn in the
 * library: the start block is the caller's.  u = 2^-53, N = npoints.
 *
 * Points.  x[n][c], float64, row-major, in host memory.  d2(i, j) is include/nm_cluster.h's: d = x[i][c] - x[j][c], c ascending, the
 *   first square a plain product, every further one a fused multiply-add; d2(i, j) == d2(j, i) bit for bit, error at most
 *   (ndim + 2) u d2.
 * Affinity.  A(i, j) = exp(-(gamma d2(i, j))) for j != i and A(i, i) = 0: float64, the product rounded once, exp the device
 *   library's double exp (1 ulp).  A is symmetric bit for bit.  It is never stored: every use of it is one pass over all pairs.
 * Degree.  deg[i] = sum_j A(i, j), in the order given under Determinism.
 * Operator.  M = D^-1/2 A D^-1/2, D = diag(deg), D^-1/2 computed as 1 / sqrt(deg[i]), two roundings.  M is symmetric, its spectrum
 *   lies in [-1, 1] and its largest eigenvalue is 1 (eigenvector D^1/2 1).
 * Wanted.  The ncomp largest eigenvalues of M, descending, with orthonormal eigenvectors v_c.
 * Embedding.  embed[i][c] = v_c[i] / sqrt(deg[i]).  The sign of column c is fixed so that its entry of largest magnitude, the first
 *   index on equal magnitudes, is positive: sklearn's deterministic sign flip.
 * Degenerate eigenvalues.  Inside the eigenspace of a multiple eigenvalue (or of eigenvalues closer than the residuals) the basis
 *   is whatever the iteration gives; only the space is defined.  Compare spaces, not vectors.
 *
 * Method: Chebyshev-filtered subspace iteration on a block V of nblock >= ncomp orthonormal columns, V_0 = the orthonormalised init.
 *   1. The Rayleigh-Ritz pass.  W = M V (one pass over all pairs), H = V^T W; the host solves the nblock x nblock symmetric
 *      eigenproblem of (H + H^T) / 2 by cyclic Jacobi, theta descending; V and W are rotated onto the Ritz vectors, and
 *      resid[c] = ||W_c - theta_c V_c||_2, formed element by element on the device and then summed: a residual, not a difference
 *      of norms.  eigval = theta.  passes += 1.
 *   2. Stop with status 0 where max_{c < ncomp} resid[c] <= tol; else with status 2 where passes + degree > max_pass (the next
 *      round would pass it).  Either way the outputs are the Ritz pairs of step 1 and their residuals.
 *   3. The filter of degree `degree`: Zhou and Saad's scaled Chebyshev recurrence for the polynomial that is 1 at 1 and
 *      equi-oscillates on the damped interval [-1, low], e = (low + 1) / 2, c = (low - 1) / 2, sigma_1 = e / (1 - c):
 *        Y_1 = (sigma_1 / e) (W - c V);   Y_k = 2 (sigma_k / e) (M Y_{k-1} - c Y_{k-1}) - sigma_{k-1} sigma_k Y_{k-2},
 *        sigma_k = 1 / (2 / sigma_1 - sigma_{k-1}),  Y_0 = V.
 *      Y_1 needs no pass (W is at hand), so a round costs degree passes: degree - 1 here and one in step 1.  low is the smallest
 *      Ritz value of step 1, not below -1 + 2^-10.  Where nblock == ncomp the block's last column is itself wanted and must stay
 *      outside the damped interval, so low stays what the first round made it; such a block converges at the rate of its gap alone,
 *      and nblock > ncomp is the intended use.
 *   4. V = the columns of Y_degree made orthonormal through their Gram matrix (Cholesky QR, applied twice); back to 1.
 *   The small matrices are solved on the host in float64; everything of length N runs on the device.
 * Determinism.  The same bytes on every call and on every device.  Every sum runs in an order fixed by the indices alone: a row's
 *   sum over j is cut into S = S(N) slices, slice s holding the columns of the tiles s, s + S, ... of 128 consecutive points, added
 *   in ascending j from +0 by one fused multiply-add each, and the slices are added in ascending s; a sum over the points (H, the
 *   Gram matrices, the residuals) is cut into chunks of 4096 points, in a chunk lane p of 64 adds the points p, p + 64, ... in
 *   ascending order, the lanes are added as a binary tree and the chunks in ascending order.  No floating-point atomic.
 * Memory.  O(N (ndim + 3 W)) on the device, W = nblock padded to 1, 8 or 16, plus the slices' partial sums, S N W doubles with
 *   S N <= about 2^20 below 2^19 points and S <= 8 above: at most 1 GiB.  No N x N array exists.  The work is N^2 affinities per pass.
 * Bounds.  Write t_ij = gamma d2(i, j).  The computed argument of exp is within (ndim + 3) u t_ij of t_ij, so the computed
 *   A(i, j) is within ((ndim + 3) t_ij + 2) u of itself; a row adds at most N + S positive terms one after the other.  So
 *     |deg[i] - exact| <= u ((ndim + 3) sum_j t_ij A(i, j) + (2 N + 2) deg[i])  <=  u ((ndim + 3) T + 2 N + 2) deg[i],
 *   T = gamma times the largest d2 of any pair.  One application of M to a vector v of unit 2-norm: a term
 *   deg[i]^-1/2 A(i, j) deg[j]^-1/2 v[j] carries the two degrees' errors halved and two roundings each for the root and the
 *   quotient, one for each of the three products, the affinity's and the row's adding; M has no negative entry and 2-norm 1, so
 *     ||computed M v - M v||_2 <= eps_M = (2 (ndim + 3) T + 4 N + 16) u.
 *   The rotation onto the Ritz vectors mixes nblock such columns, so with v_c = embed[.][c] sqrt(deg[.])
 *     |resid[c] - ||M v_c - eigval[c] v_c||_2| <= eps_R = sqrt(nblock) eps_M + 160 u,
 *   and M has an eigenvalue within resid[c] + 2 eps_R of eigval[c].  The v_c are orthonormal to 64 nblock u.
 *
 * x [npoints][ndim]; init [npoints][nblock]; embed [npoints][ncomp]; eigval, resid [nblock], every Ritz pair of the block, descending;
 * deg [npoints]; info [2]: the passes done, and the status, 0 within tol, 2 stopped at max_pass.
 * Returns 0 or a negative NM_ERR_* code; message via nm_distr_last_error(), starting with "nm_cluster_spectral:".  NM_ERR_ARG, checked
 * before the device is looked for and with every output left untouched, for, in this order: npoints outside 2..2^20, ndim outside
 * 1..16, a gamma that is not finite or not positive, ncomp outside 1..8 or above npoints, nblock outside ncomp..16 or above npoints,
 * degree outside 1..64, max_pass outside 1..100000, a tol that is not finite or is negative, a pointer that is null, a value of init
 * that is not finite (the message names the row and the column), a negative device ordinal.  Found on the device, NM_ERR_ARG as
 * well and the outputs untouched: a value of x that is not finite (a first screen; the message names the first such point); a point
 * of degree 0, which no other point reaches (the message names the first and says that gamma is too large for it); a start block
 * whose columns are dependent to working precision (a pivot of the first Cholesky factor not above 256 u of its diagonal element).
 * NM_ERR_STATE, outputs untouched, if a later Cholesky factor fails that way.  NM_ERR_HIP without a device or when a HIP call fails. */
int nm_cluster_spectral(int device, int64_t npoints, int ndim, const double *x, double gamma, int ncomp, int nblock,
                        const double *init, int degree, int max_pass, double tol, double *embed, double *eigval,
                        double *resid, double *deg, int32_t *info);

/* Where the device time of the calling thread's last successful nm_cluster_spectral went, in milliseconds between device events:
 * ms[0] the upload and the screen, ms[1] the degree pass, ms[2] the operator passes with the joining of their slices, ms[3] the
 * block reductions and applies, ms[4] the host's small matrices including their transfers.  Slots of its own. */
int nm_cluster_spectral_last_timing(double *ms);

/* nm_cluster_kmeans —k-means for the cluster stage: Lloyd's iteration of a set of points from given
 * initial centres, nrestarts independent runs in one call, the reference's other practical clustering (lammps_vae.py -cl kmeans,
 * -nc the number of clusters).  It is declared and built here, beside nm_distr_lof and with this header's error channel, because
 * the tests pin include/nm_cluster.h at its three DBSCAN symbols; the kernels share DBSCAN's distance (csrc/nm_cluster.h, cl_d2).
 * The definitions are the build's own; off ties, and while no cluster runs empty, restart r gives the labels of
 * sklearn.cluster.KMeans(n_clusters=k, init=init[r], n_init=1, algorithm='lloyd', max_iter=max_iter), and `tol` is sklearn's tol
 * already multiplied by the mean variance of the coordinates.  No random number is drawn in the library.  u = 2^-53.
 *
 * Points.  x[n][c], n = 0..npoints-1 points of c = 0..ndim-1 coordinates, float64, row-major, in host memory.
 * Distance.  d2(i, j) of point i and centre j is include/nm_cluster.h's, the point first and the centre second:
 *   d = x[i][c] - C[j][c], c ascending, the first square a plain product, every further one a fused multiply-add.  One device
 *   function for every pass: the same point and centre give the same bits everywhere.  Error at most (ndim + 2) u d2.
 * Assignment.  The label of i is the j with the smallest d2(i, j); on equal bits the smallest j.
 * Update.  Centre j becomes, coordinate by coordinate, the sum of its members divided by their number, one IEEE division rounded
 *   once.  The order of the sum is a function of the indices alone: the points are cut into chunks of 4096 and a chunk into 64
 *   pieces of 64 consecutive points; a piece's members are added in ascending index, starting from +0; the 64 pieces of a chunk are
 *   added as a binary tree (piece 2 p with piece 2 p + 1, level by level; a piece without members is +0); the chunks are added in
 *   ascending order.  A cluster without members keeps its centre and has count 0: sklearn relocates such a centre to the point
 *   farthest from its own, this library does not, and a restart in which that happens is no longer sklearn's.
 * Step t = 1, 2, ... of one restart, C_1 = init[r]:
 *   1. L_t is the assignment against C_t.
 *   2. If t > 1 and L_t == L_{t-1}: the fixed point.  status 0, iters = t - 1, the centres are C_t and the labels L_t.
 *   3. Else C_{t+1} is the update of L_t, and shift = sum_j sum_c (C_{t+1}[j][c] - C_t[j][c])^2, every square rounded once and then
 *      added, j then c ascending.
 *   4. If shift <= tol: status 1, iters = t.
 *   5. Else if t == max_iter: status 2, iters = t.
 *   6. With status 1 or 2 one more assignment, against C_{t+1}, is the result: the returned labels are always the assignment
 *      against the returned centres.
 * Inertia.  inertia[r] = the sum over i of d2(i, centre of label[i]) for the returned labels and centres of restart r, in the order
 *   of the update's sum (pieces ascending, tree, chunks ascending), every term rounded as d2 leaves it and then added.
 * Best restart.  best = the restart with the smallest inertia, the lowest index on equal bits; label, centre and count (the members
 *   of the returned labels) are that restart's, and cluster j is the one that began at init[best][j].
 * Independence.  What restart r returns is a function of x, init[r], max_iter and tol alone, not of the other restarts or of when
 *   they finish: a finished restart is frozen.
 * Determinism.  The same bytes on every call and on every device, whatever the schedule: fixed orders and one integer atomic (an
 *   OR), no floating-point atomic.
 * Memory.  O(npoints (ndim + nrestarts)) on the device: x, one byte per point and restart, and per chunk the sums of all
 *   k * nrestarts <= 4096 clusters.  No npoints x k array of distances exists.
 *
 * Returns 0 or a negative NM_ERR_* code; message via nm_distr_last_error(), starting with "nm_cluster_kmeans:".  NM_ERR_ARG, checked
 * before the device is looked for and with every output left untouched, for, in this order: npoints outside 1..2^21, ndim outside
 * 1..16, k outside 1..256 or k > npoints, nrestarts outside 1..64 or k * nrestarts > 4096, max_iter outside 1..10000, a tol that is
 * not finite or is negative, a pointer that is null, a value of init that is not finite (the message names the restart and the
 * centre), a negative device ordinal.  A value of x that is not finite is found on the device by a first screen: NM_ERR_ARG, the
 * message names the first such point, the outputs are left untouched.  NM_ERR_HIP without a device or when a HIP call fails.
 *
 * x [npoints][ndim]; init [nrestarts][k][ndim]; label [npoints]; centre [k][ndim]; count [k];
 * inertia, iters, status [nrestarts]; best [1]. */
int nm_cluster_kmeans(int device, int64_t npoints, int ndim, const double *x, int k, int nrestarts, const double *init,
                      int max_iter, double tol, int32_t *label, double *centre, int32_t *count,
                      double *inertia, int32_t *iters, int32_t *status, int32_t *best);

/* Where the device time of the calling thread's last successful nm_cluster_kmeans went, in milliseconds between device events:
 * ms[0] the upload and the screen, ms[1] the assignment passes and the inertia pass, ms[2] the update passes and the host's looks at
 * the restarts' states.  Slots of its own: nm_distr_last_timing and nm_cluster_last_timing are left alone by a k-means call. */
int nm_cluster_kmeans_last_timing(double *ms);

/* nm_distr_lof — the local outlier factor of many small sets of points at once: not a histogram of frames
 * but the distribution of a grid point's samples among themselves.  The reference's inlier selection (lammps_vae.py -ad) fits
 * sklearn.neighbors.LocalOutlierFactor(contamination='auto'), 20 neighbours, to the samples of every (P, T) grid point alone.  The
 * definitions below are the build's own; off ties they are sklearn's LocalOutlierFactor(n_neighbors=k, algorithm='brute') applied to
 * each set alone.  Every array is float64 (nbr int32) in host memory; calls are stateless.  u = 2^-53.
 *
 * Points.  x[s][i][c], s = 0..nsets-1 sets of i = 0..npts-1 points of c = 0..ndim-1 coordinates, row-major.  i, j and every stored
 *   index count within a set; no quantity of a set depends on another set.
 * Distance.  d2(i, j) = sum_c (x[s][i][c] - x[s][j][c])^2 in float64, c ascending, every difference, product and sum rounded on its
 *   own (no fused multiply-add), as in include/nm_tsne.h: the same bits wherever a pair is formed and d2(i, j) == d2(j, i).  Error
 *   at most (ndim + 2) u d2.
 * Neighbours.  nbr[s][i][0..k-1] are the k points j != i of set s with the smallest (d2(i, j), j) in lexicographic order, stored in
 *   that order: duplicates and ties are decided by the index.  The selection is exact (one pass over the set's pairs that keeps the
 *   k best of each point, then their ranks).
 * kdist.  kdist[i] = sqrt(d2(i, nbr[i][k-1])).
 * reach.  reach(i, m) = max(sqrt(d2(i, nbr[i][m])), kdist[nbr[i][m]]).
 * lrd.  lrd[i] = 1 / ((sum_m reach(i, m)) / k + 1e-10), the sum over m ascending from 0.  The 1e-10 is sklearn's and is absolute:
 *   it bounds lrd by 1e10 and is felt wherever the mean reach is not far above it, so the caller's scale matters (the outlier stage
 *   hands over pca's projections as they are, as the reference does).
 * lof.  lof[i] = (sum_m lrd[nbr[i][m]] / lrd[i]) / k, the sum over m ascending, one division per term.  sklearn's
 *   negative_outlier_factor_ is -lof, and its 'auto' rule calls i an outlier iff lof[i] > 1.5.
 * Degenerate input is defined, no error: a set whose points all coincide gives kdist = 0, lrd = 1e10, lof = 1.
 * Determinism.  Every sum runs in the fixed order above; there are no floating-point atomics and no atomics at all.  Every output
 *   is the same bytes on every call, and a set's outputs do not depend on which other sets are in the batch.
 * Bounds, with the lists given (csrc/nm_lof.h derives them): kdist to (ndim / 2 + 3) u, lrd to (ndim / 2 + k + 8) u, lof to
 *   (ndim + 3 k + 16) u of itself.
 * Memory.  O(nsets npts (ndim + k)) on the device; no npts x npts array exists at any time.  The work is npts^2 distances per set,
 *   each pair read once.
 *
 * x [nsets][npts][ndim]; lof, lrd, kdist [nsets][npts]; nbr [nsets][npts][k] (int32, indices within the set) or null.
 * Returns 0 or a negative NM_ERR_* code; message via nm_distr_last_error(), starting with "nm_distr_lof:".  NM_ERR_ARG, checked
 * before the device is looked for and with every output left untouched, for, in this order: nsets outside 1..2^20, npts outside
 * 2..4096, nsets npts above 2^21, ndim outside 1..16, k outside 1..min(npts - 1, 64), a null pointer other than nbr, a negative
 * device ordinal.  A value of x that is not finite is found on the device by a first screen, as include/nm_cluster.h's is:
 * NM_ERR_ARG, the message names the set and the first such point, the outputs are left untouched. */
int nm_distr_lof(int device, int64_t nsets, int npts, int ndim, const double *x, int k, double *lof, double *lrd, double *kdist,
                 int32_t *nbr);

/* Where the device time of the calling thread's last successful nm_distr_lof went, in milliseconds between device events: ms[0] the
 * upload of x and the screen, ms[1] the neighbour pass, ms[2] the lrd pass, ms[3] the lof pass.  The downloads of the results are
 * not in it.  NM_ERR_ARG for a null pointer. */
int nm_distr_last_timing(double *ms);

#ifdef __cplusplus
}
#endif
#endif
