/*
 * nm_reweight_hist.h — the reweighted histograms of the multistate reweighting.  It is a part of
 * nm_reweight.h, which includes it and whose definitions (samples, states, reduced potential, logd, targets, tf, centring,
 * offsets, error bound) it uses; include that header, not this one.
 *
 * Weights.  For a target (tb, tc): w_n = exp(-u_t(n) - logd[n] + tf), with the logd and the tf of nm_reweight_expect (the same
 *   kernels, the same centring of e and v on their means, the same extended-precision offsets).  They sum to 1.
 * Quantities and bins.  x[q][n], q = 0..nq-1, is any float64 per sample (the energy, the volume, an order parameter);
 *   edges[q][0..nbins] are strictly increasing.  The bin rule is numpy.histogram's: sample n is in bin j of quantity q when
 *   edges[q][j] <= x[q][n] < edges[q][j+1], the last bin is closed on the right (x = edges[q][nbins] is in bin nbins - 1); it is
 *   below when x < edges[q][0] and above when x > edges[q][nbins].
 * Outputs.  hist[t][q][j] = the sum of w_n over the samples in bin j; outside[t][q] = (the sum over the samples below, over those
 *   above).  In exact arithmetic hist[t][q][.] and outside[t][q][.] sum to 1 for every (t, q).
 * Exact bin membership.  The bin is found by float64 comparisons of x with the edges themselves (a bisection), never from a
 *   multiplication: a value that equals an edge lies in the bin that the rule names.
 * Arithmetic.  Every weight is formed in float64 and truncated to a 128-bit fixed-point number with the unit 2^-96; the bins are
 *   summed in 64-bit integers.  A bin is off by at most 2 (the error bound of tf in nm_reweight.h) times its value, from logd and
 *   tf in the exponent, plus nsamples 2^-96 from the truncation, plus one rounding of the result.
 * Determinism.  The same bits on every call: integer sums do not depend on their order; no floating-point atomics.
 * Limits.  nq in 1..8, nbins in 1..1024, nsamples <= 2^28 (the low word of the accumulator: csrc/nm_reweight.h derives it),
 *   ntargets in 1..65536.  Device memory: the 3 nsamples doubles of the other entry points, 2 nq nsamples bytes of bin codes,
 *   nsamples doubles for one quantity while its codes are made, and the counters of one launch of at most 256 targets.
 *
 * Returns 0 or a negative NM_ERR_* code; message via nm_reweight_last_error(), starting with the function's name.  NM_ERR_ARG,
 * checked before the device is looked for and with every output left untouched, for: everything nm_reweight_expect refuses
 * about the states, the samples, the targets and the device ordinal; nq outside 1..8; nbins outside 1..1024; nsamples above
 * 2^28; a null x, edges or hist; a non-finite x or edge; edges that are not strictly increasing.  outside may be NULL.
 */
#ifndef NM_REWEIGHT_HIST_H
#define NM_REWEIGHT_HIST_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* b, c, count, f [nstates] and e, v [nsamples] as for nm_reweight_expect (f as nm_reweight_solve returned it; any f[0]);
 * tb, tc [ntargets]; x [nq][nsamples]; edges [nq][nbins + 1]; hist [ntargets][nq][nbins]; outside [ntargets][nq][2] or NULL. */
int nm_reweight_histogram(int device, int nstates, const double *b, const double *c, const int64_t *count, const double *f,
                          int64_t nsamples, const double *e, const double *v, int ntargets, const double *tb, const double *tc,
                          int nq, const double *x, int nbins, const double *edges, double *hist, double *outside);

#ifdef __cplusplus
}
#endif
#endif
