/*
 * nm_reweight_boot.h — C-ABI of the block-bootstrap replicates of the multistate reweighting (nm_reweight.h; DESIGN.md §9 row
 * f-5): the MBAR solve and the expectations repeated on nrep resampled copies of the sample set in one call, so that every
 * number of nm_reweight.h gets a spread.
 *
 * Replicates.  Replicate r is the problem of nm_reweight.h on the multiset in which sample n occurs mult[r][n] times
 *   (uint16, [nrep][nsamples]; each row sums to nsamples), with the same b, c and count:
 *   logd_r[n] = LSE over the k with count[k] > 0 of (ln count[k] + f_r[k] - u_k(n))
 *   F_r(f)[i] = -LSE over the n with mult[r][n] > 0 of (ln mult[r][n] - u_i(n) - logd_r[n])
 * Iteration.  f_r <- F_r(f_r) - F_r(f_r)[0] from the start f, the base solution (nm_reweight_solve's result on the original
 *   samples), the same for every replicate.  delta[r] = max_i |f_new[i] - f_old[i]|; every replicate stops by its own
 *   delta[r] <= tol or at max_iter.  fr[r], iters[r] and delta[r] are those of the replicate's own last application: a replicate
 *   that has stopped is not moved by the applications made for the others.  fr[r][0] = 0.
 * status[r].  0: converged.  1: max_iter reached, the outputs are the last iterate.  2: a sum over the replicate's samples was
 *   zero or subnormal (or not finite) for some state - no overlap is left after the resampling -; fr[r][*] is NaN, iters[r] and
 *   delta[r] are those of the application that found it.
 * Targets.  The weights of replicate r at (tb, tc) are w_n proportional to mult[r][n] exp(-u_t(n) - logd_r[n]) with logd_r from
 *   the fr passed in (any fr[r][0]); tf, mean, cov and omean as in nm_reweight_expect with these weights, ess = (sum m w)^2 / sum
 *   m w^2 with w the weight of one copy, returned within [1, nsamples].  A replicate whose fr holds a NaN gets NaN in every output.
 * How it is computed (csrc/nm_reweight_boot.h).  f_r = f + d_r: with the base denominators logd, p_k(n) = exp(ln count[k] + f[k] -
 *   u_k(n) - logd[n]) and q_i(n) = exp(f[i] - u_i(n) - logd[n]) depend on the base solution only, ratio_r(n) = sum_k p_k(n)
 *   exp(d_r[k]), S_r[i] = sum_n mult[r][n] q_i(n) / ratio_r(n), d_r[i] <- log S_r[0] - log S_r[i].  In exact arithmetic this is the
 *   iteration above.  The exponentials are formed once per tile of 16 replicates; all terms are non-negative and, for a base f
 *   that is a solution, of order one.  A base f far from a solution may overflow q: such a replicate ends with status 2.
 * Arithmetic.  float64 throughout; e and v centred and the offsets s_k carried in extended precision as in nm_reweight.h; the
 *   same bits on every call: fixed summation order, no floating-point atomics (one integer counter of finished replicates).
 * Error bound, u = 2^-53, U, A, K as in nm_reweight.h (derivation: csrc/nm_reweight_boot.h): one application moves f_r by at
 *   most (K + 45 + N/2^18) u + 2 (2 u A + 3 u U + u max |logd|) off the exact map; tf by the same.
 * Limits: nrep 1..1024; the limits of nm_reweight.h.
 * Device memory: the 3 N doubles of nm_reweight.h, 2 nrep N bytes of multiplicities, 16 N doubles (a tile of replicates), nrep
 *   K doubles twice, and partials: 16 K ceil(N / 4096) doubles (solve), at most 2^24 doubles (expect).  No array of nrep x N doubles.
 *
 * Both functions return 0 or a negative NM_ERR_* code; message via nm_reweight_last_error(), starting with the function's name.
 * NM_ERR_ARG, before the device is looked for and with every output untouched, for: everything nm_reweight_solve or
 * nm_reweight_expect refuses (a non-finite base f included); nrep outside 1..1024; a null mult, fr, iters, delta or status; a
 * replicate whose multiplicities do not sum to nsamples; for nm_reweight_boot_expect a value in fr that is neither finite nor NaN.
 */
#ifndef NM_REWEIGHT_BOOT_H
#define NM_REWEIGHT_BOOT_H
#include "nm_reweight.h"
#ifdef __cplusplus
extern "C" {
#endif

/* b, c, count [nstates]; e, v [nsamples]; f [nstates] the base solution; mult [nrep][nsamples].
 * fr [nrep][nstates]; iters, delta, status [nrep].  NM_OK whenever the arithmetic ran: the caller reads status. */
int nm_reweight_boot_solve(int device, int nstates, const double *b, const double *c, const int64_t *count, int64_t nsamples,
                           const double *e, const double *v, const double *f, int nrep, const uint16_t *mult, double tol,
                           int max_iter, double *fr, int *iters, double *delta, int *status);

/* f [nstates] the base solution (any f[0]), fr [nrep][nstates] the replicates' (as nm_reweight_boot_solve returned them).
 * tb, tc [ntargets]; obs [nobs][nsamples] or NULL with nobs = 0.
 * tf, ess [nrep][ntargets]; mean [nrep][ntargets][2]; cov [nrep][ntargets][3]; omean [nrep][ntargets][nobs] (may be NULL with
 * nobs = 0). */
int nm_reweight_boot_expect(int device, int nstates, const double *b, const double *c, const int64_t *count, const double *f,
                            int64_t nsamples, const double *e, const double *v, int nrep, const uint16_t *mult, const double *fr,
                            int ntargets, const double *tb, const double *tc, int nobs, const double *obs, double *tf, double *ess,
                            double *mean, double *cov, double *omean);

#ifdef __cplusplus
}
#endif
#endif
