/*
 * nm_reweight.h — C-ABI of the multistate reweighting of the replica grid: MBAR (Shirts and Chodera,
 * J. Chem. Phys. 129, 124105, 2008) over the P x T states of a replica-exchange run.  The reference has no such step (it
 * locates the transition with a VAE on the histograms, lammps_vae.py); the definitions below are the build's own.
 *
 * Samples and states.  Samples n = 0..N-1 carry the energy e[n] and the volume v[n] (float64).  States k = 0..K-1 carry
 *   b[k] = 1 / thermal energy and c[k] = the Metropolis prefactor of the volume (1/et and pf of init_constant,
 *   remcmc:114-132).  count[k] >= 0 samples were drawn at state k; the counts sum to N.  Which sample came from which state
 *   is not needed.
 * Reduced potential.  u_k(n) = b[k] e[n] + c[k] v[n].  (The volume move's (natoms + 1) ln V weight is the same in every
 *   state and cancels.)
 * Map.  LSE = log-sum-exp, evaluated with the maximum taken out, so that no term overflows:
 *   logd[n] = LSE over the k with count[k] > 0 of (ln count[k] + f[k] - u_k(n))
 *   F(f)[i] = -LSE over n of (-u_i(n) - logd[n])                       for every state i, sampled or not
 * Iteration.  f <- F(f) - F(f)[0]; delta = max_i |f_new[i] - f_old[i]|; it stops when delta <= tol or after max_iter
 *   applications.  F(f + const) - F(f + const)[0] does not depend on the constant, so neither does the result on f[0] of the start.
 * Targets.  A target is any (tb, tc), sampled or not: u_t(n) = tb e[n] + tc v[n],
 *   tf   = -LSE_n(-u_t(n) - logd[n]),  the weights w_n = exp(-u_t(n) - logd[n] + tf) sum to 1,
 *   ess  = 1 / sum_n w_n^2 (Kish), which lies in [1, N] and is returned within it,
 *   mean = (<e>, <v>),  cov = (var_e, cov_ev, var_v) about those means,  omean[j] = <obs[j]>,  <A> = sum_n w_n A[n].
 * Arithmetic.  float64 throughout.  e and v are centred on their sample means before anything is multiplied (u_k(n) =
 *   b[k] (e[n] - e0) + c[k] (v[n] - v0) + s_k with s_k = b[k] e0 + c[k] v0 carried in extended precision on the host), so a
 *   large common offset of e or v costs the central moments nothing and costs f, tf and logd only the rounding of their own
 *   values.  States or targets without any overlap give finite results: a term that underflows is 0, the largest is 1.
 * Error bound, u = 2^-53, U = max |b (e[n] - e0) + c (v[n] - v0)| over samples and states or targets, A = max |ln count[k] +
 *   f[k]| over the centred f (derivation: csrc/nm_reweight.h): logd is off by at most (K/2 + 24) u + 4 u (U + A) + u |logd|, one
 *   application of the map and tf by that plus (min(N, 4096)/128 + N/2^18 + 64) u + 4 u (U + A).
 * Determinism.  The same bits on every call: every sum runs in a fixed order, no floating-point atomics.
 * No K x N array exists at any time: device memory is 3 N doubles, the observables, and a partial per (state, 4096 samples).
 *
 * Reweighted histograms of any per-sample quantity with the same weights (the probability distribution p(x | P, T), not only
 * its mean): nm_reweight_hist.h, included below; its function is part of this interface and follows the same rules.
 *
 * Both functions return 0 or a negative NM_ERR_* code (include/nm.h); message via nm_reweight_last_error(), starting with the
 * function's name.  NM_ERR_ARG, checked before the device is looked for and with every output left untouched, for: nstates
 * outside 1..4096, nsamples < 1, a count that is negative or counts that do not sum to nsamples, a non-finite value in b, c,
 * e, v, f, tb or tc, tol < 0 (or NaN), max_iter < 1, ntargets outside 1..65536, nobs outside 0..8, a needed pointer that is
 * null (obs or omean with nobs > 0 included), a bad device ordinal.  NM_ERR_HIP without a device or when a HIP call fails.
 */
#ifndef NM_REWEIGHT_H
#define NM_REWEIGHT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The self-consistent iteration.  b, c [nstates], count [nstates], e, v [nsamples].
 * f [nstates]: in, the start (any finite values; a good one is the mean of u_k over state k's own samples); out, the
 *   result, f[0] = 0.
 * logd [nsamples] or NULL: the denominators that the LAST application of the map used, that is, of the f that went into it
 *   (of the start where *iters = 1).
 * *iters: the number of applications made, 1..max_iter; *delta: the last one's delta.
 * NM_OK whenever the arithmetic ran: the caller judges convergence from *iters and *delta.  max_iter = 1 returns exactly
 * one application of the map. */
int nm_reweight_solve(int device, int nstates, const double *b, const double *c, const int64_t *count, int64_t nsamples,
                      const double *e, const double *v, double tol, int max_iter, double *f, double *logd, int *iters,
                      double *delta);

/* Expectations at ntargets targets from the states' f (as nm_reweight_solve returned it; any f[0]).
 * tb, tc [ntargets]; obs [nobs][nsamples] or NULL with nobs = 0.
 * tf, ess [ntargets]; mean [ntargets][2] = (<e>, <v>); cov [ntargets][3] = (var_e, cov_ev, var_v); omean [ntargets][nobs]
 * (not read or written with nobs = 0, may then be NULL). */
int nm_reweight_expect(int device, int nstates, const double *b, const double *c, const int64_t *count, const double *f,
                       int64_t nsamples, const double *e, const double *v, int ntargets, const double *tb, const double *tc,
                       int nobs, const double *obs, double *tf, double *ess, double *mean, double *cov, double *omean);

const char *nm_reweight_last_error(void);

#ifdef __cplusplus
}
#endif
#include "nm_reweight_hist.h"
#endif
