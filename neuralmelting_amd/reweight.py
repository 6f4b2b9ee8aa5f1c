"""Multistate reweighting of the replica grid (include/nm_reweight.h): free energies of the P x T
states, and enthalpy, volume and heat capacity as continuous curves in T at every pressure, from what `parse` wrote.

A replica-exchange run over a P x T grid is the input of MBAR (Shirts and Chodera 2008): every sample of every replica
contributes to every state.  The reference locates the transition with a VAE on the histograms instead (lammps_vae.py);
this stage is the build's own.  The arithmetic runs in the HIP library (nm_reweight_solve, nm_reweight_expect,
nm_reweight_histogram), there is no host fallback.

What makes the grid's samples the samples of its states: the sampler's exchange moves configurations between slots, never
temperatures or pressures between configurations (remcmc.py, Run.replica_exchange / exchange.sweep: the energies, volumes
and the slot-to-buffer map are swapped, et and pf stay with the slot), the record of a cycle is taken behind the cycle's
block of moves and in front of its exchange (Run.main), and slot k = p * TN + t writes the files of grid index (p, t)
(Run.file_prefix).  So row (p, t) of `.pe.npy` / `.vol.npy` holds samples generated at the target (P_p, T_t).  The reduced
potential uses the potential energy: the kinetic energy of a record is that of the HMC move's fresh momenta, Gaussian at the
state's temperature whatever the configuration, and integrates out of every configurational average.

    python -m neuralmelting_amd.reweight -v -n remcmc_run_5 -e LJ -sk 128 -ob sof sol
    python -m neuralmelting_amd.reweight -v -n remcmc_run_5 -e LJ -sk 128 -hq sof pe vol -hx 0.5     # p(x | P, T) and the equal-weight T
    python -m neuralmelting_amd.reweight -v -n remcmc_run_5 -e LJ -sk 128 -hq sof -hx 0.5 -bs 200    # and block-bootstrap error bars

Error bars (-bs R; include/nm_reweight_boot.h): every grid point's samples are a time series, so each state's series is
resampled in blocks as long as its statistical inefficiency (circular moving-block bootstrap), the whole solve and the
expectations are repeated on the R resampled sets in one batched call each (nm_reweight_boot_solve, nm_reweight_boot_expect),
and the spread over the replicates is written next to every value.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

from . import _lib as B
from ._stage import prefix as run_prefix
from .remcmc import init_constant

MAX_OBS = 8
MAX_TARGETS = 65536     # include/nm_reweight.h: ntargets of one call
MAX_HIST, MAX_BINS = 8, 1024    # include/nm_reweight_hist.h: nq and nbins
SUFFIXES = ('rwf', 'rwi', 'rwt', 'rwg', 'rwh', 'rwv', 'rwc', 'rwn', 'rwo', 'rwm')
HIST_SUFFIXES = ('rwx', 'rwp', 'rwa', 'rwe')    # written with -hq only (rwa, rwe with -hx only)
MAX_REP = 1024          # include/nm_reweight_boot.h: nrep of one call
BOOT_SUFFIXES = ('rwb', 'rwbi', 'rwfs', 'rwgs', 'rwhs', 'rwvs', 'rwcs', 'rwos', 'rwms', 'rwes')   # written with -bs only (rwos with -ob, rwes with -hx)


def parse_args(argv=None):
    p = argparse.ArgumentParser(
        description='MBAR reweighting of the (P, T) grid: .rwf (PN, TN) the states\' reduced free energies f (f[0, 0] = 0); .rwi '
        '(iterations, delta, tol); .rwt (TG,) the fine temperatures; and on (PN, TG): .rwg reduced free energy, .rwh enthalpy per '
        'atom, .rwv volume per atom, .rwc configurational Cp / (natoms kB) - the kinetic 3/2 is NOT included -, .rwn the Kish '
        'effective sample size, .rwo (PN, TG, nobs) the observables of -ob; .rwm (PN,) the temperature of the largest Cp on the '
        'fine grid.  A peak on an end of the range means that the transition is not bracketed: the value is written as it is.  With '
        '-hq: .rwx (nq, NBINS + 1) the bin edges and .rwp (PN, TG, nq, NBINS) the reweighted probability of every bin; with -hx: .rwa '
        '(PN, TG) the weight at or above the cut and .rwe (PN,) the temperature where it first crosses 1/2 (NaN without a crossing).  '
        'With -bs R, from R block-bootstrap replicates of the whole solve: .rwb (PN, TN, 2) every state\'s statistical inefficiency g and '
        'block length; .rwbi (R, 3) iterations, delta, status (0 converged, 1 not, 2 no overlap left: left out everywhere); the standard '
        'deviations (ddof 1) .rwfs (PN, TN) of f, .rwgs .rwhs .rwvs .rwcs (PN, TG) and .rwos (PN, TG, nobs) of the curves; .rwms (PN, 4) '
        'for the temperature of the largest Cp: standard deviation, 2.5 % and 97.5 % quantiles, replicates used; .rwes (PN, 4) the same '
        'for the equal-weight temperature of -hx (replicates without a crossing are left out).')
    p.add_argument('-v', '--verbose', action='store_true')
    p.add_argument('-n', '--name', type=str, default='remcmc_init')
    p.add_argument('-e', '--element', type=str, default='LJ')
    p.add_argument('-sk', '--skip', type=int, default=0, help='samples dropped at the start of every grid point')
    p.add_argument('-sd', '--stride', type=int, default=1, help='keep every STRIDE-th sample')
    p.add_argument('-tg', '--temperature_grid', type=int, default=256,
                   help='fine temperatures per pressure, linspace(T[0], T[-1], TG).  The defaults of -tg, -rt and -ri are conveniences: '
                   'whether they suit the LJ and Sutton-Chen grids has not been measured')
    p.add_argument('-rt', '--tolerance', type=float, default=1e-9, help='the iteration stops at max |f_new - f_old| <= this')
    p.add_argument('-ri', '--max_iterations', type=int, default=20000,
                   help='most applications of the map; if delta > tol then, the files are still written and the exit status is 1')
    p.add_argument('-ob', '--observables', type=str, nargs='+', default=[],
                   help='up to 8 names: <PREFIX>.NAME.npy of shape (PN, TN, SN) is averaged with the weights (e.g. distr\'s sof, sol)')
    p.add_argument('-hq', '--histogram', type=str, nargs='+', default=[],
                   help='up to 8 names to histogram with the weights: pe (potential energy per atom), vol (volume per atom), or a name as '
                   'behind -ob.  The edges are linspace(min, max, NBINS + 1) of the kept samples (min - 0.5 .. min + 0.5 for a constant)')
    p.add_argument('-hb', '--histogram_bins', type=int, default=128, help='NBINS of -hq, 1..1024')
    p.add_argument('-hx', '--histogram_cut', type=float, default=None,
                   help='a cut on the first name of -hq, moved to the nearest bin edge: the weight at or above it and its crossing of 1/2')
    p.add_argument('-bs', '--bootstrap', type=int, default=0, help='block-bootstrap replicates, 1..1024; 0: no error bars')
    p.add_argument('-bl', '--block_length', type=int, default=0,
                   help='block length of -bs in kept samples; 0: per state ceil(g) of its own b e + c v series')
    p.add_argument('-bd', '--bootstrap_seed', type=int, default=256, help='seed of the Philox generator that draws the blocks')
    p.add_argument('-dv', '--device', type=int, default=0)
    a = p.parse_args(argv)
    if not 0 <= a.bootstrap <= MAX_REP or a.block_length < 0 or a.bootstrap_seed < 0:
        p.error('need -bs in 1..1024 (0: off), -bl >= 0 and -bd >= 0')
    if a.bootstrap and a.histogram_cut is not None and len(a.observables) > MAX_OBS - 1:
        p.error('-bs with -hx passes the cut as one more observable: at most 7 names behind -ob')
    if a.histogram_cut is not None and not a.histogram:
        p.error('-hx needs -hq')
    if len(a.histogram) > MAX_HIST or not 1 <= a.histogram_bins <= MAX_BINS or (a.histogram_cut is not None and not np.isfinite(a.histogram_cut)):
        p.error('need at most 8 names behind -hq, -hb in 1..1024 and a finite -hx')
    if a.skip < 0 or a.stride < 1 or not 1 <= a.temperature_grid <= MAX_TARGETS or a.max_iterations < 1 or not a.tolerance >= 0 or len(a.observables) > MAX_OBS:
        p.error('need -sk >= 0, -sd >= 1, -tg in 1..65536 (PN x TG <= 65536), -ri >= 1, -rt >= 0 and at most 8 names behind -ob')
    return a


def _f64(x):
    return np.ascontiguousarray(x, dtype=np.float64)


def states(P, T, el):
    """(b, c) of the K = PN x TN states, k = p * TN + t: 1/et and pf of remcmc.init_constant"""
    et, pf = np.array([init_constant(P, T, el, i, j) for i in range(len(P)) for j in range(len(T))], dtype=np.float64).T
    return 1.0 / et, np.ascontiguousarray(pf)


def solve(b, c, count, e, v, f0=None, tol=1e-9, max_iter=20000, device=0, want_logd=False):
    """nm_reweight_solve: (f, iterations, delta[, logd]); f0 = None starts from zeros"""
    b, c, e, v = _f64(b), _f64(c), _f64(e).reshape(-1), _f64(v).reshape(-1)
    count = np.ascontiguousarray(count, dtype=np.int64)
    f = np.zeros(b.size) if f0 is None else _f64(f0).copy()
    if not (b.size == c.size == count.size == f.size and e.size == v.size):
        raise ValueError('b, c, count, f0 want one length and e, v another')
    logd = np.empty(e.size) if want_logd else None
    iters, delta = C.c_int(0), C.c_double(0.0)
    B.call('nm_reweight_solve', device, b.size, b, c, count, e.size, e, v, tol, max_iter, f, logd, C.byref(iters), C.byref(delta))
    return (f, iters.value, delta.value, logd) if want_logd else (f, iters.value, delta.value)


def expect(b, c, count, f, e, v, tb, tc, obs=None, device=0):
    """nm_reweight_expect: dict of tf, ess (T,), mean (T, 2), cov (T, 3), omean (T, nobs); obs (nobs, N) or None"""
    b, c, f, e, v = _f64(b), _f64(c), _f64(f), _f64(e).reshape(-1), _f64(v).reshape(-1)
    tb, tc = _f64(tb).reshape(-1), _f64(tc).reshape(-1)
    count = np.ascontiguousarray(count, dtype=np.int64)
    obs = None if obs is None or len(obs) == 0 else _f64(obs).reshape(len(obs), -1)
    nobs = 0 if obs is None else obs.shape[0]
    if not (b.size == c.size == count.size == f.size and e.size == v.size and tb.size == tc.size) or (nobs and obs.shape[1] != e.size):
        raise ValueError('b, c, count, f want one length, e, v and every observable another, tb, tc a third')
    nt = tb.size
    out = dict(tf=np.empty(nt), ess=np.empty(nt), mean=np.empty((nt, 2)), cov=np.empty((nt, 3)), omean=np.empty((nt, nobs)))
    B.call('nm_reweight_expect', device, b.size, b, c, count, f, e.size, e, v, nt, tb, tc, nobs, obs, out['tf'], out['ess'], out['mean'],
           out['cov'], out['omean'] if nobs else None)
    return out


def histogram(b, c, count, f, e, v, tb, tc, x, edges, device=0):
    """nm_reweight_histogram: (hist (T, nq, nbins), outside (T, nq, 2)); x (nq, N), edges (nq, nbins + 1)"""
    b, c, f, e, v = _f64(b), _f64(c), _f64(f), _f64(e).reshape(-1), _f64(v).reshape(-1)
    tb, tc = _f64(tb).reshape(-1), _f64(tc).reshape(-1)
    count = np.ascontiguousarray(count, dtype=np.int64)
    x, edges = _f64(x), _f64(edges)
    if not (b.size == c.size == count.size == f.size and e.size == v.size and tb.size == tc.size) or x.ndim != 2 or edges.ndim != 2 \
            or x.shape[1] != e.size or edges.shape[0] != x.shape[0] or edges.shape[1] < 2:
        raise ValueError('b, c, count, f want one length, e, v another, tb, tc a third; x (nq, N) and edges (nq, nbins + 1)')
    nt, nq, nbins = tb.size, x.shape[0], edges.shape[1] - 1
    hist, outside = np.empty((nt, nq, nbins)), np.empty((nt, nq, 2))
    B.call('nm_reweight_histogram', device, b.size, b, c, count, f, e.size, e, v, nt, tb, tc, nq, x, nbins, edges, hist, outside)
    return hist, outside


def boot_solve(b, c, count, e, v, f, mult, tol=1e-9, max_iter=20000, device=0):
    """nm_reweight_boot_solve: (fr (R, K), iters (R,), delta (R,), status (R,)); f the base solution, mult (R, N) uint16"""
    b, c, f, e, v = _f64(b), _f64(c), _f64(f), _f64(e).reshape(-1), _f64(v).reshape(-1)
    count = np.ascontiguousarray(count, dtype=np.int64)
    mult = np.ascontiguousarray(mult, dtype=np.uint16)
    if not (b.size == c.size == count.size == f.size and e.size == v.size) or mult.ndim != 2 or mult.shape[1] != e.size:
        raise ValueError('b, c, count, f want one length, e, v another; mult (R, N)')
    nrep = mult.shape[0]
    fr, delta = np.empty((nrep, b.size)), np.empty(nrep)
    iters, status = np.empty(nrep, dtype=np.intc), np.empty(nrep, dtype=np.intc)
    B.call('nm_reweight_boot_solve', device, b.size, b, c, count, e.size, e, v, f, nrep, mult, tol, max_iter, fr, iters, delta, status)
    return fr, iters, delta, status


def boot_expect(b, c, count, f, e, v, mult, fr, tb, tc, obs=None, device=0):
    """nm_reweight_boot_expect: dict of tf, ess (R, T), mean (R, T, 2), cov (R, T, 3), omean (R, T, nobs)"""
    b, c, f, e, v = _f64(b), _f64(c), _f64(f), _f64(e).reshape(-1), _f64(v).reshape(-1)
    tb, tc, fr = _f64(tb).reshape(-1), _f64(tc).reshape(-1), _f64(fr)
    count = np.ascontiguousarray(count, dtype=np.int64)
    mult = np.ascontiguousarray(mult, dtype=np.uint16)
    obs = None if obs is None or len(obs) == 0 else _f64(obs).reshape(len(obs), -1)
    nobs = 0 if obs is None else obs.shape[0]
    if not (b.size == c.size == count.size == f.size and e.size == v.size and tb.size == tc.size) or (nobs and obs.shape[1] != e.size) \
            or mult.ndim != 2 or mult.shape[1] != e.size or fr.shape != (mult.shape[0], b.size):
        raise ValueError('b, c, count, f want one length, e, v and every observable another, tb, tc a third; mult (R, N), fr (R, K)')
    nrep, nt = mult.shape[0], tb.size
    out = dict(tf=np.empty((nrep, nt)), ess=np.empty((nrep, nt)), mean=np.empty((nrep, nt, 2)), cov=np.empty((nrep, nt, 3)),
               omean=np.empty((nrep, nt, nobs)))
    B.call('nm_reweight_boot_expect', device, b.size, b, c, count, f, e.size, e, v, nrep, mult, fr, nt, tb, tc, nobs, obs, out['tf'],
           out['ess'], out['mean'], out['cov'], out['omean'] if nobs else None)
    return out


def statistical_inefficiency(x):
    """g = 1 + 2 sum_{t >= 1} (1 - t/n) C(t) of a time series, C(t) = mean_i(dx_i dx_{i+t}) / mean(dx^2) over the n - t pairs, summed
    up to the first C(t) <= 0; 1 for a constant series or one of length 1, never below 1"""
    x = _f64(x).reshape(-1)
    n = x.size
    if n < 2:
        return 1.0
    dx = x - x.mean()
    var = float(dx @ dx) / n
    if not var > 0.0:
        return 1.0
    g = 1.0
    for t in range(1, n):
        ct = float(dx[:-t] @ dx[t:]) / ((n - t) * var)
        if ct <= 0.0:
            break
        g += 2.0 * (1.0 - t / n) * ct
    return max(g, 1.0)


def _draw_starts(rng, sn, nb):
    return rng.integers(0, sn, nb)


def block_multiplicities(sn, L, nrep, seed):
    """circular moving-block bootstrap of K series of sn samples each: uint16 (nrep, K, sn), how often every sample is drawn.  L: the
    block length, one int for a single series or K of them.  Per replicate and series (in that order) ceil(sn / L) block starts are
    drawn uniformly from numpy.random.Generator(Philox(seed)); a block is L consecutive samples, wrapping round; the draws are cut
    to sn.  L >= sn is the series itself: all ones.  ValueError where a count exceeds 65535."""
    L = np.atleast_1d(np.asarray(L, dtype=np.int64))
    if sn < 1 or nrep < 1 or (L < 1).any():
        raise ValueError('block_multiplicities: sn, nrep and every L must be at least 1')
    rng = np.random.Generator(np.random.Philox(seed))
    out = np.empty((nrep, L.size, sn), dtype=np.uint16)
    for r in range(nrep):
        for k, lk in enumerate(np.minimum(L, sn)):
            starts = np.asarray(_draw_starts(rng, sn, -(-sn // int(lk))), dtype=np.int64)
            idx = (starts[:, None] + np.arange(lk)[None, :]).reshape(-1)[:sn] % sn
            cnt = np.bincount(idx, minlength=sn)
            if cnt.max() > 65535:
                raise ValueError('block_multiplicities: a sample is drawn %d times, more than the 65535 of a uint16' % cnt.max())
            out[r, k] = cnt
    return out


def _spread(x):
    """the standard deviation (ddof 1) over the first axis; NaN with fewer than two replicates"""
    return np.std(x, axis=0, ddof=1) if x.shape[0] > 1 else np.full(x.shape[1:], np.nan)


def _interval(x):
    """(PN, 4) of the replicates' values x (R, PN), NaN = left out: standard deviation, 2.5 % and 97.5 % quantiles, replicates used"""
    out = np.full((x.shape[1], 4), np.nan)
    for p in range(x.shape[1]):
        y = x[:, p][~np.isnan(x[:, p])]
        out[p, 3] = y.size
        if y.size > 1:
            out[p, 0] = np.std(y, ddof=1)
        if y.size > 0:
            out[p, 1:3] = np.quantile(y, [0.025, 0.975])
    return out


def boot_spreads(fr, status, tfine, tb, tc, ex, natoms, nobs, with_cut):
    """the arrays of -bs, keyed by suffix, from the replicates' solutions fr (R, PN, TN), their status and nm_reweight_boot_expect's
    results: curves() per replicate, replicates of status 2 left out.  with_cut: the last observable is the indicator of -hx"""
    use = np.nonzero(np.asarray(status) != 2)[0]
    per = [curves(fr[r], 0, 0.0, 0.0, tfine, tb, tc, {key: val[r] for key, val in ex.items()}, natoms) for r in use]
    stack = lambda key: np.stack([c[key] for c in per]) if per else np.empty((0,) + tb.shape)
    out = dict(rwfs=_spread(fr[use]), rwgs=_spread(stack('rwg')), rwhs=_spread(stack('rwh')), rwvs=_spread(stack('rwv')),
               rwcs=_spread(stack('rwc')), rwms=_interval(np.stack([c['rwm'] for c in per]) if per else np.empty((0, tb.shape[0]))))
    if nobs:
        out['rwos'] = _spread(np.stack([c['rwo'][..., :nobs] for c in per]) if per else np.empty((0,) + tb.shape + (nobs,)))
    if with_cut:
        out['rwes'] = _interval(np.stack([equal_weight(tfine, c['rwo'][..., -1]) for c in per]) if per else np.empty((0, tb.shape[0])))
    return out


def equal_weight(tfine, above):
    """per pressure the temperature where `above` (PN, TG), the weight above a cut, first crosses 1/2: the first pair of
    neighbouring fine temperatures with (a_i - 1/2)(a_i+1 - 1/2) <= 0 and a_i != a_i+1, interpolated linearly in T; NaN where
    there is none (a flat stretch at 1/2 is no crossing)"""
    tfine, d = _f64(tfine), np.atleast_2d(_f64(above)) - 0.5
    out = np.full(d.shape[0], np.nan)
    for p, row in enumerate(d):
        hit = np.nonzero((row[:-1] * row[1:] <= 0.0) & (row[:-1] != row[1:]))[0]
        if hit.size:
            i = hit[0]
            out[p] = tfine[i] + (tfine[i + 1] - tfine[i]) * (row[i] / (row[i] - row[i + 1]))
    return out


def linear_edges(x, nbins):
    """linspace(min, max, nbins + 1) of every row of x (nq, N); min - 0.5 .. min + 0.5 for a constant row"""
    lo, hi = x.min(axis=1), x.max(axis=1)
    flat = lo == hi
    return np.stack([np.linspace(l - 0.5 if s else l, l + 0.5 if s else h, nbins + 1) for l, h, s in zip(lo, hi, flat)])


def cut_weight(hist, edges, cut):
    """(the weight (T,) of the bins of quantity 0 at or above the edge nearest to `cut`, that edge)"""
    j = int(np.argmin(np.abs(edges[0] - cut)))
    return hist[:, 0, j:].sum(axis=1), float(edges[0, j])


def fine_targets(P, T, el, tg):
    """the fine temperatures (TG,) and the targets (tb, tc), each (PN, TG), with init_constant's constants"""
    tf = np.linspace(float(T[0]), float(T[-1]), tg)
    tb, tc = states(np.asarray(P, dtype=np.float64), tf, el)
    return tf, tb.reshape(len(P), tg), tc.reshape(len(P), tg)


def curves(f, iters, delta, tol, tfine, tb, tc, ex, natoms):
    """the ten arrays, keyed by suffix, from the solution (f (PN, TN), iters, delta, tol), the fine temperatures (TG,), the
    targets tb, tc (PN, TG) and nm_reweight_expect's results for them in that order; host arithmetic only.
    H = <e> + (c/b) <v>: c/b is the pressure in energy per volume.  Cp here is d<H>/dT at constant P per atom and kB,
    (b^2 var_e + 2 b c cov_ev + c^2 var_v) / natoms = var(u) / natoms, without the kinetic 3/2."""
    pn, tg = tb.shape
    mean, cov = ex['mean'].reshape(pn, tg, 2), ex['cov'].reshape(pn, tg, 3)
    n = float(natoms)
    cp = (tb * tb * cov[..., 0] + 2.0 * tb * tc * cov[..., 1] + tc * tc * cov[..., 2]) / n
    return dict(rwf=_f64(f), rwi=np.array([float(iters), float(delta), float(tol)]), rwt=_f64(tfine),
                rwg=ex['tf'].reshape(pn, tg), rwh=(mean[..., 0] + tc / tb * mean[..., 1]) / n, rwv=mean[..., 1] / n, rwc=cp,
                rwn=ex['ess'].reshape(pn, tg), rwo=ex['omean'].reshape(pn, tg, -1), rwm=_f64(tfine)[np.argmax(cp, axis=1)])


def load_observables(prefix, names, shape, flag='-ob'):
    """the (PN, TN, SN) arrays of -ob (or -hq), or ValueError naming the file that is missing or misshapen"""
    out = []
    for name in names:
        path = prefix + '.%s.npy' % name
        if not os.path.isfile(path):
            raise ValueError('%s %s: %s is missing' % (flag, name, path))
        a = np.load(path)
        if a.shape != tuple(shape):
            raise ValueError('%s %s: %s has shape %s, not %s' % (flag, name, path, a.shape, tuple(shape)))
        out.append(a)
    return out


def main(argv=None):
    a = parse_args(argv)
    el = a.element
    prefix = run_prefix(a.name, el)
    P = np.load(prefix + '.virial.trgt.npy')
    T = np.load(prefix + '.temp.trgt.npy')
    pe = np.load(prefix + '.pe.npy')
    vol = np.load(prefix + '.vol.npy')
    natoms = int(np.load(prefix + '.natoms.npy').reshape(-1)[0])
    pn, tn = P.size, T.size
    if pn * a.temperature_grid > MAX_TARGETS:
        raise SystemExit('reweight: -tg %d at %d pressures is more than the %d targets of one nm_reweight_expect call' % (a.temperature_grid, pn, MAX_TARGETS))
    if pe.shape != vol.shape or pe.shape[:2] != (pn, tn):
        raise SystemExit('reweight: .pe.npy %s and .vol.npy %s do not fit the %d x %d grid' % (pe.shape, vol.shape, pn, tn))
    try:
        obs = load_observables(prefix, a.observables, pe.shape)         # refused before anything is written
        hq = [_f64(pe) / natoms if name == 'pe' else _f64(vol) / natoms if name == 'vol' else load_observables(prefix, [name], pe.shape, '-hq')[0]
              for name in a.histogram]
    except ValueError as err:
        raise SystemExit('reweight: %s' % err)
    keep = slice(a.skip, None, a.stride)
    e = _f64(pe[:, :, keep]).reshape(pn * tn, -1)
    v = _f64(vol[:, :, keep]).reshape(pn * tn, -1)
    sn = e.shape[1]
    if sn < 1:
        raise SystemExit('reweight: -sk %d leaves no sample' % a.skip)
    obs = [_f64(o[:, :, keep]).reshape(-1) for o in obs]
    x = np.stack([_f64(q[:, :, keep]).reshape(-1) for q in hq]) if hq else None
    if hq and not np.isfinite(x).all():
        raise SystemExit('reweight: -hq: a kept sample is not finite')
    b, c = states(P, T, el)
    count = np.full(pn * tn, sn, dtype=np.int64)
    f0 = b * e.mean(axis=1) + c * v.mean(axis=1)                        # the mean of u_k over state k's own samples
    if a.verbose:
        print('reweighting %d states x %d samples of %d atoms' % (pn * tn, pn * tn * sn, natoms))
    f, iters, delta = solve(b, c, count, e, v, f0, a.tolerance, a.max_iterations, a.device)
    tfine, tb, tc = fine_targets(P, T, el, a.temperature_grid)
    ex = expect(b, c, count, f, e, v, tb, tc, obs, a.device)
    out = curves(f.reshape(pn, tn), iters, delta, a.tolerance, tfine, tb, tc, ex, natoms)
    for key in SUFFIXES:
        if key != 'rwo' or obs:
            np.save(prefix + '.%s.npy' % key, out[key])
    if a.verbose:
        print('%d iterations, delta %.3g; largest Cp at T = %s' % (iters, delta, np.array2string(out['rwm'], precision=4)))
    if hq:
        edges = linear_edges(x, a.histogram_bins)
        hist, _ = histogram(b, c, count, f, e, v, tb, tc, x, edges, a.device)
        np.save(prefix + '.rwx.npy', edges)
        np.save(prefix + '.rwp.npy', hist.reshape(pn, a.temperature_grid, len(hq), a.histogram_bins))
        if a.histogram_cut is not None:
            above, at = cut_weight(hist, edges, a.histogram_cut)
            above = above.reshape(pn, a.temperature_grid)
            np.save(prefix + '.rwa.npy', above)
            np.save(prefix + '.rwe.npy', equal_weight(tfine, above))
            if a.verbose:
                print('-hx %g on %s: the cut is the edge %.9g; equal weight at T = %s' % (
                    a.histogram_cut, a.histogram[0], at, np.array2string(equal_weight(tfine, above), precision=4)))
    status = 0
    if a.bootstrap:
        series = b[:, None] * e + c[:, None] * v                        # a state's own reduced potential, the series that is blocked
        g = np.array([statistical_inefficiency(row) for row in series])
        length = np.full(g.size, a.block_length, dtype=np.int64) if a.block_length else np.minimum(np.ceil(g), sn).astype(np.int64)
        try:
            mult = block_multiplicities(sn, length, a.bootstrap, a.bootstrap_seed).reshape(a.bootstrap, -1)
        except ValueError as err:
            raise SystemExit('reweight: %s' % err)
        fr, biters, bdelta, bstatus = boot_solve(b, c, count, e, v, f, mult, a.tolerance, a.max_iterations, a.device)
        bobs, with_cut = list(obs), bool(hq) and a.histogram_cut is not None
        if with_cut:                                                    # the weight at or above the cut's edge as one more observable
            j = int(np.argmin(np.abs(edges[0] - a.histogram_cut)))
            bobs.append((x[0] >= edges[0, j]).astype(np.float64) if j < a.histogram_bins else np.zeros(x.shape[1]))
        exb = boot_expect(b, c, count, f, e, v, mult, fr, tb, tc, bobs, a.device)
        sp = boot_spreads(fr.reshape(a.bootstrap, pn, tn), bstatus, tfine, tb, tc, exb, natoms, len(obs), with_cut)
        sp['rwb'] = np.stack([g, length.astype(np.float64)], axis=1).reshape(pn, tn, 2)
        sp['rwbi'] = np.stack([biters.astype(np.float64), bdelta, bstatus.astype(np.float64)], axis=1)
        for key in BOOT_SUFFIXES:
            if key in sp:
                np.save(prefix + '.%s.npy' % key, sp[key])
        if a.verbose:
            print('%d replicates, blocks of %d..%d samples; standard deviation of the largest-Cp temperature %s' % (
                a.bootstrap, length.min(), length.max(), np.array2string(sp['rwms'][:, 0], precision=4)))
        if (bstatus == 2).any():
            print('reweight: %d of %d bootstrap replicates kept no overlap (status 2) and are left out' % ((bstatus == 2).sum(), a.bootstrap),
                  file=sys.stderr)
        if (bstatus == 1).any():
            print('reweight: %d of %d bootstrap replicates did not converge: largest delta = %.6g > %g' % (
                (bstatus == 1).sum(), a.bootstrap, bdelta[bstatus == 1].max(), a.tolerance), file=sys.stderr)
            status = 1
    if not delta <= a.tolerance:
        print('reweight: not converged: delta = %.6g > %g after %d iterations' % (delta, a.tolerance, iters), file=sys.stderr)
        return 1
    return status


if __name__ == '__main__':
    sys.exit(main())
