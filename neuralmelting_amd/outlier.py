"""Outliers between pca and the manifold: the local outlier factor of every grid point's samples among themselves (DESIGN.md §9
row f-10; include/nm_distr.h).  lammps_vae.py's inlier selection (-ad) fits sklearn's LocalOutlierFactor(contamination='auto'),
20 neighbours, to the projections of each (P, T) grid point alone and embeds and clusters only the inliers; this stage computes the
same factor for all PN TN grid points in one call of the HIP library (nm_distr_lof: one pass over each set's pairs that keeps
the k nearest of each sample, then two gathers; there is no host fallback), and `manifold -il` and `cluster -il` leave the outliers out:

    python -m neuralmelting_amd.pca -v -n remcmc_run_5 -e LJ -sk 128
    python -m neuralmelting_amd.outlier -v -n remcmc_run_5 -e LJ -sk 128
    python -m neuralmelting_amd.manifold -v -n remcmc_run_5 -e LJ -sk 128 -il
    python -m neuralmelting_amd.cluster -v -n remcmc_run_5 -e LJ -sk 128 -il -em mfy -nc 0.02
    python -m neuralmelting_amd.reweight -v -n remcmc_run_5 -e LJ -sk 128 -ob cdf.loi

The samples that a chain produces while it crosses between two phases, or before it has equilibrated, are few and lie apart from
the rest of their grid point: the inlier fraction `.F.loi` as a curve in T dips where the phases coexist.  The projections are
taken as they are, as the reference takes them: the factor's 1e-10 is absolute (include/nm_distr.h).
"""
import argparse
import sys

import numpy as np

from . import _lib as B
from . import _stage as S

MAX_SETS, MAX_PTS, MAX_POINTS, MAX_DIM, MAX_K = 2 ** 20, 4096, 2 ** 21, 16, 64     # include/nm_distr.h: nm_distr_lof


def parse_args(argv=None):
    p = argparse.ArgumentParser(
        description='The local outlier factor of the projections .F.pcz of pca, every (P, T) grid point a set of its own: .F.lof (PN, TN, SN) '
        'float64 the factor, NaN for samples left out; .F.lod (PN, TN, SN) float64 the local reachability density (NaN likewise); .F.loi '
        '(PN, TN, SN) float64, 1 where lof <= TH, 0 for outliers and for samples left out, for reweight -ob F.loi; .F.lon (PN, TN) int32 '
        'the outliers of each grid point.')
    p.add_argument('-v', '--verbose', action='store_true')
    p.add_argument('-n', '--name', type=str, default='remcmc_init')
    p.add_argument('-e', '--element', type=str, default='LJ')
    p.add_argument('-ft', '--feature', type=str, default='cdf', help='the feature F whose projections <PREFIX>.F.pcz.npy are screened')
    p.add_argument('-nd', '--dimensions', type=int, default=None, help='leading components used, 1..16 and at most LD (default: all)')
    p.add_argument('-nn', '--neighbours', type=int, default=20, help='neighbours of a sample within its grid point, 1..64')
    p.add_argument('-th', '--threshold', type=float, default=1.5, help="a sample is an outlier where lof > TH (sklearn's 'auto': 1.5)")
    p.add_argument('-sk', '--skip', type=int, default=0, help='samples of every grid point left out at its start')
    p.add_argument('-sd', '--stride', type=int, default=1, help='every STRIDE-th sample is screened')
    p.add_argument('-dv', '--device', type=int, default=0)
    a = p.parse_args(argv)
    if (a.skip < 0 or a.stride < 1 or (a.dimensions is not None and not 1 <= a.dimensions <= MAX_DIM) or a.neighbours < 1
            or not (np.isfinite(a.threshold) and a.threshold > 0.0)):
        p.error('need -sk >= 0, -sd >= 1, -nd in 1..16, -nn >= 1 and a finite -th > 0')
    return a


def lof(x, k, device=0, neighbours=False):
    """nm_distr_lof of x (NSETS, NPTS, ND), every set alone: (lof, lrd, kdist (NSETS, NPTS)), and with `neighbours` also
    nbr (NSETS, NPTS, k) int32, the indices within the set"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError('x wants the shape (NSETS, NPTS, ND)')
    nsets, npts, nd = x.shape
    factor, lrd, kdist = np.empty((nsets, npts)), np.empty((nsets, npts)), np.empty((nsets, npts))
    nbr = np.empty((nsets, npts, max(int(k), 0)), dtype=np.int32) if neighbours else None
    B.call('nm_distr_lof', device, nsets, npts, nd, x, int(k), factor, lrd, kdist, nbr)
    return (factor, lrd, kdist, nbr) if neighbours else (factor, lrd, kdist)


def main(argv=None):
    a = parse_args(argv)
    el, ft, k = a.element, a.feature, a.neighbours
    prefix = S.prefix(a.name, el)
    P, T, pe, pcz, path = S.grid_inputs('outlier', prefix, ft + '.pcz', 'the components')
    pn, tn, sn, ld = pcz.shape
    nd = ld if a.dimensions is None else a.dimensions
    if nd > ld or nd > MAX_DIM:
        raise SystemExit('outlier: -nd %d is more than the %d components of %s or than %d' % (nd, ld, path, MAX_DIM))
    kept, xk = S.kept(pcz, a.skip, a.stride)
    if not 2 <= kept <= MAX_PTS:
        raise SystemExit('outlier: -sk %d -sd %d leave %d samples of every grid point of %s, not 2..%d' % (a.skip, a.stride, kept, path, MAX_PTS))
    if not 1 <= k <= min(kept - 1, MAX_K):
        raise SystemExit('outlier: -nn %d neighbours among %d samples: need 1..%d' % (k, kept, min(kept - 1, MAX_K)))
    if pn * tn > MAX_SETS or pn * tn * kept > MAX_POINTS:
        raise SystemExit('outlier: %d grid points of %d samples of %s are more than %d sets or %d samples' % (pn * tn, kept, path, MAX_SETS, MAX_POINTS))
    x = np.ascontiguousarray(xk[..., :nd], dtype=np.float64).reshape(pn * tn, kept, nd)
    if a.verbose:
        print('%d sets of %d of %d samples of %s in %d components, %d neighbours' % (pn * tn, kept, sn, ft, nd, k))
    try:
        factor, lrd, _ = lof(x, k, a.device)
    except (RuntimeError, ValueError) as err:
        raise SystemExit('outlier: %s: %s' % (path, err))
    factor, lrd = factor.reshape(pn, tn, kept), lrd.reshape(pn, tn, kept)
    inlier = factor <= a.threshold
    count = (~inlier).sum(axis=2).astype(np.int32)
    np.save(prefix + '.%s.lof.npy' % ft, S.spread(factor, pe.shape, a.skip, a.stride, np.nan))
    np.save(prefix + '.%s.lod.npy' % ft, S.spread(lrd, pe.shape, a.skip, a.stride, np.nan))
    np.save(prefix + '.%s.loi.npy' % ft, S.spread(inlier.astype(np.float64), pe.shape, a.skip, a.stride, 0.0))
    np.save(prefix + '.%s.lon.npy' % ft, count)
    if a.verbose:
        ip, it = np.unravel_index(int(count.argmax()), count.shape)
        print('lof %.4g .. %.4g, median %.4g; %d of %d samples (%.3g %%) are outliers at lof > %g' % (
            factor.min(), factor.max(), np.median(factor), count.sum(), factor.size, 100.0 * count.sum() / factor.size, a.threshold))
        print('the most, %d of %d, at grid point (%d, %d): P %g, T %g' % (count[ip, it], kept, ip, it, P[ip], T[it]))
    return 0


if __name__ == '__main__':
    sys.exit(main())
