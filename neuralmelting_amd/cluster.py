"""Phases from the embedding: DBSCAN of the principal components' projections over the whole replica grid (DESIGN.md §9 row f-7;
include/nm_cluster.h).  lammps_vae.py clusters its embedding into phases, DBSCAN being its default (-cl); this stage clusters the
leading projections that `pca` wrote, in the HIP library (nm_cluster_dbscan: three all-pairs scans and a lock-free union-find,
there is no host fallback), and gives every sample a phase label without a cut chosen by hand.

The indicators are per-sample observables of `.pe.npy`'s shape, so the reweighting stage takes them like any order parameter: the
liquid fraction as a curve in T, its equal-weight temperature and both with error bars:

    python -m neuralmelting_amd.pca -v -n remcmc_run_5 -e LJ -sk 128
    python -m neuralmelting_amd.cluster -v -n remcmc_run_5 -e LJ -sk 128 -nc 0.02
    python -m neuralmelting_amd.reweight -v -n remcmc_run_5 -e LJ -sk 128 -ob cdf.cl1 -hq cdf.cl1 -hx 0.5 -bs 200

The unit of -nc: the used components are divided by one factor, max - min of component 0 over the clustered points, so EPS is a
fraction of pc0's range and the geometry is unchanged.  There is no default: `.F.cld.npy`, the number of samples within EPS of each
sample, is the data to choose it from.  Of the NK largest clusters the one with the lowest mean target temperature is cl0 (on a
melting grid the solid), the next cl1 (the liquid).
"""
import argparse
import sys

import numpy as np

from . import _lib as B
from . import _stage as S
from ._stage import spread

MAX_POINTS, MAX_DIM, MAX_KEPT = 2 ** 21, 16, 8     # include/nm_cluster.h: npoints and ndim; the indicators of -nk


def parse_args(argv=None):
    p = argparse.ArgumentParser(
        description='DBSCAN of the projections .F.pcz of pca over the (P, T) grid: .F.cll (PN, TN, SN) int32 the labels, -1 for noise and for '
        'samples left out; .F.cld (PN, TN, SN) int32 the samples within EPS, the sample among them; .F.cls (K, 3 + ND) float64 per '
        'cluster: members, core members, mean target temperature, centroid in the projections; .F.cl0 ... (PN, TN, SN) float64 the '
        'membership indicators of the NK largest clusters from the coldest to the hottest, for reweight -ob F.cl1 -hq F.cl1 -hx 0.5.')
    p.add_argument('-v', '--verbose', action='store_true')
    p.add_argument('-n', '--name', type=str, default='remcmc_init')
    p.add_argument('-e', '--element', type=str, default='LJ')
    p.add_argument('-ft', '--feature', type=str, default='cdf', help='the feature F whose projections <PREFIX>.F.pcz.npy are clustered')
    p.add_argument('-em', '--embedding', type=str, default='pcz', choices=('pcz', 'mfy'),
                   help="what is clustered: pca's projections <PREFIX>.F.pcz.npy, or manifold's embedding <PREFIX>.F.mfy.npy of the same -sk and -sd")
    p.add_argument('-nd', '--dimensions', type=int, default=2, help='leading components used, 1..16 and at most LD')
    p.add_argument('-nc', '--neighbourhood', type=float, required=True, metavar='EPS',
                   help='the radius of a neighbourhood as a fraction of the range of component 0')
    p.add_argument('-ms', '--min_samples', type=int, default=5, help='samples within EPS, itself among them, that make a sample a core')
    p.add_argument('-nk', '--clusters_kept', type=int, default=2, help='phase indicators written, 1..8')
    p.add_argument('-sk', '--skip', type=int, default=0, help='samples of every grid point left out at its start')
    p.add_argument('-sd', '--stride', type=int, default=1, help='every STRIDE-th sample is clustered')
    p.add_argument('-il', '--inliers', action='store_true',
                   help="cluster only the inliers of `outlier` (<PREFIX>.F.lof.npy and .F.loi.npy of the same -sk and -sd); its outliers get label -1")
    p.add_argument('-dv', '--device', type=int, default=0)
    a = p.parse_args(argv)
    if (a.skip < 0 or a.stride < 1 or not 1 <= a.dimensions <= MAX_DIM or not 1 <= a.clusters_kept <= MAX_KEPT or a.min_samples < 1
            or not (np.isfinite(a.neighbourhood) and a.neighbourhood > 0.0)):
        p.error('need -sk >= 0, -sd >= 1, -nd in 1..16, -nk in 1..8, -ms >= 1 and a finite -nc > 0')
    return a


def dbscan(x, eps, min_pts, device=0):
    """nm_cluster_dbscan of x (N, ND): (label (N,) int32, degree (N,) int32, nclusters)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError('x wants the shape (N, ND)')
    n, nd = x.shape
    label, degree, ncl = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32), np.zeros(1, dtype=np.int32)
    B.call('nm_cluster_dbscan', device, n, nd, x, float(eps), int(min_pts), label, degree, ncl)
    return label, degree, int(ncl[0])


def scaled(z):
    """z (N, ND) divided by the range of its component 0; ValueError where that range is 0"""
    z = np.asarray(z, dtype=np.float64)
    s = float(z[:, 0].max() - z[:, 0].min())
    if not s > 0.0:
        raise ValueError('component 0 is %g in every clustered sample, -nc has no unit' % z[0, 0])
    return z / s


def table(label, degree, min_pts, temp, z):
    """the cluster table (K, 3 + ND) of labelled points: members, core members, the members' mean target temperature, their centroid
    in the projections z (N, ND) as they are; K is the largest label + 1"""
    label, z = np.asarray(label), np.asarray(z, dtype=np.float64)
    k = int(label.max()) + 1 if label.size else 0
    out = np.zeros((max(k, 0), 3 + z.shape[1]))
    core = np.asarray(degree) >= min_pts
    for c in range(k):
        m = label == c
        out[c, 0], out[c, 1] = m.sum(), (m & core).sum()
        out[c, 2] = np.asarray(temp, dtype=np.float64)[m].mean()
        out[c, 3:] = z[m].mean(axis=0)
    return out


def phases(tab, nk):
    """the labels behind cl0, cl1, ...: the nk largest clusters of the table by members (the smaller label wins a tie), ordered from
    the lowest mean target temperature to the highest (the smaller label first where they are equal); fewer where there are fewer"""
    largest = sorted(range(tab.shape[0]), key=lambda c: (-tab[c, 0], c))[:nk]
    return sorted(largest, key=lambda c: (tab[c, 2], c))


def main(argv=None):
    a = parse_args(argv)
    el, ft, nd = a.element, a.feature, a.dimensions
    prefix = S.prefix(a.name, el)
    P, T, pe, pcz, path = S.grid_inputs('cluster', prefix, ft + '.' + a.embedding, 'the components')
    pn, tn, sn, ld = pcz.shape
    if nd > ld:
        raise SystemExit('cluster: -nd %d is more than the %d components of %s' % (nd, ld, path))
    kept, zk = S.kept(pcz, a.skip, a.stride)
    keep = S.inliers('cluster', prefix, ft, pe.shape, a.skip, a.stride) if a.inliers else np.ones((pn, tn, kept), dtype=bool)
    n = int(keep.sum())
    if not 1 <= n <= MAX_POINTS:
        raise SystemExit('cluster: -sk %d -sd %d%s leave %d samples of %s, not 1..%d' % (a.skip, a.stride, ' -il' if a.inliers else '', n, path,
                                                                                       MAX_POINTS))
    z = np.ascontiguousarray(zk[..., :nd], dtype=np.float64)[keep]
    if a.embedding == 'mfy':                                         # manifold left out what this run leaves out, NaN there and nowhere else
        out = np.ones(sn, dtype=bool)
        out[a.skip::a.stride] = False
        if np.isnan(z).any() or not np.isnan(pcz[:, :, out]).all() or not np.isnan(zk[~keep]).all():
            raise SystemExit('cluster: -sk %d -sd %d%s are not those that %s was written with' % (a.skip, a.stride, ' -il' if a.inliers else '', path))
    temp = np.broadcast_to(np.asarray(T, dtype=np.float64)[None, :, None], (pn, tn, kept))[keep]
    if a.verbose:
        print('clustering %d of %d samples of %s in %d components, eps %g of the range of pc0, min_pts %d' % (
            n, pn * tn * sn, ft, nd, a.neighbourhood, a.min_samples))
    try:
        label, degree, ncl = dbscan(scaled(z), a.neighbourhood, a.min_samples, a.device)
    except (RuntimeError, ValueError) as err:
        raise SystemExit('cluster: %s: %s' % (path, err))
    tab = table(label, degree, a.min_samples, temp, z)
    order = phases(tab, a.clusters_kept)
    full = S.spread_kept(label, keep, pe.shape, a.skip, a.stride, -1)
    np.save(prefix + '.%s.cll.npy' % ft, full)
    np.save(prefix + '.%s.cld.npy' % ft, S.spread_kept(degree, keep, pe.shape, a.skip, a.stride, 0))
    np.save(prefix + '.%s.cls.npy' % ft, tab)
    for k in range(a.clusters_kept):
        np.save(prefix + '.%s.cl%d.npy' % (ft, k), (full == order[k]).astype(np.float64) if k < len(order) else np.zeros(pe.shape))
    if a.verbose:
        print('%d clusters, %d samples are noise; degree %d .. %d, median %d' % (ncl, int((label < 0).sum()), degree.min(), degree.max(),
                                                                              int(np.median(degree))))
        for k, c in enumerate(order):
            print('cl%d: cluster %d, %d members (%d core), mean target temperature %.6g' % (k, c, tab[c, 0], tab[c, 1], tab[c, 2]))
        if len(order) < a.clusters_kept:
            print('only %d clusters: cl%d .. cl%d are all zero' % (len(order), len(order), a.clusters_kept - 1))
    return 0


if __name__ == '__main__':
    sys.exit(main())
