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

-cl kmeans is the reference's other clustering, for a grid whose number of phases is known: -nc is then the number of clusters and
nothing is tuned.  The restarts (-ri, seeded on the host by k-means++ from -rs) run as one batch in the library (nm_cluster_kmeans),
the restart with the smallest inertia gives the labels, and `.F.clr.npy` says how every restart ended:

    python -m neuralmelting_amd.cluster -v -n remcmc_run_5 -e LJ -sk 128 -cl kmeans -nc 2

-cl spectral is for what centroids cannot cut: two curved, elongated branches joined by a thin bridge of coexistence samples.  -nc is
again the number of clusters.  The library (nm_cluster_spectral) finds the -nc leading eigenvectors of the normalised Gaussian affinity
of the scaled points by a Chebyshev-filtered subspace iteration, every application of the affinity one pass over all pairs with no
N x N array; the embedding then goes through the same seeds and the same k-means.  `.F.clg.npy`, the degree of every sample, is the
data to judge the width -gm from, `.F.cle.npy` says how the eigensolver ended:

    python -m neuralmelting_amd.cluster -v -n remcmc_run_5 -e LJ -sk 128 -cl spectral -nc 2
"""
import argparse
import sys

import numpy as np

from . import _lib as B
from . import _stage as S
from ._stage import spread

MAX_POINTS, MAX_DIM, MAX_KEPT = 2 ** 21, 16, 8     # include/nm_cluster.h: npoints and ndim; the indicators of -nk
MAX_K, MAX_RESTARTS, MAX_CENTRES, MAX_ITER = 256, 64, 4096, 10000      # include/nm_distr.h, nm_cluster_kmeans: k, nrestarts, their product, max_iter
SP_MAX_POINTS, SP_MAX_K, SP_MAX_BLOCK, SP_MAX_DEGREE, SP_MAX_PASS = 2 ** 20, 8, 16, 64, 100000     # nm_cluster_spectral: npoints, ncomp, nblock, degree, max_pass


def parse_args(argv=None):
    p = argparse.ArgumentParser(
        description='DBSCAN of the projections .F.pcz of pca over the (P, T) grid: .F.cll (PN, TN, SN) int32 the labels, -1 for noise and for '
        'samples left out; .F.cld (PN, TN, SN) int32 the samples within EPS, the sample among them; .F.cls (K, 3 + ND) float64 per '
        'cluster: members, core members, mean target temperature, centroid in the projections; .F.cl0 ... (PN, TN, SN) float64 the '
        'membership indicators of the NK largest clusters from the coldest to the hottest, for reweight -ob F.cl1 -hq F.cl1 -hx 0.5.  '
        'With -cl kmeans: .F.cll the labels of the best restart, .F.cls with core members = members, .F.cl0 ... as above, .F.clr (R, 3) '
        'float64 the inertia, the iterations and the status (0 a fixed point, 1 within -tl, 2 stopped at -mi) of every restart; '
        '.F.cld is not written.  With -cl spectral: the files of -cl kmeans from k-means of the spectral embedding, and .F.cle (NB, 2) '
        'float64 the Ritz values of the block and their residuals, .F.clv (PN, TN, SN, K) float64 the embedding and .F.clg (PN, TN, SN) '
        'float64 the degree, both NaN for samples left out.')
    p.add_argument('-v', '--verbose', action='store_true')
    p.add_argument('-n', '--name', type=str, default='remcmc_init')
    p.add_argument('-e', '--element', type=str, default='LJ')
    p.add_argument('-ft', '--feature', type=str, default='cdf', help='the feature F whose projections <PREFIX>.F.pcz.npy are clustered')
    p.add_argument('-em', '--embedding', type=str, default='pcz', choices=('pcz', 'mfy'),
                   help="what is clustered: pca's projections <PREFIX>.F.pcz.npy, or manifold's embedding <PREFIX>.F.mfy.npy of the same -sk and -sd")
    p.add_argument('-nd', '--dimensions', type=int, default=2, help='leading components used, 1..16 and at most LD')
    p.add_argument('-cl', '--clustering', type=str, default='dbscan', choices=('dbscan', 'kmeans', 'spectral'))
    p.add_argument('-nc', '--neighbourhood', type=float, required=True, metavar='EPS',
                   help='the radius of a neighbourhood as a fraction of the range of component 0; with -cl kmeans the number of clusters, 1..256, with -cl spectral 2..8')
    p.add_argument('-ms', '--min_samples', type=int, default=5,
                   help='samples within EPS, itself among them, that make a sample a core; ignored with -cl kmeans')
    p.add_argument('-ri', '--restarts', type=int, default=10, help='-cl kmeans: restarts from k-means++ seeds, 1..64; the best is kept')
    p.add_argument('-mi', '--max_iter', type=int, default=300, help='-cl kmeans: steps of a restart at most, 1..10000')
    p.add_argument('-tl', '--tolerance', type=float, default=1e-4,
                   help="-cl kmeans: a restart stops where its centres' squared shift is at most TL times the mean variance of the used components")
    p.add_argument('-rs', '--seed', type=int, default=256, help='-cl kmeans: the seed of the k-means++ draws')
    p.add_argument('-gm', '--gamma', type=float, default=1.0,
                   help="-cl spectral: the width of the affinity exp(-gamma d^2), in the unit 1 / (the sum of the used scaled components' variances "
                   "over the clustered points): the library's gamma is GM divided by that sum")
    p.add_argument('-eb', '--eigen_block', type=int, default=16,
                   help='-cl spectral: columns of the iterated block, -nc..16; fewer where fewer samples are clustered')
    p.add_argument('-ed', '--eigen_degree', type=int, default=8, help='-cl spectral: the degree of the Chebyshev filter, 1..64')
    p.add_argument('-et', '--eigen_tolerance', type=float, default=1e-6,
                   help='-cl spectral: the largest residual of the -nc leading Ritz pairs at which the eigensolver stops')
    p.add_argument('-ei', '--eigen_passes', type=int, default=2000, help='-cl spectral: passes over all pairs at most, 1..100000')
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
    if a.clustering == 'spectral':
        if a.neighbourhood != int(a.neighbourhood) or not 2 <= a.neighbourhood <= SP_MAX_K:
            p.error('with -cl spectral -nc is the number of clusters: an integer in 2..8')
        if (not (np.isfinite(a.gamma) and a.gamma > 0.0) or not a.neighbourhood <= a.eigen_block <= SP_MAX_BLOCK
                or not 1 <= a.eigen_degree <= SP_MAX_DEGREE or not (np.isfinite(a.eigen_tolerance) and a.eigen_tolerance >= 0.0)
                or not 1 <= a.eigen_passes <= SP_MAX_PASS):
            p.error('need a finite -gm > 0, -eb in -nc..16, -ed in 1..64, a finite -et >= 0 and -ei in 1..100000')
    if a.clustering in ('kmeans', 'spectral'):
        if a.neighbourhood != int(a.neighbourhood) or not 1 <= a.neighbourhood <= MAX_K:
            p.error('with -cl kmeans -nc is the number of clusters: an integer in 1..256')
        if (not 1 <= a.restarts <= MAX_RESTARTS or int(a.neighbourhood) * a.restarts > MAX_CENTRES or not 1 <= a.max_iter <= MAX_ITER
                or not (np.isfinite(a.tolerance) and a.tolerance >= 0.0) or a.seed < 0):
            p.error('need -ri in 1..64 with -nc * -ri <= 4096, -mi in 1..10000, a finite -tl >= 0 and -rs >= 0')
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


def kmeans(x, init, max_iter=300, tol=0.0, device=0):
    """nm_cluster_kmeans of x (N, ND) from the initial centres init (R, K, ND): (label (N,) int32, centre (K, ND), count (K,) int32 of
    the best restart; inertia (R,), iters (R,) int32, status (R,) int32 of every restart; best)"""
    x, init = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(init, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError('x wants the shape (N, ND)')
    if init.ndim != 3 or init.shape[2] != x.shape[1]:
        raise ValueError('init wants the shape (R, K, ND)')
    (n, nd), (r, k) = x.shape, init.shape[:2]
    label, centre, count = np.empty(n, dtype=np.int32), np.empty((k, nd)), np.empty(k, dtype=np.int32)
    inertia, iters, status, best = np.empty(r), np.empty(r, dtype=np.int32), np.empty(r, dtype=np.int32), np.zeros(1, dtype=np.int32)
    B.call('nm_cluster_kmeans', device, n, nd, x, k, r, init, int(max_iter), float(tol), label, centre, count, inertia, iters, status, best)
    return label, centre, count, inertia, iters, status, int(best[0])


def spectral(x, gamma, ncomp, init, degree=8, max_pass=2000, tol=1e-6, device=0):
    """nm_cluster_spectral of x (N, ND) from the start block init (N, NB): (embed (N, ncomp), eigval (NB,), resid (NB,), deg (N,), the
    passes done, the status: 0 within tol, 2 stopped at max_pass)"""
    x, init = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(init, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError('x wants the shape (N, ND)')
    if init.ndim != 2 or init.shape[0] != x.shape[0]:
        raise ValueError('init wants the shape (N, NB)')
    (n, nd), nb = x.shape, init.shape[1]
    embed, eigval, resid, deg, info = np.empty((n, max(int(ncomp), 0))), np.empty(nb), np.empty(nb), np.empty(n), np.zeros(2, dtype=np.int32)
    B.call('nm_cluster_spectral', device, n, nd, x, float(gamma), int(ncomp), nb, init, int(degree), int(max_pass), float(tol), embed, eigval,
           resid, deg, info)
    return embed, eigval, resid, deg, int(info[0]), int(info[1])


def seeds(x, k, nrestarts, seed):
    """k-means++ on the host, (R, K, ND): the first centre of a restart is a point drawn uniformly, every further one a point drawn
    with a probability proportional to its squared distance from the nearest centre so far (a point that is a centre already has
    none), so a restart's centres are k distinct points of x; numpy.random.default_rng(seed), restart after restart.  ValueError
    where x has fewer than k distinct points."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError('x wants the shape (N, ND)')
    rng = np.random.default_rng(seed)
    out = np.empty((nrestarts, k, x.shape[1]))
    for r in range(nrestarts):
        i = int(rng.integers(x.shape[0]))
        near = np.full(x.shape[0], np.inf)
        for j in range(k):
            if j:
                if not near.max() > 0.0:
                    raise ValueError('x has only %d distinct points, fewer than the %d clusters' % (j, k))
                i = int(rng.choice(x.shape[0], p=near / near.sum()))
            out[r, j] = x[i]
            near = np.minimum(near, ((x - x[i]) ** 2).sum(axis=1))
    return out


def kmeans_table(label, count, temp, z):
    """the cluster table (K, 3 + ND) of k-means labels: `table` with every member a core member; a cluster without members is a row
    of zeros"""
    out = np.zeros((len(count), 3 + z.shape[1]))
    for c in np.nonzero(count)[0]:
        out[c] = table(np.where(label == c, 0, -1), np.ones(len(label), dtype=np.int32), 1, temp, z)[0]
    return out


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
    if a.clustering == 'kmeans':
        return main_kmeans(a, prefix, path, pe.shape, keep, z, temp)
    if a.clustering == 'spectral':
        return main_spectral(a, prefix, path, pe.shape, keep, z, temp)
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


def main_kmeans(a, prefix, path, shape, keep, z, temp, embedded=None):
    """-cl kmeans of the clustered points z (N, ND) with their target temperatures: the files of the best of -ri restarts.
    embedded: a function of the scaled points that gives what k-means clusters in their place, and the generator of its seeds"""
    ft, k, n = a.feature, int(a.neighbourhood), z.shape[0]
    if k > n:
        raise SystemExit('cluster: -nc %d clusters are more than the %d samples of %s' % (k, n, path))
    try:
        zs, rng = scaled(z), a.seed
        if embedded:
            zs, rng = embedded(zs)
        tol = a.tolerance * float(zs.var(axis=0).mean())
        if a.verbose:
            print('clustering %d samples of %s in %d components into %d clusters: %d restarts, max_iter %d, tol %g' % (
                n, ft, zs.shape[1], k, a.restarts, a.max_iter, tol))
        label, centre, count, inertia, iters, status, best = kmeans(zs, seeds(zs, k, a.restarts, rng), a.max_iter, tol, a.device)
    except (RuntimeError, ValueError) as err:
        raise SystemExit('cluster: %s: %s' % (path, err))
    tab = kmeans_table(label, count, temp, z)
    order = [c for c in phases(tab, a.clusters_kept) if count[c]]
    full = S.spread_kept(label, keep, shape, a.skip, a.stride, -1)
    np.save(prefix + '.%s.cll.npy' % ft, full)
    np.save(prefix + '.%s.cls.npy' % ft, tab)
    np.save(prefix + '.%s.clr.npy' % ft, np.stack([inertia, iters.astype(np.float64), status.astype(np.float64)], axis=1))
    for c in range(a.clusters_kept):
        np.save(prefix + '.%s.cl%d.npy' % (ft, c), (full == order[c]).astype(np.float64) if c < len(order) else np.zeros(shape))
    if a.verbose:
        print('best restart %d of %d: inertia %.9g after %d steps, status %d; the inertias lie in %.9g .. %.9g' % (
            best, a.restarts, inertia[best], iters[best], status[best], inertia.min(), inertia.max()))
        if status[best] == 2:
            print('warning: the best restart stopped at -mi %d before its centres came to rest' % a.max_iter)
        if count.min() == 0:
            print('warning: %d clusters of the best restart have no member' % int((count == 0).sum()))
        for c, j in enumerate(order):
            print('cl%d: cluster %d, %d members, mean target temperature %.6g' % (c, j, tab[j, 0], tab[j, 2]))
        if len(order) < a.clusters_kept:
            print('only %d clusters: cl%d .. cl%d are all zero' % (len(order), len(order), a.clusters_kept - 1))
    return 0


def main_spectral(a, prefix, path, shape, keep, z, temp):
    """-cl spectral: the spectral embedding of the scaled points, its files, then main_kmeans on the embedding.  The start block is
    drawn first and the k-means++ seeds behind it, from one generator numpy.random.default_rng(-rs)."""
    ft, k, n = a.feature, int(a.neighbourhood), z.shape[0]
    if not k <= n <= SP_MAX_POINTS:
        raise SystemExit('cluster: -cl spectral wants %d..%d samples, %s leaves %d' % (k, SP_MAX_POINTS, path, n))

    def embedded(zs):
        rng = np.random.default_rng(a.seed)
        nb = min(a.eigen_block, n)
        gamma = a.gamma / float(zs.var(axis=0).sum())
        if not np.isfinite(gamma):
            raise ValueError('the used components do not vary, -gm has no unit')
        if a.verbose:
            print('spectral embedding of %d samples of %s in %d components: gamma %g, block %d, filter degree %d, tol %g' % (
                n, ft, zs.shape[1], gamma, nb, a.eigen_degree, a.eigen_tolerance))
        embed, eigval, resid, deg, passes, status = spectral(zs, gamma, k, rng.standard_normal((n, nb)), a.eigen_degree, a.eigen_passes,
                                                             a.eigen_tolerance, a.device)
        np.save(prefix + '.%s.cle.npy' % ft, np.stack([eigval, resid], axis=1))
        np.save(prefix + '.%s.clv.npy' % ft, S.spread_kept(embed, keep, shape + (k,), a.skip, a.stride, np.nan))
        np.save(prefix + '.%s.clg.npy' % ft, S.spread_kept(deg, keep, shape, a.skip, a.stride, np.nan))
        if a.verbose:
            print('eigenvalues %s after %d passes, residuals at most %.3g; the gap behind the %d-th is %s; degree %.4g .. %.4g, median %.4g' % (
                ' '.join('%.6f' % v for v in eigval[:k]), passes, resid[:k].max(), k, '%.3g' % (eigval[k - 1] - eigval[k]) if nb > k else 'not known (-eb = -nc)',
                deg.min(), deg.max(), float(np.median(deg))))
            if status == 2:
                print('warning: the eigensolver stopped at -ei %d passes before its residuals came to -et %g' % (a.eigen_passes, a.eigen_tolerance))
        return embed, rng

    return main_kmeans(a, prefix, path, shape, keep, z, temp, embedded)


if __name__ == '__main__':
    sys.exit(main())
