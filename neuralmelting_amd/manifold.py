"""The manifold between pca and cluster: exact t-SNE of the principal components' projections over the whole replica grid
(include/nm_tsne.h).  lammps_vae.py embeds its projections with sklearn's TSNE (its default -mf) before it
clusters them; this stage does so in the HIP library (nm_tsne_affinities, nm_tsne_descend: all-pairs scans, no tree and no angle
parameter, there is no host fallback) and writes the embedding for `cluster -em mfy`:

    python -m neuralmelting_amd.pca -v -n remcmc_run_5 -e LJ -sk 128
    python -m neuralmelting_amd.manifold -v -n remcmc_run_5 -e LJ -sk 128
    python -m neuralmelting_amd.cluster -v -n remcmc_run_5 -e LJ -sk 128 -em mfy -nc 0.02

The schedule is sklearn's: k = min(N - 1, int(3 PX + 1)) neighbours, the start the first NC input components divided by the
standard deviation of component 0 and multiplied by 1e-4 (init='pca'), XI steps at exaggeration EX with momentum 0.5, the rest of
the NI steps at exaggeration 1 with momentum 0.8.  There is no random number anywhere: two runs write the same bytes.
"""
import argparse
import sys

import numpy as np

from . import _lib as B
from . import _stage as S

MAX_POINTS, MAX_DIM, MAX_COMP, MAX_K = 2 ** 20, 16, 3, 4096     # include/nm_tsne.h


def parse_args(argv=None):
    p = argparse.ArgumentParser(
        description='t-SNE of the projections .F.pcz of pca over the (P, T) grid: .F.mfy (PN, TN, SN, NC) float64 the embedding, NaN for '
        'samples left out; .F.mfb (PN, TN, SN) float64 the beta of each sample (NaN likewise); .F.mft (NI, 3) float64 per step: the '
        'Kullback-Leibler divergence, Z and the norm of the gradient.')
    p.add_argument('-v', '--verbose', action='store_true')
    p.add_argument('-n', '--name', type=str, default='remcmc_init')
    p.add_argument('-e', '--element', type=str, default='LJ')
    p.add_argument('-ft', '--feature', type=str, default='cdf', help='the feature F whose projections <PREFIX>.F.pcz.npy are embedded')
    p.add_argument('-nd', '--dimensions', type=int, default=None, help='leading input components used, 1..16 and at most LD (default: all)')
    p.add_argument('-px', '--perplexity', type=float, default=None, help='default: the kept samples of a grid point')
    p.add_argument('-ex', '--exaggeration', type=float, default=24.0)
    p.add_argument('-lr', '--learning_rate', type=float, default=200.0)
    p.add_argument('-ni', '--iterations', type=int, default=1000)
    p.add_argument('-xi', '--exaggerated', type=int, default=250, help='the first XI iterations run under the exaggeration')
    p.add_argument('-nc', '--components', type=int, default=2, help='output components, 1..3 and at most ND')
    p.add_argument('-sk', '--skip', type=int, default=0, help='samples of every grid point left out at its start')
    p.add_argument('-sd', '--stride', type=int, default=1, help='every STRIDE-th sample is embedded')
    p.add_argument('-il', '--inliers', action='store_true',
                   help="embed only the inliers of `outlier` (<PREFIX>.F.lof.npy and .F.loi.npy of the same -sk and -sd); NaN for its outliers")
    p.add_argument('-dv', '--device', type=int, default=0)
    a = p.parse_args(argv)
    if (a.skip < 0 or a.stride < 1 or (a.dimensions is not None and not 1 <= a.dimensions <= MAX_DIM) or not 1 <= a.components <= MAX_COMP
            or (a.perplexity is not None and not (np.isfinite(a.perplexity) and a.perplexity > 1.0))
            or not (np.isfinite(a.exaggeration) and a.exaggeration > 0.0) or not (np.isfinite(a.learning_rate) and a.learning_rate > 0.0)
            or a.iterations < 1 or not 0 <= a.exaggerated <= a.iterations):
        p.error('need -sk >= 0, -sd >= 1, -nd in 1..16, -nc in 1..3, a finite -px > 1, finite -ex > 0 and -lr > 0, -ni >= 1 and -xi in 0..NI')
    return a


def affinities(x, perplexity, k, device=0):
    """nm_tsne_affinities of x (N, ND): (nbr (N, k) int32, p (N, k), beta (N,))"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError('x wants the shape (N, ND)')
    n, nd = x.shape
    nbr, p, beta = np.empty((n, max(k, 0)), dtype=np.int32), np.empty((n, max(k, 0))), np.empty(n)
    B.call('nm_tsne_affinities', device, n, nd, x, float(perplexity), int(k), nbr, p, beta)
    return nbr, p, beta


def _lists(nbr, p):
    nbr, p = np.ascontiguousarray(nbr, dtype=np.int32), np.ascontiguousarray(p, dtype=np.float64)
    if nbr.ndim != 2 or nbr.shape != p.shape:
        raise ValueError('nbr and p want one shape (N, k)')
    return nbr, p


def gradient(nbr, p, y, exaggeration=1.0, device=0):
    """nm_tsne_gradient: (grad (N, NC), kl, Z)"""
    nbr, p = _lists(nbr, p)
    y = np.ascontiguousarray(y, dtype=np.float64)
    if y.ndim != 2 or y.shape[0] != nbr.shape[0]:
        raise ValueError('y wants the shape (N, NC)')
    grad, kl, z = np.empty_like(y), np.empty(1), np.empty(1)
    B.call('nm_tsne_gradient', device, nbr.shape[0], nbr.shape[1], nbr, p, y.shape[1], y, float(exaggeration), grad, kl, z)
    return grad, float(kl[0]), float(z[0])


def descend(nbr, p, y, update, gains, niter, exaggeration, momentum, learning_rate, device=0):
    """nm_tsne_descend on y, update and gains (N, NC), float64 and C-contiguous, in place: the trace (niter, 3)"""
    nbr, p = _lists(nbr, p)
    for a in (y, update, gains):
        if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.flags.writeable and a.ndim == 2
                and a.shape == y.shape and a.shape[0] == nbr.shape[0]):
            raise ValueError('y, update and gains want one shape (N, NC), float64, C-contiguous and writeable')
    trace = np.empty((max(niter, 0), 3))
    B.call('nm_tsne_descend', device, nbr.shape[0], nbr.shape[1], nbr, p, y.shape[1], y, update, gains, int(niter), float(exaggeration),
           float(momentum), float(learning_rate), trace)
    return trace


def neighbours(n, perplexity):
    """sklearn's number of neighbours"""
    return min(n - 1, int(3.0 * perplexity + 1))


def start(x, nc):
    """sklearn's init='pca' on projections that are principal components already: the first nc of them divided by the standard
    deviation of component 0, times 1e-4; ValueError where that deviation is 0"""
    x = np.asarray(x, dtype=np.float64)
    s = float(np.std(x[:, 0]))
    if not s > 0.0:
        raise ValueError('component 0 is %g in every embedded sample, the start has no scale' % x[0, 0])
    return np.ascontiguousarray(x[:, :nc] / s * 1e-4)


def embed(x, nc, perplexity, exaggeration, learning_rate, niter, nexag, device=0):
    """the whole schedule on x (N, ND): (y (N, nc), beta (N,), trace (niter, 3))"""
    n = x.shape[0]
    nbr, p, beta = affinities(x, perplexity, neighbours(n, perplexity), device)
    y = start(x, nc)
    update, gains = np.zeros_like(y), np.ones_like(y)
    trace = [np.empty((0, 3))]
    if nexag:
        trace.append(descend(nbr, p, y, update, gains, nexag, exaggeration, 0.5, learning_rate, device))
    if niter > nexag:
        trace.append(descend(nbr, p, y, update, gains, niter - nexag, 1.0, 0.8, learning_rate, device))
    return y, beta, np.concatenate(trace)


def spread(values, shape, skip, stride):
    """values (PN, TN, kept, ...) of the embedded samples skip, skip + stride, ... in a float64 array of `shape` filled with NaN"""
    return S.spread(np.asarray(values, dtype=np.float64), shape, skip, stride, np.nan)


def main(argv=None):
    a = parse_args(argv)
    el, ft, nc = a.element, a.feature, a.components
    prefix = S.prefix(a.name, el)
    P, T, pe, pcz, path = S.grid_inputs('manifold', prefix, ft + '.pcz', 'the components')
    pn, tn, sn, ld = pcz.shape
    nd = ld if a.dimensions is None else a.dimensions
    if nd > ld or nd > MAX_DIM:
        raise SystemExit('manifold: -nd %d is more than the %d components of %s or than %d' % (nd, ld, path, MAX_DIM))
    if nc > nd:
        raise SystemExit('manifold: -nc %d is more than the %d input components' % (nc, nd))
    kept, xk = S.kept(pcz, a.skip, a.stride)
    keep = S.inliers('manifold', prefix, ft, pe.shape, a.skip, a.stride) if a.inliers else np.ones((pn, tn, kept), dtype=bool)
    n = int(keep.sum())
    if not 3 <= n <= MAX_POINTS:
        raise SystemExit('manifold: -sk %d -sd %d%s leave %d samples of %s, not 3..%d' % (a.skip, a.stride, ' -il' if a.inliers else '', n, path,
                                                                                        MAX_POINTS))
    px = float(kept) if a.perplexity is None else a.perplexity
    k = neighbours(n, px)
    if not (1.0 < px < k <= MAX_K):
        raise SystemExit('manifold: the perplexity %g wants %d neighbours of %d samples: need 1 < PX < k <= %d' % (px, k, n, MAX_K))
    x = np.ascontiguousarray(xk[..., :nd], dtype=np.float64)[keep]
    if a.verbose:
        print('embedding %d of %d samples of %s from %d to %d components, perplexity %g, %d neighbours, %d steps (%d at exaggeration %g)' % (
            n, pn * tn * sn, ft, nd, nc, px, k, a.iterations, a.exaggerated, a.exaggeration))
    try:
        y, beta, trace = embed(x, nc, px, a.exaggeration, a.learning_rate, a.iterations, a.exaggerated, a.device)
    except (RuntimeError, ValueError) as err:
        raise SystemExit('manifold: %s: %s' % (path, err))
    np.save(prefix + '.%s.mfy.npy' % ft, S.spread_kept(y, keep, pe.shape + (nc,), a.skip, a.stride, np.nan))
    np.save(prefix + '.%s.mfb.npy' % ft, S.spread_kept(beta, keep, pe.shape, a.skip, a.stride, np.nan))
    np.save(prefix + '.%s.mft.npy' % ft, trace)
    if a.verbose:
        print('kl %.6g at the start, %.6g before step %d; beta %.4g .. %.4g; the embedding spans %s' % (
            trace[0, 0], trace[-1, 0], a.iterations, beta.min(), beta.max(), np.ptp(y, axis=0)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
