"""Principal components of the structural histograms over the whole replica grid (include/nm_pca.h):
the linear form of the reference's last stage.  lammps_vae.py scales distr's histograms, embeds them with a VAE and applies
PCA to the latents; this stage scales them the same way (-sc), diagonalises their covariance over all kept samples of the
grid, and projects every sample on the leading components.  The moments and the projections run in the HIP library
(nm_pca_moments: the covariance on the float64 matrix instruction; nm_pca_project), there is no host fallback; the D x D
eigenproblem (D <= 4096) is numpy's on the host.

The projections are per-sample observables of `.pe.npy`'s shape, so the reweighting stage takes them like any order parameter:

    python -m neuralmelting_amd.distr -v -n remcmc_run_5 -e LJ -cb 11
    python -m neuralmelting_amd.pca -v -n remcmc_run_5 -e LJ -sk 128
    python -m neuralmelting_amd.reweight -v -n remcmc_run_5 -e LJ -sk 128 -ob cdf.pc0 -hq cdf.pc0 -hx 0.0 -bs 200

Scalers: the features are divided by s_j before the covariance is taken, algebraically: cov[i][j] = gram[i][j] / (s_i s_j (N - 1)).
none: s = 1.  global (the reference's default): one s = max - min over all features.  standard: s_j = the population standard
deviation (sklearn's StandardScaler), 1 for a constant feature.  minmax: s_j = max_j - min_j, 1 for a constant feature.
Each component's sign is fixed so that its mean over the hottest temperature column is not below that over the coldest one.
"""
import argparse
import sys

import numpy as np

from . import _lib as B
from . import _stage as S

SCALERS = ('none', 'global', 'standard', 'minmax')
MAX_FEAT, MAX_COMP = 4096, 64       # include/nm_pca.h: nfeat and ncomp
SUFFIXES = ('pcm', 'pcs', 'pcc', 'pcv', 'pcz', 'pcr')


def parse_args(argv=None):
    p = argparse.ArgumentParser(
        description='PCA of a feature F of distr over the (P, T) grid, all float64: .F.pcm (D,) the mean; .F.pcs (D,) the scale s; .F.pcc '
        '(LD, D) the components; .F.pcv (2, LD) their eigenvalues and shares of the trace; .F.pcz (PN, TN, SN, LD) the projections of '
        'every sample; .F.pcr (PN, TN, SN) the squared reconstruction error; .F.pc0 ... (PN, TN, SN) one component each, for '
        'reweight -ob F.pc0 -hq F.pc0.')
    p.add_argument('-v', '--verbose', action='store_true')
    p.add_argument('-n', '--name', type=str, default='remcmc_init')
    p.add_argument('-e', '--element', type=str, default='LJ')
    p.add_argument('-ft', '--feature', type=str, default='cdf',
                   help='<PREFIX>.FEATURE.npy of shape (PN, TN, SN, ...): the trailing axes are the D features of a sample')
    p.add_argument('-sc', '--scaler', type=str, default='global', choices=SCALERS)
    p.add_argument('-ld', '--latent_dimension', type=int, default=8, help='components kept, 1..64 and at most D')
    p.add_argument('-sk', '--skip', type=int, default=0, help='samples of every grid point left out of the FIT at its start')
    p.add_argument('-sd', '--stride', type=int, default=1, help='the fit uses every STRIDE-th sample; all samples are projected')
    p.add_argument('-dv', '--device', type=int, default=0)
    a = p.parse_args(argv)
    if a.skip < 0 or a.stride < 1 or not 1 <= a.latent_dimension <= MAX_COMP:
        p.error('need -sk >= 0, -sd >= 1 and -ld in 1..64')
    return a


def _f64(x):
    return np.ascontiguousarray(x, dtype=np.float64)


def moments(x, device=0):
    """nm_pca_moments of x (N, D) float32: (mean (D,), lo (D,), hi (D,), gram (D, D))"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError('x wants the shape (N, D)')
    n, d = x.shape
    mean, lo, hi, gram = np.empty(d), np.empty(d), np.empty(d), np.empty((d, d))
    B.call('nm_pca_moments', device, n, d, x, mean, lo, hi, gram)
    return mean, lo, hi, gram


def project(x, mean, inv_scale, comp, device=0):
    """nm_pca_project of x (N, D) float32 on comp (C, D): (z (N, C), norm2 (N,))"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    mean, inv_scale, comp = _f64(mean), _f64(inv_scale), np.atleast_2d(_f64(comp))
    if x.ndim != 2 or mean.shape != (x.shape[1],) or inv_scale.shape != mean.shape or comp.shape[1] != x.shape[1]:
        raise ValueError('x wants the shape (N, D), mean and inv_scale (D,), comp (C, D)')
    n, d = x.shape
    z, norm2 = np.empty((n, comp.shape[0])), np.empty(n)
    B.call('nm_pca_project', device, n, d, x, mean, inv_scale, comp.shape[0], comp, z, norm2)
    return z, norm2


def scales(scaler, lo, hi, gram, n):
    """s (D,) of a scaler from the moments of n samples; ValueError for `global` on data without any spread"""
    d = lo.size
    if scaler == 'none':
        return np.ones(d)
    if scaler == 'global':
        s = float(hi.max() - lo.min())
        if not s > 0.0:
            raise ValueError('-sc global: every value of the feature is %g, there is nothing to scale' % lo.min())
        return np.full(d, s)
    s = np.sqrt(np.diag(gram) / n) if scaler == 'standard' else hi - lo
    return np.where(s > 0.0, s, 1.0)


def fit(lo, hi, gram, n, scaler, ld):
    """the host half of the fit, from nm_pca_moments' results for n samples: (s (D,), comp (ld, D), pcv (2, ld)).  The covariance
    gram / (s_i s_j (n - 1)) is diagonalised by numpy.linalg.eigh; the eigenvalues are sorted descending (eigh's order reversed)
    and clipped at 0, comp holds the unit eigenvectors of the ld largest, pcv their eigenvalues and shares of the clipped trace
    (0 where the trace is 0).  The signs are eigh's: orient() fixes them."""
    lo, hi, gram = _f64(lo), _f64(hi), _f64(gram)
    s = scales(scaler, lo, hi, gram, n)
    cov = gram / (s[:, None] * s[None, :] * (n - 1.0))
    w, v = np.linalg.eigh(cov)
    w, v = np.maximum(w[::-1], 0.0), v[:, ::-1]
    total = w.sum()
    share = w[:ld] / total if total > 0.0 else np.zeros(ld)
    return s, np.ascontiguousarray(v[:, :ld].T), np.stack([w[:ld], share])


def orient(comp, hot, cold):
    """the sign (ld,) of +-1 that every component (and its projections) is multiplied with: hot and cold (ld,) are the projections'
    means over the hottest and the coldest temperature column; the hot one is to be the larger.  Where they are equal the
    component's entry of largest magnitude (the first of equals) is made positive."""
    sign = np.where(hot >= cold, 1.0, -1.0)
    for c in np.nonzero(hot == cold)[0]:
        sign[c] = -1.0 if comp[c, np.argmax(np.abs(comp[c]))] < 0.0 else 1.0
    return sign


def main(argv=None):
    a = parse_args(argv)
    el, ft, ld = a.element, a.feature, a.latent_dimension
    prefix = S.prefix(a.name, el)
    P, T, pe, feat, path = S.grid_inputs('pca', prefix, ft, 'the feature axes', more_axes=True)
    (pn, tn, sn), d = pe.shape, int(np.prod(feat.shape[3:]))
    if not 1 <= d <= MAX_FEAT:
        raise SystemExit('pca: %s has %d features per sample, more than %d' % (path, d, MAX_FEAT))
    if ld > d:
        raise SystemExit('pca: -ld %d is more than the %d features of %s' % (ld, d, path))
    x = np.ascontiguousarray(feat, dtype=np.float32).reshape(pn, tn, sn, d)
    kept, xfit = S.kept(x, a.skip, a.stride)
    n = pn * tn * kept
    if n < 2:
        raise SystemExit('pca: -sk %d -sd %d leave %d samples of %s, fewer than two' % (a.skip, a.stride, n, path))
    xfit = np.ascontiguousarray(xfit)                                # (x itself where no sample is left out)
    if a.verbose:
        print('pca of %s: %d features, fit on %d of %d samples, scaler %s' % (ft, d, n, pn * tn * sn, a.scaler))
    try:
        mean, lo, hi, gram = moments(xfit.reshape(n, d), a.device)
        s, comp, pcv = fit(lo, hi, gram, n, a.scaler, ld)
        z, norm2 = project(x.reshape(-1, d), mean, 1.0 / s, comp, a.device)
    except (RuntimeError, ValueError) as err:
        raise SystemExit('pca: %s: %s' % (path, err))
    z = z.reshape(pn, tn, sn, ld)
    sign = orient(comp, z[:, int(np.argmax(T))].mean(axis=(0, 1)), z[:, int(np.argmin(T))].mean(axis=(0, 1)))
    comp, z = comp * sign[:, None], z * sign
    out = dict(pcm=mean, pcs=s, pcc=comp, pcv=pcv, pcz=z, pcr=norm2.reshape(pn, tn, sn) - (z * z).sum(axis=-1))
    for key in SUFFIXES:
        np.save(prefix + '.%s.%s.npy' % (ft, key), out[key])
    for c in range(ld):
        np.save(prefix + '.%s.pc%d.npy' % (ft, c), np.ascontiguousarray(z[..., c]))
    if a.verbose:
        print('explained variance: %s' % np.array2string(pcv[1], precision=4))
        print('pc0 in %.6g .. %.6g; its state means at P = %g: %s' % (z[..., 0].min(), z[..., 0].max(), P[pn // 2],
                                                                    np.array2string(z[pn // 2, :, :, 0].mean(axis=1), precision=4)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
