"""The reference's variational autoencoder over the whole replica grid (include/nm_vae.h): lammps_vae.py's
3-D convolutional VAE of distr's cube histograms, trained and applied in the HIP library (nm_vae_*: convolutions and their
gradients on the float32 matrix instruction, Keras 2's Nadam); there is no host fallback.  The host draws what is random and
keeps the schedule: the initial weights (convolution kernels He-normal truncated at two standard deviations, with Keras's fans
27 * shape[-2]; dense kernels Glorot-uniform; biases zero), the split of the fit samples into training and validation, every
epoch's order and noise, all from numpy.random.default_rng(seed) in this order (the build's own streams: Keras's cannot be
matched), and ReduceLROnPlateau on the validation loss with Keras's defaults (factor 0.1, patience 4, min_delta 1e-4).

The latents are per-sample features and observables, so the stages behind take them unchanged - the reference's chain:

    python -m neuralmelting_amd.distr -v -n remcmc_run_5 -e LJ -cb 12
    python -m neuralmelting_amd.vae -v -n remcmc_run_5 -e LJ -sk 128 -ep 64
    python -m neuralmelting_amd.pca -v -n remcmc_run_5 -e LJ -ft cdf.vam -ld 2
    python -m neuralmelting_amd.manifold -v -n remcmc_run_5 -e LJ -ft cdf.vam
    python -m neuralmelting_amd.reweight -v -n remcmc_run_5 -e LJ -sk 128 -ob cdf.vm0 -hq cdf.vm0 -bs 200

Scalers (fitted on the training and validation samples, applied to all): none; global (the reference's default):
(x - min) / (max - min) over everything; standard: (x - mean_j) / std_j per voxel; minmax: (x - min_j) / (max_j - min_j) per
voxel; a constant voxel is divided by 1.
"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

from . import _lib as B
from . import _stage as S

SCALERS = ('none', 'global', 'standard', 'minmax')
SUFFIXES = ('vaw', 'vat', 'vam', 'vas', 'vak', 'var')
FACTOR, PATIENCE, MIN_DELTA = 0.1, 4, 1e-4      # ReduceLROnPlateau, Keras's defaults
CONV_LAYERS = (0, 1, 2, 3, 8, 9, 10, 11, 12)    # of the 13 layers c0 c1 c2 c3 d0 dm dv d1 t0 t1 t2 t3 t4
TRANSPOSED_FROM = 8                             # t0 .. t4 are transposed convolutions


def parse_args(argv=None):
    p = argparse.ArgumentParser(
        description='VAE of the cube feature F of distr over the (P, T) grid: .F.vaw the parameters (float32, include/nm_vae.h\'s order); '
        '.F.vat (EP, 3) training loss, validation loss, learning rate; .F.vam and .F.vas (PN, TN, SN, LD) z_mean and exp(z_log_var / 2); '
        '.F.vak and .F.var (PN, TN, SN) kl and the squared reconstruction error at z = z_mean; .F.vm0 ... one latent mean each, for '
        'reweight -ob F.vm0 -hq F.vm0.  All but .vaw float64.')
    p.add_argument('-v', '--verbose', action='store_true')
    p.add_argument('-n', '--name', type=str, default='remcmc_init')
    p.add_argument('-e', '--element', type=str, default='LJ')
    p.add_argument('-ft', '--feature', type=str, default='cdf', help='<PREFIX>.FEATURE.npy of shape (PN, TN, SN, S, S, S), S a multiple of 4 in 4..32')
    p.add_argument('-sc', '--scaler', type=str, default='global', choices=SCALERS)
    p.add_argument('-ld', '--latent_dimension', type=int, default=8, help='1..64')
    p.add_argument('-ep', '--epochs', type=int, default=1024)
    p.add_argument('-lr', '--learning_rate', type=float, default=1e-4)
    p.add_argument('-bs', '--batch_size', type=int, default=64, help='1..4096')
    p.add_argument('-sd', '--seed', type=int, default=256)
    p.add_argument('-sk', '--skip', type=int, default=0, help='samples of every grid point left out of the FIT at its start')
    p.add_argument('-st', '--stride', type=int, default=1, help='the fit uses every STRIDE-th sample; all samples are encoded')
    p.add_argument('-vf', '--validation_fraction', type=float, default=0.25, help='the share of the fit samples that only validates')
    p.add_argument('-lw', '--load_weights', action='store_true', help='load .F.vaw.npy and only encode')
    p.add_argument('-dv', '--device', type=int, default=0)
    a = p.parse_args(argv)
    if a.skip < 0 or a.stride < 1 or not 1 <= a.latent_dimension <= 64 or a.epochs < 1 or not 1 <= a.batch_size <= 4096:
        p.error('need -sk >= 0, -st >= 1, -ld in 1..64, -ep >= 1 and -bs in 1..4096')
    if not a.learning_rate > 0.0 or not 0.0 <= a.validation_fraction < 1.0:
        p.error('need -lr > 0 and -vf in [0, 1)')
    return a


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def nparams(side, latent):
    return B.call('nm_vae_nparams', side, latent)


def layout(side, latent):
    """the 27 offsets of the parameter tensors in the flat vector (include/nm_vae.h)"""
    off = np.zeros(B.NM_VAE_NTENSORS + 1, dtype=np.int64)
    B.call('nm_vae_layout', side, latent, off)
    return off


def initial_params(side, latent, rng):
    """the flat float32 parameter vector as Keras would draw its kind: see the module's text"""
    off = layout(side, latent)
    theta = np.zeros(off[-1], dtype=np.float32)
    for l in range(13):
        count, out = int(off[2 * l + 1] - off[2 * l]), int(off[2 * l + 2] - off[2 * l + 1])      # of the kernel; of the bias: cout or dout
        if l in CONV_LAYERS:
            w = rng.standard_normal(count)
            while True:
                far = np.nonzero(np.abs(w) > 2.0)[0]
                if far.size == 0:
                    break
                w[far] = rng.standard_normal(far.size)
            # the kernel's axis -2: cin of a convolution (k, cin, cout), cout of a transposed one (k, cout, cin)
            w *= np.sqrt(2.0 / (27 * (count // (27 * out) if l < TRANSPOSED_FROM else out)))
        else:
            limit = np.sqrt(6.0 / (count // out + out))
            w = rng.uniform(-limit, limit, count)
        theta[off[2 * l]:off[2 * l + 1]] = w
    return theta


class Model:
    """an nm_vae context: the parameters, the optimiser's state and the resident samples on the device"""

    def __init__(self, side, latent, device=0):
        self.L, self.side, self.latent, self.ctx = B.load(), side, latent, C.c_void_p()
        B.call('nm_vae_create', device, side, latent, C.byref(self.ctx))
        self.nparams = nparams(side, latent)

    def close(self):
        if self.ctx:
            self.L.nm_vae_destroy(self.ctx)
            self.ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_params(self, theta):
        theta = _f32(theta)
        if theta.shape != (self.nparams,):
            raise ValueError('theta wants the shape (%d,)' % self.nparams)
        B.call('nm_vae_set_params', self.ctx, theta)

    def get_params(self):
        theta = np.empty(self.nparams, dtype=np.float32)
        B.call('nm_vae_get_params', self.ctx, theta)
        return theta

    def data(self, x):
        x = _f32(x).reshape(-1, self.side ** 3)
        B.call('nm_vae_data', self.ctx, x.shape[0], x)

    def _idx(self, idx, eps):
        idx, eps = np.ascontiguousarray(idx, dtype=np.int64), _f32(eps)
        if idx.ndim != 1 or (eps is not None and eps.shape != (idx.size, self.latent)):
            raise ValueError('idx wants the shape (n,), eps (n, %d)' % self.latent)
        return idx, eps

    def eval(self, idx, eps=None, recon=False):
        """(z_mean, z_log_var, rec, kl[, recon]) of the resident samples idx"""
        idx, eps = self._idx(idx, eps)
        n = idx.size
        mu, lv = np.empty((n, self.latent), dtype=np.float32), np.empty((n, self.latent), dtype=np.float32)
        rec, kl = np.empty(n, dtype=np.float32), np.empty(n, dtype=np.float32)
        y = np.empty((n, self.side ** 3), dtype=np.float32) if recon else None
        B.call('nm_vae_eval', self.ctx, n, idx, eps, mu, lv, y, rec, kl)
        return (mu, lv, rec, kl, y) if recon else (mu, lv, rec, kl)

    def grad(self, idx, eps=None):
        """(the gradient of the batch's mean loss, (mean rec, mean kl))"""
        idx, eps = self._idx(idx, eps)
        g, loss = np.empty(self.nparams, dtype=np.float32), np.empty(2)
        B.call('nm_vae_grad', self.ctx, idx.size, idx, eps, g, loss)
        return g, loss

    def epoch(self, idx, eps, batch, lr):
        """Nadam steps over the consecutive batches of idx: (mean rec, mean kl)"""
        idx, eps = self._idx(idx, eps)
        loss = np.empty(2)
        B.call('nm_vae_epoch', self.ctx, idx.size, idx, eps, batch, lr, loss)
        return loss

    def timing(self):
        ms = np.empty(4)
        B.call('nm_vae_last_timing', ms)
        return ms


def scale(x, fit, scaler):
    """x (N, D) float32 scaled by `scaler` fitted on its rows `fit`"""
    if scaler == 'none':
        return x
    f = x[fit].astype(np.float64)
    if scaler == 'global':
        lo, s = f.min(), f.max() - f.min()
        if not s > 0.0:
            raise ValueError('-sc global: every value of the feature is %g, there is nothing to scale' % lo)
    elif scaler == 'standard':
        lo, s = f.mean(axis=0), f.std(axis=0)
    else:
        lo, s = f.min(axis=0), f.max(axis=0) - f.min(axis=0)
    s = np.where(s > 0.0, s, 1.0)
    return ((x - lo) / s).astype(np.float32)


class Plateau:
    """Keras's ReduceLROnPlateau (mode min, no cooldown, min_lr 0)"""

    def __init__(self, lr):
        self.lr, self.best, self.wait = lr, np.inf, 0

    def update(self, loss):
        if loss < self.best - MIN_DELTA:
            self.best, self.wait = loss, 0
            return
        self.wait += 1
        if self.wait >= PATIENCE:
            self.lr, self.wait = self.lr * FACTOR, 0


def train(model, train_idx, val_idx, epochs, batch, lr, rng, verbose=False):
    """(EP, 3) training loss, validation loss (the training loss where nothing validates), learning rate"""
    trace, plateau, ld = np.zeros((epochs, 3)), Plateau(lr), model.latent
    for ep in range(epochs):
        order = rng.permutation(train_idx)
        loss = model.epoch(order, rng.standard_normal((order.size, ld), dtype=np.float32), batch, plateau.lr).sum()
        val = loss
        if val_idx.size:
            _, _, rec, kl = model.eval(val_idx, rng.standard_normal((val_idx.size, ld), dtype=np.float32))
            val = float(np.mean(rec.astype(np.float64) + kl))
        trace[ep] = loss, val, plateau.lr
        if verbose:
            print('epoch %4d: loss %.6g, validation %.6g, lr %g' % (ep + 1, loss, val, plateau.lr))
        plateau.update(val)
    return trace


def main(argv=None):
    a = parse_args(argv)
    el, ft, ld = a.element, a.feature, a.latent_dimension
    prefix = S.prefix(a.name, el)
    P, T, pe, feat, path = S.grid_inputs('vae', prefix, ft, 'the three axes of a cube', more_axes=True)
    pn, tn, sn = pe.shape
    side = feat.shape[3]
    if feat.ndim != 6 or feat.shape[3:] != (side,) * 3:
        raise SystemExit('vae: %s has shape %s, not %s followed by the three equal axes of a cube' % (path, feat.shape, pe.shape))
    if side % 4 or not 4 <= side <= 32:
        raise SystemExit('vae: %s holds cubes of side %d, but the side must be a multiple of 4 in 4..32: the decoder doubles a quarter of '
                         'the side twice (distr -cb 11 would give 11 -> 6 -> 3 -> 6 -> 12); run distr with -cb 8, 12, 16, ...' % (path, side))
    wpath = prefix + '.%s.vaw.npy' % ft
    if a.load_weights and not os.path.isfile(wpath):
        raise SystemExit('vae: -lw: %s is missing' % wpath)
    x = np.ascontiguousarray(feat, dtype=np.float32).reshape(pn * tn * sn, side ** 3)
    fit = np.arange(pn * tn * sn).reshape(pn, tn, sn)[:, :, a.skip::a.stride].ravel()
    if fit.size < 2:
        raise SystemExit('vae: -sk %d -st %d leave %d samples of %s, fewer than two' % (a.skip, a.stride, fit.size, path))
    rng = np.random.default_rng(a.seed)
    try:
        x = scale(x, fit, a.scaler)
        with Model(side, ld, a.device) as model:
            model.data(x)
            if a.load_weights:
                theta = np.load(wpath)
                if theta.shape != (model.nparams,):
                    raise ValueError('%s has shape %s, not (%d,): another side or -ld' % (wpath, theta.shape, model.nparams))
                model.set_params(theta)
            else:
                model.set_params(initial_params(side, ld, rng))
                mixed = rng.permutation(fit)
                nval = int(round(a.validation_fraction * fit.size))
                if nval >= fit.size:
                    raise ValueError('-vf %g leaves no sample to train on' % a.validation_fraction)
                if a.verbose:
                    print('vae of %s: side %d, latent %d, %d parameters; %d samples train, %d validate, scaler %s'
                          % (ft, side, ld, model.nparams, fit.size - nval, nval, a.scaler))
                trace = train(model, mixed[:fit.size - nval], mixed[fit.size - nval:], a.epochs, a.batch_size, a.learning_rate, rng, a.verbose)
                np.save(wpath, model.get_params())
                np.save(prefix + '.%s.vat.npy' % ft, trace)
            mu, lv, rec, kl = model.eval(np.arange(pn * tn * sn))
    except (RuntimeError, ValueError) as err:
        raise SystemExit('vae: %s: %s' % (path, err))
    mu = mu.astype(np.float64).reshape(pn, tn, sn, ld)
    out = dict(vam=mu, vas=np.exp(0.5 * lv.astype(np.float64)).reshape(pn, tn, sn, ld), vak=kl.astype(np.float64).reshape(pn, tn, sn),
               var=rec.astype(np.float64).reshape(pn, tn, sn))
    for key, value in out.items():
        np.save(prefix + '.%s.%s.npy' % (ft, key), value)
    for c in range(ld):
        np.save(prefix + '.%s.vm%d.npy' % (ft, c), np.ascontiguousarray(mu[..., c]))
    if a.verbose:
        print('z_mean 0 in %.6g .. %.6g; its state means at P = %g: %s' % (mu[..., 0].min(), mu[..., 0].max(), P[pn // 2],
                                                                        np.array2string(mu[pn // 2, :, :, 0].mean(axis=1), precision=4)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
