"""The cases and inputs of tests/golden/ref_vae.json, for its maker (tests/golden/make_golden_vae.py, run once at the commit whose
bytes the fixture pins) and for tests/test_vae_golden_gpu.py: the model at the smallest sizes at which each piece of the host logic
of csrc/nm_vae_api.hip can go wrong (the parameter offsets, the activations' sizes and their growth, the order and the buffers of
forward and backward), and one call of each layer primitive.  The stage is deterministic ("the same call twice gives the same
bits"), so every output is pinned byte for byte.

values(): the 64-bit linear congruential generator of tests/scan_cases.py (Knuth's MMIX constants) in closed form, s_k = A^k s_0 +
C (A^(k-1) + .. + 1) modulo 2^64, so numpy's wrapping uint64 products give the whole stream at once and no random-number library
is asked; the top 23 bits of a state, as a signed integer, times a power of two.  Every value is a dyadic rational of at most 23
significant bits, exact in float32.  The data lie in [-1, 1), the noise in [-4, 4), a parameter tensor in +-2^-max(3, ceil(log2(fan
in) / 2)), at most 1/8, its fan-in the kernel's count over the bias's: the activations then neither die out nor overflow on the way
through thirteen layers (the maker asserts that every output is finite and that no gradient tensor is all zero)."""
import ctypes as C
import hashlib

import numpy as np

from neuralmelting_amd import _lib as B

RELU = B.NM_VAE_ACT_RELU
SENTINEL = -77.0
LR = 2.0 ** -10

# (side, latent, n, batch): see model_case
MODEL_CASES = ((4, 1, 3, 2),        # the (S/4)^3 = 1 position layers, tiles with one to three live rows, a dense dout of 1, a ragged last batch of 1
               (8, 3, 5, 2),        # a ragged last batch of 1
               (12, 2, 2, 2),       # an odd quarter side: the parity classes of the stride-2 adjoint at 3^3
               (16, 8, 66, 3))      # eval crosses its internal batch of 64 (64 + 2); the epoch runs over the first 7 samples only
EPOCH_MOST, GRAD_MOST = 7, 3
PRIMITIVE_CASES = ('conv', 'conv_grad', 'conv_grad_nogx', 'dense', 'dense_grad')
CONV = dict(n=3, side=4, cin=32, cout=64, stride=2, transposed=0, act=RELU)
DENSE = dict(n=3, din=5, dout=1025, act=RELU)           # dout >= 1024: the wide form of the data gradient

_A, _C = np.uint64(6364136223846793005), np.uint64(1442695040888963407)


def values(count, seed, log2_bound):
    """(count,) float32 of the formula above, within +-2^log2_bound; `seed` picks the stream"""
    s0 = np.uint64((seed * 0x9E3779B97F4A7C15 + 1) & ((1 << 64) - 1))
    ak = np.cumprod(np.full(count, _A, dtype=np.uint64))                        # A^1 .. A^count, modulo 2^64
    geo = np.cumsum(np.concatenate([np.ones(1, dtype=np.uint64), ak[:-1]]))      # 1 + A + .. + A^(k-1)
    s = ak * s0 + _C * geo
    u = (s >> np.uint64(41)).astype(np.int64) - (1 << 22)
    x = (u * 2.0 ** (log2_bound - 22)).astype(np.float32)
    assert (x.astype(np.float64) * 2.0 ** (22 - log2_bound) == u).all()
    return x


def params(side, latent):
    """the flat parameter vector: every tensor, the biases too, from its own stream at its own bound"""
    off = np.zeros(B.NM_VAE_NTENSORS + 1, dtype=np.int64)
    assert B.load().nm_vae_layout(side, latent, off) == B.NM_OK
    theta = np.zeros(off[-1], dtype=np.float32)
    for l in range(B.NM_VAE_NTENSORS // 2):
        fan = int(off[2 * l + 1] - off[2 * l]) // int(off[2 * l + 2] - off[2 * l + 1])
        bound = -max(3, -(-(fan - 1).bit_length() // 2))                        # ceil(ceil(log2 fan) / 2)
        for t in (2 * l, 2 * l + 1):
            theta[off[t]:off[t + 1]] = values(int(off[t + 1] - off[t]), 100 * side + t, bound)
    assert np.abs(theta).max() <= 0.125
    return theta


def digest(a):
    """the shape, the dtype and the SHA-256 of an output's bytes; an array of at most 64 elements in full as well (a float's JSON
    form reads back to the same bits), so that a failure shows numbers"""
    assert a.dtype in (np.float32, np.float64) and a.flags.c_contiguous
    d = {'shape': list(a.shape), 'dtype': a.dtype.name, 'sha256': hashlib.sha256(a.tobytes()).hexdigest()}
    if a.size <= 64:
        d['values'] = a.ravel().tolist()
    return d


def _out(*shape, dtype=np.float32):
    return np.full(shape, SENTINEL, dtype=dtype)


def _ok(L, rc):
    assert rc == B.NM_OK, L.nm_vae_last_error().decode()


def model_key(side, latent, n, batch):
    return 'model_s%d_ld%d_n%d_b%d' % (side, latent, n, batch)


def model_case(side, latent, n, batch):
    """every output, by name, of these calls through the raw ABI on sentinel-filled arrays, in this order on ONE context, so that
    the activations grow without gradients, then with them, and are then used again: nm_vae_eval of all n samples with noise and
    recon; nm_vae_grad of the first min(n, 3); two nm_vae_epoch at `batch` over the first min(n, 7), last first; nm_vae_get_params;
    nm_vae_eval without noise and without recon"""
    L = B.load()
    per, ne, ng = side ** 3, min(n, EPOCH_MOST), min(n, GRAD_MOST)
    theta, x = params(side, latent), values(n * per, 7000 + side, 0).reshape(n, per)
    eps = values(n * latent, 8000 + side, 2).reshape(n, latent)
    all_idx, epoch_idx = np.arange(n, dtype=np.int64), np.arange(ne, dtype=np.int64)[::-1].copy()
    out = {}
    ctx = C.c_void_p()
    _ok(L, L.nm_vae_create(0, side, latent, C.byref(ctx)))
    try:
        _ok(L, L.nm_vae_set_params(ctx, theta))
        _ok(L, L.nm_vae_data(ctx, n, x))
        e = out['eval_mu'], out['eval_lv'], out['eval_recon'], out['eval_rec'], out['eval_kl'] = (
            _out(n, latent), _out(n, latent), _out(n, per), _out(n), _out(n))
        _ok(L, L.nm_vae_eval(ctx, n, all_idx, eps, *e))
        out['grad'], out['grad_loss'] = _out(theta.size), _out(2, dtype=np.float64)
        _ok(L, L.nm_vae_grad(ctx, ng, all_idx[:ng].copy(), eps[:ng].copy(), out['grad'], out['grad_loss']))
        for k in (1, 2):
            out['epoch%d_loss' % k] = _out(2, dtype=np.float64)
            noise = values(ne * latent, 9000 + 10 * side + k, 2).reshape(ne, latent)
            _ok(L, L.nm_vae_epoch(ctx, ne, epoch_idx, noise, batch, LR, out['epoch%d_loss' % k]))
        out['params'] = _out(theta.size)
        _ok(L, L.nm_vae_get_params(ctx, out['params']))
        p = out['plain_mu'], out['plain_lv'], out['plain_rec'], out['plain_kl'] = _out(n, latent), _out(n, latent), _out(n), _out(n)
        _ok(L, L.nm_vae_eval(ctx, n, all_idx, None, p[0], p[1], None, p[2], p[3]))
    finally:
        L.nm_vae_destroy(ctx)
    return out


def primitive_case(name):
    """one call of a layer primitive: the 32 -> 64 stride-2 convolution at side 4 and its gradient (with gx, and with gx = NULL), the
    dense layer 5 -> 1025 and its gradient; the gradients at the y that the forward call of the same shape gives"""
    L = B.load()
    if name.startswith('conv'):
        c = CONV
        n, so = c['n'], c['side'] // c['stride']
        head = (0, n, c['side'], c['cin'], c['cout'], c['stride'], c['transposed'], c['act'])
        x, w = values(n * c['side'] ** 3 * c['cin'], 11, 0), values(27 * c['cin'] * c['cout'], 12, -5)
        b, y = values(c['cout'], 13, -5), _out(n, so, so, so, c['cout'])
        _ok(L, L.nm_vae_conv(*head, x, w, b, y))
        if name == 'conv':
            return {'y': y}
        out = {'gw': _out(27, c['cin'], c['cout']), 'gb': _out(c['cout'])}
        if name == 'conv_grad':
            out['gx'] = _out(n, c['side'], c['side'], c['side'], c['cin'])
        _ok(L, L.nm_vae_conv_grad(*head, x, w, y, values(y.size, 14, 0), out.get('gx'), out['gw'], out['gb']))
        return out
    d = DENSE
    head = (0, d['n'], d['din'], d['dout'], d['act'])
    x, w, b, y = values(d['n'] * d['din'], 21, 0), values(d['din'] * d['dout'], 22, -1), values(d['dout'], 23, -1), _out(d['n'], d['dout'])
    _ok(L, L.nm_vae_dense(*head, x, w, b, y))
    if name == 'dense':
        return {'y': y}
    out = {'gx': _out(d['n'], d['din']), 'gw': _out(d['din'], d['dout']), 'gb': _out(d['dout'])}
    _ok(L, L.nm_vae_dense_grad(*head, x, w, y, values(y.size, 24, 0), out['gx'], out['gw'], out['gb']))
    return out


def every_case():
    """(key, a function that runs the case) of all of them, in the fixture's order"""
    return [(model_key(*c), lambda c=c: model_case(*c)) for c in MODEL_CASES] + [(name, lambda name=name: primitive_case(name)) for name in PRIMITIVE_CASES]
