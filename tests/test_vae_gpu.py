"""The VAE stage on the GPU (include/nm_vae.h) against tests/vae_ref.py: every layer of the network at sides 4 (a 1^3 bottleneck:
every tap but the centre is padding), 8 and 12 (odd inner sides 6 -> 3) and n = 1, 3, 65 (ragged against every 32- and 64-row tile),
exact on integers and within the any-order summation bound on floats; the model's forward, gradient, Nadam steps and training
against float64 within 8 times what float32 on the CPU differs from it, also at sides 16 and 32, latent sizes 1 and 64, without noise,
at a batch of one, a batch longer than the epoch and a repeated sample; a sample's forward bits whatever its batch; one context through
many calls; and neuralmelting_amd.vae end to end.  (tests/test_vae_forms_gpu.py: the kernel forms that these layers do not reach.)"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import vae_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import pca, vae

pytestmark = pytest.mark.gpu

SENT = np.float32(-7.25e30)
U = 2.0 ** -24
SIDES, COUNTS = (4, 8, 12), (1, 3, 65)
LAYERS = ('c0', 'c1', 'c2', 'c3', 't0', 't1', 't2', 't3', 't4')


def layer(name, S):
    """(side_in, cin, cout, stride, transposed, the network's act)"""
    h, q = S // 2, S // 4
    return dict(c0=(S, 1, 32, 1, 0, R.RELU), c1=(S, 32, 64, 2, 0, R.RELU), c2=(h, 64, 32, 1, 0, R.RELU), c3=(h, 32, 64, 2, 0, R.RELU),
                t0=(q, 64, 64, 1, 1, R.RELU), t1=(q, 64, 32, 2, 1, R.RELU), t2=(h, 32, 64, 1, 1, R.RELU), t3=(h, 64, 32, 2, 1, R.RELU),
                t4=(S, 32, 1, 1, 1, R.TANH))[name]


def _p(a):
    return None if a is None else a.ctypes.data_as(B.c_float_p)


def _check(rc):
    assert rc == B.NM_OK, B.load().nm_vae_last_error().decode()


def gpu_conv(x, w, b, stride, transposed, act):
    n, side, cin = x.shape[0], x.shape[1], x.shape[4]
    cout = b.size
    so = side * stride if transposed else side // stride
    y = np.full((n, so, so, so, cout), SENT)
    _check(B.load().nm_vae_conv(0, n, side, cin, cout, stride, transposed, act, _p(x), _p(w), _p(b), _p(y)))
    assert (y != SENT).all()
    return y


def gpu_conv_grad(x, w, y, gy, stride, transposed, act, want_gx=True):
    n, side, cin = x.shape[0], x.shape[1], x.shape[4]
    cout = y.shape[4]
    gx, gw, gb = np.full(x.shape, SENT), np.full(w.shape, SENT), np.full(cout, SENT)
    _check(B.load().nm_vae_conv_grad(0, n, side, cin, cout, stride, transposed, act, _p(x), _p(w), _p(y), _p(gy), _p(gx) if want_gx else None, _p(gw),
                                     _p(gb)))
    assert (gw != SENT).all() and (gb != SENT).all() and (gx != SENT).all() == want_gx
    return gx, gw, gb


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def layer_data(name, S, n, integer, seed):
    side, cin, cout, stride, tr, act = layer(name, S)
    so = side * stride if tr else side // stride
    rng = np.random.default_rng(seed)
    wshape = (3, 3, 3, cout, cin) if tr else (3, 3, 3, cin, cout)
    if integer:
        draw = lambda shape, m: f32(rng.integers(-m, m + 1, shape))
        return draw((n, side, side, side, cin), 4), draw(wshape, 3), draw(cout, 3), draw((n, so, so, so, cout), 4)
    draw = lambda shape: f32(rng.standard_normal(shape))
    return draw((n, side, side, side, cin)), draw(wshape) * np.float32(0.1), draw(cout), draw((n, so, so, so, cout))


# ---- exact on integers: |x|, |gy| <= 4, |w|, |b| <= 3, so every partial sum stays below 2^24 (forward and gx: at most 1729 terms of at
# most 12; gw and gb: at most 65 * 12^3 terms of at most 16 < 2^21) and the result is the restatement's whatever the order
@pytest.mark.parametrize('name', LAYERS)
@pytest.mark.parametrize('n', COUNTS)
@pytest.mark.parametrize('S', SIDES)
def test_conv_layers_are_exact_on_integers(S, n, name):
    side, cin, cout, stride, tr, _ = layer(name, S)
    x, w, b, gy = layer_data(name, S, n, True, 100 * S + n)
    for act in (R.NONE, R.RELU):
        ref = R.conv(x, w, b, stride, tr, act)
        y = gpu_conv(x, w, b, stride, tr, act)
        np.testing.assert_array_equal(y, ref)
        gx, gw, gb = gpu_conv_grad(x, w, y, gy, stride, tr, act)
        rx, rw, rb = R.conv_grad(x, w, ref, gy, stride, tr, act)
        np.testing.assert_array_equal(gx, rx)
        np.testing.assert_array_equal(gw, rw)
        np.testing.assert_array_equal(gb, rb)
    gx, gw2, gb2 = gpu_conv_grad(x, w, y, gy, stride, tr, act, want_gx=False)       # gx may be null; the same bits again
    assert (gx == SENT).all() and np.array_equal(gw2, gw) and np.array_equal(gb2, gb)


def dense_sizes(S, LD=8):
    f = 64 * (S // 4) ** 3
    return ((f, 8 * LD), (8 * LD, LD), (LD, f))


def gpu_dense(x, w, b, act):
    n, (din, dout) = x.shape[0], w.shape
    y = np.full((n, dout), SENT)
    _check(B.load().nm_vae_dense(0, n, din, dout, act, _p(x), _p(w), _p(b), _p(y)))
    assert (y != SENT).all()
    return y


def gpu_dense_grad(x, w, y, gy, act, want_gx=True):
    n, (din, dout) = x.shape[0], w.shape
    gx, gw, gb = np.full(x.shape, SENT), np.full(w.shape, SENT), np.full(dout, SENT)
    _check(B.load().nm_vae_dense_grad(0, n, din, dout, act, _p(x), _p(w), _p(y), _p(gy), _p(gx) if want_gx else None, _p(gw), _p(gb)))
    assert (gw != SENT).all() and (gb != SENT).all() and (gx != SENT).all() == want_gx
    return gx, gw, gb


@pytest.mark.parametrize('n', COUNTS)
@pytest.mark.parametrize('S', SIDES)
def test_dense_layers_are_exact_on_integers(S, n):
    rng = np.random.default_rng(7 * S + n)
    for din, dout in dense_sizes(S):
        x, w, b, gy = (f32(rng.integers(-m, m + 1, shape)) for shape, m in (((n, din), 4), ((din, dout), 3), (dout, 3), ((n, dout), 4)))
        for act in (R.NONE, R.RELU):
            ref = R.dense(x, w, b, act)
            y = gpu_dense(x, w, b, act)
            np.testing.assert_array_equal(y, ref)
            for got, want in zip(gpu_dense_grad(x, w, y, gy, act), R.dense_grad(x, w, ref, gy, act)):
                np.testing.assert_array_equal(got, want)


# ---- floats: within gamma_(K+1) sum |terms| of float64, K the number of terms (the bias included), u = 2^-24
def gamma(k):
    return k * U / (1.0 - k * U)


def within(name, got, ref, bound):
    err = np.abs(got.astype(np.float64) - ref)
    print('%s: error / bound %.3g' % (name, float((err / np.maximum(bound, 1e-300)).max())))
    assert (err <= bound).all(), name


@pytest.mark.parametrize('name', LAYERS)
@pytest.mark.parametrize('S,n', [(4, 3), (8, 65), (12, 1)])
def test_conv_layers_on_floats(S, n, name):
    side, cin, cout, stride, tr, act = layer(name, S)
    x, w, b, gy = layer_data(name, S, n, False, 1000 * S + n)
    so = side * stride if tr else side // stride
    pre = R.conv(x, w, b, stride, tr, R.NONE)
    bound = gamma(27 * cin + 2) * R.conv_abs(x, w, b, stride, tr)
    within('%s pre-activation' % name, gpu_conv(x, w, b, stride, tr, R.NONE), pre, bound)
    ref = R.conv(x, w, b, stride, tr, act)
    y = gpu_conv(x, w, b, stride, tr, act)
    # relu moves no two values apart; tanh's slope is at most 1 and the header gives its own error as 2 ulp of the result
    within('%s activated' % name, y, ref, bound + (2.0 ** -22 * np.abs(ref) if act == R.TANH else 0.0))
    # the gradients from the DEVICE's y: the prologue gy * act'(y) is one exact product for relu, three roundings more for tanh
    extra = 4 if act == R.TANH else 0
    gx, gw, gb = gpu_conv_grad(x, w, y, gy, stride, tr, act)
    rx, rw, rb = R.conv_grad(x, w, y, gy, stride, tr, act)
    ax, aw, ab = R.conv_grad_abs(x, w, y, gy, stride, tr, act)
    small = min(side, so) ** 3
    within('%s gx' % name, gx, rx, gamma(27 * cout + 1 + extra) * ax)
    within('%s gw' % name, gw, rw, gamma(n * small + 1 + extra) * aw)
    within('%s gb' % name, gb, rb, gamma(n * so ** 3 + 1 + extra) * ab)


@pytest.mark.parametrize('S,n', [(4, 3), (8, 65), (12, 1)])
def test_dense_layers_on_floats(S, n):
    rng = np.random.default_rng(S + n)
    for din, dout in dense_sizes(S):
        x, w, b, gy = (f32(rng.standard_normal(shape)) for shape in ((n, din), (din, dout), dout, (n, dout)))
        ref = R.dense(x, w, b, R.RELU)
        y = gpu_dense(x, w, b, R.RELU)
        within('dense %d->%d' % (din, dout), y, ref, gamma(din + 2) * (np.abs(x).astype(np.float64) @ np.abs(w) + np.abs(b)))
        g = np.abs(gy * R.dact(y, R.RELU))
        for what, got, want, bound in zip(('gx', 'gw', 'gb'), gpu_dense_grad(x, w, y, gy, R.RELU), R.dense_grad(x, w, y, gy, R.RELU),
                                          (gamma(dout + 1) * (g @ np.abs(w.T)), gamma(n + 1) * (np.abs(x.T).astype(np.float64) @ g), gamma(n + 1) * g.sum(axis=0))):
            within('dense %d->%d %s' % (din, dout, what), got, want, bound)


# ---- the model.  No bound is derivable through nine layers, so the allowance is measured: per tensor, 8 times the max-norm
# difference between the restatement in float32 on the CPU and in float64.  Both are float32 evaluations in different orders; a
# wrong tap or layout errs at order 1.
def allowance(what, got, ref32, ref64, parts=None):
    """got within 8 (ref32 - ref64) of ref64 in the max norm, for every part (slice) of the arrays"""
    worst, over = 0.0, []
    for name, sl in (parts or [(what, slice(None))]):
        allow = float(np.abs(np.asarray(ref32[sl], dtype=np.float64) - ref64[sl]).max())
        err = float(np.abs(np.asarray(got[sl], dtype=np.float64) - ref64[sl]).max())
        ratio = err / allow if allow > 0.0 else (0.0 if err == 0.0 else np.inf)
        worst = max(worst, ratio)
        if parts:
            print('  %s: error %.3g, float32 on the CPU differs by %.3g: ratio %.3g' % (name, err, allow, ratio))
        if not err <= 8.0 * allow:
            over.append('%s: error %.3g, float32 on the CPU differs by %.3g' % (name, err, allow))
    print('%s: largest (GPU - f64) / (CPU f32 - f64) = %.3g' % (what, worst))
    assert not over, '%s: %s' % (what, '; '.join(over))
    return worst


def tensors(S, LD):
    off = R.offsets(S, LD)
    names = [n + k for n in R.NAMES for k in ('.kernel', '.bias')]
    return [(names[i], slice(int(off[i]), int(off[i + 1]))) for i in range(26)]


def random_params(S, LD, rng):
    """the command line's initial parameters, with biases that count"""
    theta = vae.initial_params(S, LD, rng)
    off = R.offsets(S, LD)
    for l in range(13):
        theta[off[2 * l + 1]:off[2 * l + 2]] = 0.1 * rng.standard_normal(int(off[2 * l + 2] - off[2 * l + 1]))
    return theta


@functools.lru_cache(maxsize=None)
def model_case(S, LD, n):
    """random parameters, n samples in [0, 1), noise; the restatement's forward and gradient in both precisions, computed once"""
    rng = np.random.default_rng(S * 1000 + LD * 10 + n)
    theta = random_params(S, LD, rng)
    x = rng.random((n + 2, S, S, S), dtype=np.float32)
    idx = np.arange(n + 2, dtype=np.int64)[::-1][:n].copy()                 # the resident samples in another order, two left out
    eps = rng.standard_normal((n, LD), dtype=np.float32)
    ref = {}
    for key, dt in (('f64', torch.float64), ('f32', torch.float32)):
        ref[key] = dict(ev=R.evaluate(theta, S, LD, x[idx], eps, dt), ev0=R.evaluate(theta, S, LD, x[idx], None, dt), gr=R.gradient(theta, S, LD, x[idx], eps, dt))
    return theta, x, idx, eps, ref


def raw_eval(m, idx, eps, recon=True):
    n = idx.size
    out = [np.full((n, m.latent), SENT), np.full((n, m.latent), SENT), np.full((n, m.side ** 3), SENT), np.full(n, SENT), np.full(n, SENT)]
    _check(m.L.nm_vae_eval(m.ctx, n, idx.ctypes.data_as(B.c_int64_p), _p(eps), _p(out[0]), _p(out[1]), _p(out[2]) if recon else None, _p(out[3]), _p(out[4])))
    assert all((o != SENT).all() for i, o in enumerate(out) if recon or i != 2) and (recon or (out[2] == SENT).all())
    return out


def raw_grad(m, idx, eps):
    g, loss = np.full(m.nparams, SENT), np.full(2, -7.25e300)
    _check(m.L.nm_vae_grad(m.ctx, idx.size, idx.ctypes.data_as(B.c_int64_p), _p(eps), _p(g), loss.ctypes.data_as(B.c_double_p)))
    assert (g != SENT).all() and (loss != -7.25e300).all()
    return g, loss


# (the last two: long sides, and both ends of the latent size's range)
MODEL_CASES = [(4, 2, 3), (8, 8, 65), (12, 3, 1), (16, 64, 2), (32, 1, 1)]


@pytest.mark.parametrize('S,LD,n', MODEL_CASES)
def test_model_eval(S, LD, n):
    theta, x, idx, eps, ref = model_case(S, LD, n)
    with vae.Model(S, LD) as m:
        m.set_params(theta)
        m.data(x)
        np.testing.assert_array_equal(m.get_params(), theta)
        for key, e in (('ev', eps), ('ev0', None)):
            out = raw_eval(m, idx, e)
            for what, got, r32, r64 in zip(('z_mean', 'z_log_var', 'recon', 'rec', 'kl'), out, ref['f32'][key], ref['f64'][key]):
                allowance('eval %s (S %d, LD %d, n %d%s)' % (what, S, LD, n, '' if e is not None else ', no noise'), got, r32, r64)
            again = raw_eval(m, idx, e, recon=False)
            assert all(np.array_equal(a, b) for i, (a, b) in enumerate(zip(out, again)) if i != 2)


@pytest.mark.parametrize('S,LD,n', MODEL_CASES)
def test_model_grad(S, LD, n):
    theta, x, idx, eps, ref = model_case(S, LD, n)
    with vae.Model(S, LD) as m:
        m.set_params(theta)
        m.data(x)
        g, loss = raw_grad(m, idx, eps)
        allowance('grad (S %d, LD %d, n %d)' % (S, LD, n), g, ref['f32']['gr'][0], ref['f64']['gr'][0], tensors(S, LD))
        allowance('grad loss', loss, np.array(ref['f32']['gr'][1]), np.array(ref['f64']['gr'][1]))
        g2, loss2 = raw_grad(m, idx, eps)
        assert np.array_equal(g, g2) and np.array_equal(loss, loss2)
        np.testing.assert_array_equal(m.get_params(), theta)             # no update


def test_model_state_and_data_refusals():
    with vae.Model(4, 2) as m:
        idx, buf, two = np.zeros(1, dtype=np.int64), np.full(64, SENT), np.full(2, -7.25)
        assert m.L.nm_vae_grad(m.ctx, 1, idx.ctypes.data_as(B.c_int64_p), None, _p(buf), two.ctypes.data_as(B.c_double_p)) == B.NM_ERR_STATE
        m.set_params(np.zeros(m.nparams, dtype=np.float32))
        assert m.L.nm_vae_epoch(m.ctx, 1, idx.ctypes.data_as(B.c_int64_p), None, 1, 1e-3, two.ctypes.data_as(B.c_double_p)) == B.NM_ERR_STATE
        x = np.zeros((5, 64), dtype=np.float32)
        x[3, 17] = np.inf
        x[4, 0] = np.nan
        with pytest.raises(RuntimeError, match='nm_vae_data: x is not finite in sample 3'):
            m.data(x)
        m.data(np.zeros((5, 64), dtype=np.float32))
        idx[0] = 5
        assert m.L.nm_vae_grad(m.ctx, 1, idx.ctypes.data_as(B.c_int64_p), None, _p(buf), two.ctypes.data_as(B.c_double_p)) == B.NM_ERR_ARG
        assert 'idx[0]' in m.L.nm_vae_last_error().decode() and (two == -7.25).all()
        bad = np.zeros(m.nparams, dtype=np.float32)
        bad[7] = np.nan
        with pytest.raises(RuntimeError, match='not finite'):
            m.set_params(bad)


def test_optimiser_three_steps():
    """S = 4: 7 samples at batch 3, two full batches and a ragged one, against the restatement's three Nadam steps"""
    S, LD = 4, 2
    theta, x, _, _, _ = model_case(S, LD, 3)
    rng = np.random.default_rng(77)
    x = rng.random((7, S, S, S), dtype=np.float32)
    idx, eps = rng.permutation(7).astype(np.int64), rng.standard_normal((7, LD), dtype=np.float32)
    ref = {}
    for key, dt, ty in (('f64', torch.float64, np.float64), ('f32', torch.float32, np.float32)):
        opt = R.Nadam(theta.astype(ty))
        loss = R.epoch(opt, S, LD, x, idx, eps, 3, 1e-3, dt)
        ref[key] = (opt.theta, loss)
    with vae.Model(S, LD) as m:
        m.set_params(theta)
        m.data(x)
        loss = m.epoch(idx, eps, 3, 1e-3)
        got = m.get_params()
        # what three steps moved, not the parameters themselves: the steps are what the optimiser computes
        allowance('three Nadam steps', got.astype(np.float64) - theta, ref['f32'][0].astype(np.float64) - theta, ref['f64'][0] - theta, tensors(S, LD))
        # (the loss trace has its own test; here the batches' weights 3, 3, 1: rec is a sum of 64 squares, a few ulp; kl adds terms of
        # size 1 that cancel to about lv^2 / 2, so a few ulp OF 1)
        np.testing.assert_allclose(loss, ref['f64'][1], rtol=1e-5, atol=1e-6)
        m.set_params(theta)                                              # resets the optimiser: the same bits again
        loss2 = m.epoch(idx, eps, 3, 1e-3)
        assert np.array_equal(loss, loss2) and np.array_equal(m.get_params(), got)


# ---- the training paths at the edges of their arguments: no noise (the `eps ?` branches), a batch of one (the scale 2 / nb), a batch
# longer than the epoch, a sample twice in a batch
def both_precisions(f):
    """f(torch dtype, numpy type) for float32 and float64"""
    return f(torch.float32, np.float32), f(torch.float64, np.float64)


@functools.lru_cache(maxsize=None)
def seven_samples():
    S, LD = 4, 2
    rng = np.random.default_rng(78)
    return (S, LD, random_params(S, LD, rng), rng.random((7, S, S, S), dtype=np.float32), rng.permutation(7).astype(np.int64),
            rng.standard_normal((7, LD), dtype=np.float32))


def test_model_grad_without_noise():
    S, LD, n = 4, 2, 3
    theta, x, idx, _, _ = model_case(S, LD, n)
    r32, r64 = both_precisions(lambda dt, ty: R.gradient(theta, S, LD, x[idx], None, dt))
    with vae.Model(S, LD) as m:
        m.set_params(theta)
        m.data(x)
        g, loss = raw_grad(m, idx, None)
        allowance('grad without noise', g, r32[0], r64[0], tensors(S, LD))
        allowance('grad loss without noise', loss, np.array(r32[1]), np.array(r64[1]))


def test_model_grad_of_a_repeated_sample():
    S, LD, theta, x, _, eps = seven_samples()
    idx, e = np.array([5, 2, 5, 0, 5], dtype=np.int64), eps[:5]
    r32, r64 = both_precisions(lambda dt, ty: R.gradient(theta, S, LD, x[idx], e, dt))
    with vae.Model(S, LD) as m:
        m.set_params(theta)
        m.data(x)
        g, loss = raw_grad(m, idx, e)
        allowance('grad of a batch that repeats a sample', g, r32[0], r64[0], tensors(S, LD))
        allowance('its loss', loss, np.array(r32[1]), np.array(r64[1]))


@pytest.mark.parametrize('batch,noise', [(3, False), (1, True), (16, True)], ids=['batch3-no-noise', 'batch1', 'batch16'])
def test_optimiser_batch_shapes(batch, noise):
    """7 samples: three steps without noise, seven steps of one sample, one step of all seven (batch > nidx), against the
    restatement's steps as in test_optimiser_three_steps"""
    S, LD, theta, x, idx, eps = seven_samples()
    e = eps if noise else None

    def steps(dt, ty):
        opt = R.Nadam(theta.astype(ty))
        loss = R.epoch(opt, S, LD, x, idx, e, batch, 1e-3, dt)
        return opt.theta, loss
    r32, r64 = both_precisions(steps)
    with vae.Model(S, LD) as m:
        m.set_params(theta)
        m.data(x)
        loss = m.epoch(idx, e, batch, 1e-3)
        got = m.get_params()
        allowance('Nadam steps at batch %d%s' % (batch, '' if noise else ', no noise'), got.astype(np.float64) - theta, r32[0].astype(np.float64) - theta,
                  r64[0] - theta, tensors(S, LD))
        np.testing.assert_allclose(loss, r64[1], rtol=1e-5, atol=1e-6)      # (as in test_optimiser_three_steps)


def test_forward_does_not_depend_on_the_batch():
    """131 samples in eval's batches of 64, 64 and 3: every forward sum is one output's own, in tap and channel order, so a sample's
    results are the same bits alone, in another batch or at another row of a tile"""
    S, LD, n = 8, 3, 131
    rng = np.random.default_rng(80)
    theta, x = random_params(S, LD, rng), rng.random((n, S, S, S), dtype=np.float32)
    idx, eps = rng.permutation(n).astype(np.int64), rng.standard_normal((n, LD), dtype=np.float32)
    with vae.Model(S, LD) as m:
        m.set_params(theta)
        m.data(x)
        whole = raw_eval(m, idx, eps)
        for sl in [slice(i, i + 1) for i in (0, 63, 64, 127, 128, 130)] + [slice(64, 128)]:
            part = raw_eval(m, idx[sl].copy(), eps[sl].copy())
            for what, a, b in zip(('z_mean', 'z_log_var', 'recon', 'rec', 'kl'), part, whole):
                assert np.array_equal(a, b[sl]), (what, sl)


def test_one_context_through_many_calls():
    """the activations' buffers grow and keep their gradient halves (grad of 3, eval of 70, grad of 3; eval first, then grad), and no
    call leaves anything behind that the next one reads"""
    S, LD, n = 4, 2, 70
    rng = np.random.default_rng(79)
    theta, x = random_params(S, LD, rng), rng.random((n, S, S, S), dtype=np.float32)
    few, many = np.array([69, 0, 33], dtype=np.int64), rng.permutation(n).astype(np.int64)
    eps3, eps70 = rng.standard_normal((3, LD), dtype=np.float32), rng.standard_normal((n, LD), dtype=np.float32)
    with vae.Model(S, LD) as fresh:
        fresh.set_params(theta)
        fresh.data(x)
        want = raw_eval(fresh, many, eps70)
        g0 = raw_grad(fresh, few, eps3)                                     # buffers without gradients, then with
    with vae.Model(S, LD) as m:
        m.set_params(theta)
        m.data(x)
        g1 = raw_grad(m, few, eps3)
        got = raw_eval(m, many, eps70)
        assert all(np.array_equal(a, b) for a, b in zip(got, want))
        g2 = raw_grad(m, few, eps3)
        m.epoch(many[:6].copy(), eps70[:6].copy(), 2, 1e-3)
        assert not np.array_equal(m.get_params(), theta)
        m.set_params(theta)
        g3 = raw_grad(m, few, eps3)
        for g in (g0, g2, g3):
            assert np.array_equal(g[0], g1[0]) and np.array_equal(g[1], g1[1])
        m.data(x[:5])                                                       # fewer samples: 69 was resident, and is not any more
        ip, buf, two = few.ctypes.data_as(B.c_int64_p), np.full(m.nparams, SENT), np.full(2, -7.25)
        assert m.L.nm_vae_grad(m.ctx, 1, ip, None, _p(buf), two.ctypes.data_as(B.c_double_p)) == B.NM_ERR_ARG
        assert 'idx[0]' in m.L.nm_vae_last_error().decode()
        out = [np.full((1, LD), SENT), np.full((1, LD), SENT), np.full((1, S ** 3), SENT), np.full(1, SENT), np.full(1, SENT)]
        assert m.L.nm_vae_eval(m.ctx, 1, ip, None, *[_p(o) for o in out]) == B.NM_ERR_ARG
        assert m.L.nm_vae_epoch(m.ctx, 1, ip, None, 1, 1e-3, two.ctypes.data_as(B.c_double_p)) == B.NM_ERR_ARG
        assert (buf == SENT).all() and (two == -7.25).all() and all((o == SENT).all() for o in out)
        np.testing.assert_array_equal(m.get_params(), theta)
        raw_grad(m, np.array([4], dtype=np.int64), None)                   # the last of the new samples is taken


def test_learning_two_kinds_of_cubes():
    """S = 4, LD = 2: 256 cubes, a checkerboard or its complement plus small noise; 5 epochs at lr 1e-3 follow the restatement's
    loss trace from the same weights, order and noise, and the loss falls"""
    S, LD, n, batch, epochs = 4, 2, 256, 32, 5
    rng = np.random.default_rng(2024)
    z, y, xx = np.meshgrid(np.arange(S), np.arange(S), np.arange(S), indexing='ij')
    board = ((z + y + xx) % 2).astype(np.float32)
    kind = rng.integers(0, 2, n)
    x = f32(np.where(kind[:, None, None, None] == 1, board, 1.0 - board) + 0.05 * rng.standard_normal((n, S, S, S)))
    theta = vae.initial_params(S, LD, rng)
    orders = [rng.permutation(n).astype(np.int64) for _ in range(epochs)]
    noise = [rng.standard_normal((n, LD), dtype=np.float32) for _ in range(epochs)]
    ref = {}
    for key, dt, ty in (('f64', torch.float64, np.float64), ('f32', torch.float32, np.float32)):
        opt = R.Nadam(theta.astype(ty))
        ref[key] = np.array([R.epoch(opt, S, LD, x, orders[e], noise[e], batch, 1e-3, dt) for e in range(epochs)])
    with vae.Model(S, LD) as m:
        m.set_params(theta)
        m.data(x)
        trace = np.array([m.epoch(orders[e], noise[e], batch, 1e-3) for e in range(epochs)])
    print('loss per epoch (rec + kl): %s' % np.array2string(trace.sum(axis=1), precision=5))
    allowance('loss trace of 5 epochs', trace, ref['f32'], ref['f64'])
    assert trace[-1].sum() < trace[0].sum()


def test_end_to_end(tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    pn, tn, sn, S, LD = 2, 3, 8, 4, 2
    rng = np.random.default_rng(1)
    pre = vae.S.prefix('run', 'LJ')
    np.save(pre + '.virial.trgt.npy', np.float32([1, 2]))
    np.save(pre + '.temp.trgt.npy', np.float32([0.5, 1.0, 1.5]))
    np.save(pre + '.pe.npy', rng.standard_normal((pn, tn, sn)))
    cdf = rng.random((pn, tn, sn, S, S, S)) * np.float32([0.5, 1.0, 1.5])[None, :, None, None, None, None]
    np.save(pre + '.cdf.npy', cdf.astype(np.float32))
    common = ['-n', 'run', '-ld', str(LD), '-bs', '16', '-sk', '2']       # (-sk is the scaler's fit too: -lw wants the same)
    assert vae.main(common + ['-v', '-ep', '2']) == 0
    assert 'epoch    2' in capsys.readouterr().out
    want = dict(vaw=((R.nparams(S, LD),), np.float32), vat=((2, 3), np.float64), vam=((pn, tn, sn, LD), np.float64), vas=((pn, tn, sn, LD), np.float64),
                vak=((pn, tn, sn), np.float64), var=((pn, tn, sn), np.float64), vm0=((pn, tn, sn), np.float64), vm1=((pn, tn, sn), np.float64))
    out = {k: np.load(pre + '.cdf.%s.npy' % k) for k in want}
    for k, (shape, dtype) in want.items():
        assert out[k].shape == shape and out[k].dtype == dtype and np.isfinite(out[k]).all(), k
    assert np.array_equal(out['vm1'], out['vam'][..., 1]) and (out['vas'] > 0).all() and (out['vak'] >= 0).all() and (out['var'] >= 0).all()
    assert (out['vat'][:, 2] == 1e-4).all()
    assert vae.main(common + ['-lw']) == 0
    assert np.array_equal(np.load(pre + '.cdf.vam.npy'), out['vam'])
    assert np.array_equal(np.load(pre + '.cdf.vat.npy'), out['vat'])         # -lw leaves the trace alone
    assert pca.main(['-n', 'run', '-ft', 'cdf.vam', '-ld', '2']) == 0
    assert np.load(pre + '.cdf.vam.pcz.npy').shape == (pn, tn, sn, 2)
    np.save(pre + '.cdf.npy', np.zeros((pn, tn, sn, 11, 11, 11), dtype=np.float32))
    with pytest.raises(SystemExit) as e:
        vae.main(common)
    assert '11 -> 6 -> 3 -> 6 -> 12' in str(e.value)
