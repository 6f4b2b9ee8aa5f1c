"""The VAE stage without a GPU (include/nm_vae.h, neuralmelting_amd/vae.py): the interface, every refusal that precedes the device
check on sentinel-filled outputs, the parameter count, and tests/vae_ref.py itself: the adjoint identity of both stride-2 maps,
its Nadam against the formula written out by hand, its gradient against central differences."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import vae_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import vae

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = np.float32(-7.25e30)


def test_header_symbols_are_exported_and_bound():
    txt = open(os.path.join(ROOT, 'include', 'nm_vae.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    syms = sorted(set(re.findall(r'\b(nm_[a-z_0-9]+)\s*\(', txt)))
    assert syms == sorted(B.VAE_SYMBOLS) and len(syms) == 16
    raw = C.CDLL(B.LIB_PATH)
    for s in syms:
        assert hasattr(raw, s), s
    L = B.load()
    assert L.nm_vae_nparams.restype is C.c_int64
    assert L.nm_vae_conv.restype is C.c_int and len(L.nm_vae_conv.argtypes) == 12
    assert len(L.nm_vae_conv_grad.argtypes) == 15 and len(L.nm_vae_dense.argtypes) == 9 and len(L.nm_vae_dense_grad.argtypes) == 12
    assert len(L.nm_vae_eval.argtypes) == 9 and len(L.nm_vae_grad.argtypes) == 6 and len(L.nm_vae_epoch.argtypes) == 7
    assert L.nm_vae_last_error.restype is C.c_char_p


@pytest.mark.parametrize('side', [4, 8, 16])
@pytest.mark.parametrize('latent', [1, 8])
def test_nparams_and_layout_match_the_restatement(side, latent):
    assert B.load().nm_vae_nparams(side, latent) == R.nparams(side, latent)
    np.testing.assert_array_equal(vae.layout(side, latent), R.offsets(side, latent))


@pytest.mark.parametrize('side,latent', [(4, 1), (8, 8), (16, 64), (32, 1)])
def test_initial_params_are_the_restatement_s_draws(side, latent):
    """bit for bit, and the generator left where the restatement leaves it: convolution kernels He-normal with Keras's fan 27 *
    shape[-2], redrawn beyond two standard deviations; dense kernels Glorot-uniform; biases zero; the shapes from vae_ref"""
    seed = 1000 * side + latent
    rng, shapes, off = np.random.default_rng(seed), R.shapes(side, latent), R.offsets(side, latent)
    want = np.zeros(off[-1], dtype=np.float32)
    for l in range(len(R.NAMES)):
        k = shapes[2 * l]
        if len(k) == 5:
            w = rng.standard_normal(int(np.prod(k)))
            while (np.abs(w) > 2.0).any():
                far = np.nonzero(np.abs(w) > 2.0)[0]
                w[far] = rng.standard_normal(far.size)
            w *= np.sqrt(2.0 / (27 * k[-2]))
        else:
            limit = np.sqrt(6.0 / (k[0] + k[1]))
            w = rng.uniform(-limit, limit, int(np.prod(k)))
        want[off[2 * l]:off[2 * l + 1]] = w
    mine = np.random.default_rng(seed)
    got = vae.initial_params(side, latent, mine)
    assert got.dtype == np.float32 and got.shape == want.shape and got.tobytes() == want.tobytes()
    assert mine.random() == rng.random()


# ---- refusals: NM_ERR_ARG without a device, the message in the function's name, the outputs untouched
def _p(a):
    return None if a is None else a.ctypes.data_as(B.c_float_p)


def call_conv(grad=False, device=0, n=2, side=4, cin=32, cout=64, stride=2, transposed=0, act=1, null=()):
    L = B.load()
    m, s, ci, co = max(n, 1), max(side, 1), max(cin, 1), max(cout, 1)       # the arrays of a refused call only have to exist
    so = s * max(stride, 1) if transposed else max(s // max(stride, 1), 1)
    rng = np.random.default_rng(3)
    a = dict(x=rng.random((m, s, s, s, ci), dtype=np.float32), w=rng.random((27, ci, co), dtype=np.float32), b=rng.random(co, dtype=np.float32),
             y=rng.random((m, so, so, so, co), dtype=np.float32), gy=rng.random((m, so, so, so, co), dtype=np.float32))
    if grad:
        out = dict(gx=np.full(a['x'].shape, SENT), gw=np.full(a['w'].shape, SENT), gb=np.full(co, SENT))
        args = [a[k] if k not in null else None for k in ('x', 'w', 'y', 'gy')] + [out[k] if k not in null else None for k in ('gx', 'gw', 'gb')]
        rc = L.nm_vae_conv_grad(device, n, side, cin, cout, stride, transposed, act, *[_p(v) for v in args])
    else:
        out = dict(y=np.full(a['y'].shape, SENT))
        args = [a[k] if k not in null else None for k in ('x', 'w', 'b')] + [out['y'] if 'y' not in null else None]
        rc = L.nm_vae_conv(device, n, side, cin, cout, stride, transposed, act, *[_p(v) for v in args])
    return rc, L.nm_vae_last_error().decode(), all((v == SENT).all() for v in out.values())


def call_dense(grad=False, device=0, n=3, din=5, dout=4, act=1, null=()):
    L = B.load()
    rng = np.random.default_rng(4)
    m, di, do = max(n, 1), max(din, 1), max(dout, 1)
    a = dict(x=rng.random((m, di), dtype=np.float32), w=rng.random((di, do), dtype=np.float32), b=rng.random(do, dtype=np.float32),
             y=rng.random((m, do), dtype=np.float32), gy=rng.random((m, do), dtype=np.float32))
    if grad:
        out = dict(gx=np.full((m, di), SENT), gw=np.full((di, do), SENT), gb=np.full(do, SENT))
        args = [a[k] if k not in null else None for k in ('x', 'w', 'y', 'gy')] + [out[k] if k not in null else None for k in ('gx', 'gw', 'gb')]
        rc = L.nm_vae_dense_grad(device, n, din, dout, act, *[_p(v) for v in args])
    else:
        out = dict(y=np.full((m, do), SENT))
        args = [a[k] if k not in null else None for k in ('x', 'w', 'b')] + [out['y'] if 'y' not in null else None]
        rc = L.nm_vae_dense(device, n, din, dout, act, *[_p(v) for v in args])
    return rc, L.nm_vae_last_error().decode(), all((v == SENT).all() for v in out.values())


CONV_BAD = {
    'stride3': dict(stride=3), 'stride0': dict(stride=0), 'transposed2': dict(transposed=2), 'act3': dict(act=3), 'act-1': dict(act=-1),
    'cin0': dict(cin=0), 'cout65': dict(cout=65), 'side0': dict(side=0), 'side65': dict(side=65), 'odd-side-stride2': dict(side=5),
    'out-side-128': dict(side=64, transposed=1, n=1, cin=1, cout=1), 'n0': dict(n=0), 'n-2': dict(n=-2), 'device-1': dict(device=-1),
    'null-x': dict(null=('x',)), 'null-w': dict(null=('w',)),
}


@pytest.mark.parametrize('case', sorted(CONV_BAD))
@pytest.mark.parametrize('grad', [False, True])
def test_conv_refusals(case, grad):
    rc, msg, untouched = call_conv(grad, **CONV_BAD[case])
    assert rc == B.NM_ERR_ARG and untouched
    assert msg.startswith('nm_vae_conv_grad: ' if grad else 'nm_vae_conv: ')


@pytest.mark.parametrize('grad,null', [(False, 'b'), (False, 'y'), (True, 'y'), (True, 'gy'), (True, 'gw'), (True, 'gb')])
def test_conv_null_pointers(grad, null):
    rc, msg, untouched = call_conv(grad, null=(null,))
    assert rc == B.NM_ERR_ARG and untouched and 'null' in msg


DENSE_BAD = {'n0': dict(n=0), 'din0': dict(din=0), 'dout-1': dict(dout=-1), 'act5': dict(act=5), 'device-1': dict(device=-1), 'null-x': dict(null=('x',)),
             'null-w': dict(null=('w',))}


@pytest.mark.parametrize('case', sorted(DENSE_BAD))
@pytest.mark.parametrize('grad', [False, True])
def test_dense_refusals(case, grad):
    rc, msg, untouched = call_dense(grad, **DENSE_BAD[case])
    assert rc == B.NM_ERR_ARG and untouched
    assert msg.startswith('nm_vae_dense_grad: ' if grad else 'nm_vae_dense: ')


@pytest.mark.parametrize('side,latent,word', [(11, 8, '11 -> 6 -> 3 -> 6 -> 12'), (0, 8, 'side'), (36, 8, 'side'), (6, 8, 'side'), (8, 0, 'latent'),
                                              (8, 65, 'latent'), (8, -1, 'latent')])
def test_model_refusals(side, latent, word):
    L = B.load()
    ctx = C.c_void_p(0x5a5a)
    assert L.nm_vae_create(0, side, latent, C.byref(ctx)) == B.NM_ERR_ARG and ctx.value == 0x5a5a
    msg = L.nm_vae_last_error().decode()
    assert msg.startswith('nm_vae_create: ') and word in msg
    assert L.nm_vae_nparams(side, latent) == B.NM_ERR_ARG
    assert L.nm_vae_last_error().decode().startswith('nm_vae_nparams: ')
    off = np.full(27, -5, dtype=np.int64)
    assert L.nm_vae_layout(side, latent, off.ctypes.data_as(B.c_int64_p)) == B.NM_ERR_ARG and (off == -5).all()


def test_model_null_and_device_refusals():
    L = B.load()
    ctx = C.c_void_p(0x5a5a)
    assert L.nm_vae_create(-1, 8, 8, C.byref(ctx)) == B.NM_ERR_ARG and ctx.value == 0x5a5a
    assert 'device' in L.nm_vae_last_error().decode()
    assert L.nm_vae_create(0, 8, 8, None) == B.NM_ERR_ARG
    assert L.nm_vae_layout(8, 8, None) == B.NM_ERR_ARG
    assert L.nm_vae_last_timing(None) == B.NM_ERR_ARG
    buf, two, idx = np.full(4, SENT), np.full(2, -7.25), np.zeros(1, dtype=np.int64)
    ip, dp = idx.ctypes.data_as(B.c_int64_p), two.ctypes.data_as(B.c_double_p)
    for fn, rc in (('nm_vae_destroy', L.nm_vae_destroy(None)), ('nm_vae_set_params', L.nm_vae_set_params(None, _p(buf))),
                   ('nm_vae_get_params', L.nm_vae_get_params(None, _p(buf))), ('nm_vae_data', L.nm_vae_data(None, 1, _p(buf))),
                   ('nm_vae_eval', L.nm_vae_eval(None, 1, ip, None, _p(buf), _p(buf), None, _p(buf), _p(buf))),
                   ('nm_vae_grad', L.nm_vae_grad(None, 1, ip, None, _p(buf), dp)), ('nm_vae_epoch', L.nm_vae_epoch(None, 1, ip, None, 1, 1e-3, dp))):
        assert rc == B.NM_ERR_ARG, fn
    assert L.nm_vae_last_error().decode() == 'nm_vae_epoch: ctx is null'
    assert (buf == SENT).all() and (two == -7.25).all()


def test_the_error_channel_is_the_stage_s_own():
    L = B.load()
    assert call_conv(stride=3)[0] == B.NM_ERR_ARG
    mine = L.nm_vae_last_error().decode()
    assert L.nm_pca_last_timing(None) == B.NM_ERR_ARG
    assert L.nm_vae_last_error().decode() == mine and L.nm_pca_last_error().decode().startswith('nm_pca_last_timing')


# ---- the restatement itself
@pytest.mark.parametrize('side', [2, 3, 4])
def test_stride2_maps_are_adjoint(side):
    """<conv(x), g> == <x, convT(g)> for the stride-2 convolution with w, and convT is exactly autograd's adjoint"""
    rng = np.random.default_rng(side)
    x = torch.as_tensor(rng.standard_normal((2, 3, 2 * side, 2 * side, 2 * side))).requires_grad_(True)
    w = torch.as_tensor(rng.standard_normal((3, 3, 3, 3, 5)))             # conv layout (k, cin 3, cout 5) = transposed layout (k, cout 3, cin 5)
    g = torch.as_tensor(rng.standard_normal((2, 5, side, side, side)))
    y = R.conv_t(x, w, 2, False)
    assert y.shape == g.shape
    (adj,) = torch.autograd.grad(y, x, g)
    back = R.conv_t(g, w, 2, True)
    assert back.shape == x.shape
    assert torch.equal(back, adj)
    assert abs(float((y.detach() * g).sum() - (x.detach() * back).sum())) <= 1e-12 * float((y.detach() * g).abs().sum())
    # before / after padding is not symmetric: reflecting the input does not reflect the output
    assert not torch.allclose(R.conv_t(x.detach().flip(4), w.flip(2), 2, False), y.detach().flip(4))


def test_nadam_matches_the_formula_by_hand():
    theta0, g1, g2, lr = np.array([0.5, -1.25]), np.array([0.3, -0.02]), np.array([-0.1, 0.4]), 1e-3
    opt = R.Nadam(theta0)
    got1 = opt.step(g1, lr).copy()
    got2 = opt.step(g2, lr).copy()
    b1, b2, eps = 0.9, 0.999, 1e-7
    mc1, mc2, mc3 = (b1 * (1 - 0.5 * 0.96 ** (0.004 * t)) for t in (1, 2, 3))
    M = mc1
    m = (1 - b1) * g1
    v = (1 - b2) * g1 ** 2
    want1 = theta0 - lr * ((1 - mc1) * g1 / (1 - M) + mc2 * m / (1 - M * mc2)) / (np.sqrt(v / (1 - b2)) + eps)
    np.testing.assert_allclose(got1, want1, rtol=1e-14)
    M = M * mc2
    m = b1 * m + (1 - b1) * g2
    v = b2 * v + (1 - b2) * g2 ** 2
    want2 = want1 - lr * ((1 - mc2) * g2 / (1 - M) + mc3 * m / (1 - M * mc3)) / (np.sqrt(v / (1 - b2 ** 2)) + eps)
    np.testing.assert_allclose(got2, want2, rtol=1e-14)


def test_gradient_matches_central_differences():
    S, LD, n = 4, 2, 2
    rng = np.random.default_rng(11)
    theta = 0.2 * rng.standard_normal(R.nparams(S, LD))
    x, eps = rng.random((n, S, S, S)), rng.standard_normal((n, LD))
    g, _ = R.gradient(theta, S, LD, x, eps)
    off = R.offsets(S, LD)

    def loss(t):
        _, _, _, rec, kl = R.evaluate(t, S, LD, x, eps)
        return float((rec + kl).mean())
    for i in range(26):                                                   # two entries of every tensor
        for j in {int(off[i]), int(off[i] + (off[i + 1] - off[i]) // 2)}:
            h = 1e-6
            tp, tm = theta.copy(), theta.copy()
            tp[j] += h
            tm[j] -= h
            fd = (loss(tp) - loss(tm)) / (2 * h)
            # the loss is piecewise smooth: of the ~10^4 relu units a few change side within +-h and shift the quotient by a share
            # of their own small contribution; rounding gives 1e-16 * loss / h ~ 1e-8.  A wrong term errs at the order of g itself
            assert abs(fd - g[j]) <= 1e-4 * max(1.0, abs(g[j])), (i, j, fd, g[j])


def test_layer_gradients_of_the_restatement_are_autograd_s():
    rng = np.random.default_rng(2)
    x, w, b = rng.standard_normal((2, 4, 4, 4, 3)), rng.standard_normal((3, 3, 3, 3, 5)), rng.standard_normal(5)
    y = R.conv(x, w, b, 2, False, R.RELU)
    gy = rng.standard_normal(y.shape)
    gx, gw, gb = R.conv_grad(x, w, y, gy, 2, False, R.RELU)
    xt, wt, bt = (torch.as_tensor(v).requires_grad_(True) for v in (x, w, b))
    out = torch.relu(R.conv_t(xt.permute(0, 4, 1, 2, 3), wt, 2, False) + bt.view(1, -1, 1, 1, 1))
    ax, aw, ab = torch.autograd.grad(out, (xt, wt, bt), torch.as_tensor(gy).permute(0, 4, 1, 2, 3))
    np.testing.assert_allclose(gx, ax.numpy(), atol=1e-13)
    np.testing.assert_allclose(gw, aw.numpy(), atol=1e-13)
    np.testing.assert_allclose(gb, ab.numpy(), atol=1e-13)


# ---- a guard on the case lists of tests/test_vae_forms_gpu.py, not an oracle: vae_split, wgrad_split and bgrad_split of nm_vae_api.hip
# restated, and every edge of a split that those cases are there to reach.  It fails when the constants change and the cases
# silently stop covering an edge.
def vae_split(count, most, even):
    """(L, chunks): count positions in chunks of L consecutive ones, at most `most` of them; even: L is even"""
    L = -(-count // most)
    if even:
        L = max(2, L + (L & 1))
    L = max(L, 1)
    return L, -(-count // L)


def splits_of(case):
    """(count, L, chunks, on the matrix unit) of the weight gradient's split, (rows, L, chunks) of the bias gradient's"""
    cin, cout, stride, tr, side, n = case
    so = side * stride if tr else side // stride
    mfma = cin % 32 == 0 and cout % 32 == 0
    count, rows = n * min(side, so) ** 3, n * so ** 3
    return (count,) + vae_split(count, 32 if mfma else 256, mfma) + (mfma,), (rows,) + vae_split(rows, 256, False)


def test_the_forms_cases_reach_every_edge_of_the_splits():
    from test_vae_forms_gpu import CUBE_CASES, PLAIN_CASES
    txt = open(os.path.join(ROOT, 'neuralmelting_amd', 'csrc', 'nm_vae.h')).read()
    assert re.search(r'VAE_WG_CHUNKS_MFMA = 32, VAE_WG_CHUNKS_PLAIN = 256, VAE_BG_CHUNKS = 256;', txt)
    wg, bg = zip(*[splits_of(c) for c in CUBE_CASES + PLAIN_CASES])
    both = [(count, L, chunks) for count, L, chunks, _ in wg] + list(bg)
    for count, L, chunks in both:
        assert (chunks - 1) * L < count <= chunks * L and chunks <= 256
    assert all(L % 2 == 0 and chunks <= 32 for _, L, chunks, mfma in wg if mfma)
    reached = {
        'a single chunk, matrix unit': any(mfma and chunks == 1 for _, _, chunks, mfma in wg),
        'a single chunk, plain': any(not mfma and chunks == 1 for _, _, chunks, mfma in wg),
        'a single chunk, bias': any(chunks == 1 for _, _, chunks in bg),
        'a ragged last sixteen in the sum of the chunks, matrix unit': any(mfma and chunks > 16 and chunks % 16 for _, _, chunks, mfma in wg),
        'a ragged last sixteen in the sum of the chunks, plain': any(not mfma and chunks > 16 and chunks % 16 for _, _, chunks, mfma in wg),
        'a ragged last sixteen in the sum of the chunks, bias': any(chunks > 16 and chunks % 16 for _, _, chunks in bg),
        'fewer than sixteen chunks but more than one': any(1 < chunks < 16 for _, _, chunks in both),
        'all 32 chunks of the matrix unit': any(mfma and chunks == 32 for _, _, chunks, mfma in wg),
        'a last chunk shorter than L, matrix unit': any(mfma and count % L for count, L, _, mfma in wg),
        'a last chunk shorter than L, plain': any(not mfma and count % L for count, L, _, mfma in wg),
        'a last chunk shorter than L, bias': any(rows % L for rows, L, _ in bg),
        # L is even and the two half-waves take alternate positions: an odd count ends on the low half-wave, the high one's is masked
        'an odd position count under the even-L rule, one chunk': any(mfma and count % 2 and chunks == 1 for count, _, chunks, mfma in wg),
        'an odd position count under the even-L rule, 32 chunks': any(mfma and count % 2 and chunks == 32 for count, _, chunks, mfma in wg),
        'a plain split with L >= 2': any(not mfma and L >= 2 for _, L, _, mfma in wg),
        'a bias split with L >= 2': any(L >= 2 for _, L, _ in bg),
    }
    assert all(reached.values()), [k for k, v in reached.items() if not v]


def test_command_line_refusals(tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    for argv in (['-ld', '0'], ['-ld', '65'], ['-bs', '0'], ['-vf', '1.0'], ['-lr', '0'], ['-sc', 'tanh'], ['-ep', '0']):
        with pytest.raises(SystemExit):
            vae.parse_args(argv)
    with pytest.raises(SystemExit) as e:
        vae.main(['-n', 'nothing'])
    assert 'is missing' in str(e.value)
    pre = vae.S.prefix('run', 'LJ')
    np.save(pre + '.virial.trgt.npy', np.float32([1, 2]))
    np.save(pre + '.temp.trgt.npy', np.float32([1, 2, 3]))
    np.save(pre + '.pe.npy', np.zeros((2, 3, 4)))
    np.save(pre + '.cdf.npy', np.zeros((2, 3, 4, 11, 11, 11), dtype=np.float32))
    with pytest.raises(SystemExit) as e:
        vae.main(['-n', 'run'])
    assert 'side 11' in str(e.value) and '11 -> 6 -> 3 -> 6 -> 12' in str(e.value)
    np.save(pre + '.cdf.npy', np.zeros((2, 3, 4, 8, 8), dtype=np.float32))
    with pytest.raises(SystemExit) as e:
        vae.main(['-n', 'run'])
    assert 'cube' in str(e.value)
