"""Every form of the VAE stage's kernels (neuralmelting_amd/csrc/nm_vae.h) through the layer primitives, at shapes and sides that the
network itself never runs, against tests/vae_ref.py: exact on integers, within the header's any-order bound on floats.

The matrix-unit cube (CUBE_CASES): all 16 layers (cin, cout) in {32, 64}^2 x stride {1, 2} x transposed {0, 1}.  A layer's forward
is nm_vae_gather_mfma_kernel<cin, transposed, stride> with co = cout, its data gradient <cout, !transposed, stride> with co = cin
(co = 32: blockIdx.y 0 only; co = 64: 0 and 1), its weight gradient nm_vae_wgrad_mfma_kernel with (cb, cs) = (cin, cout), transposed:
(cout, cin):

    layer (cin, cout, stride, transposed)   forward <CR, ADJ, STRIDE>, co    gx <CR, ADJ, STRIDE>, co    wgrad (cb, cs)
    (32, 32, 1, 0)                          <32, 0, 1>, 32                   <32, 1, 1>, 32              (32, 32)
    (32, 64, 1, 0)                          <32, 0, 1>, 64                   <64, 1, 1>, 32              (32, 64)
    (64, 32, 1, 0)                          <64, 0, 1>, 32                   <32, 1, 1>, 64              (64, 32)
    (64, 64, 1, 0)                          <64, 0, 1>, 64                   <64, 1, 1>, 64              (64, 64)
    (32, 32, 2, 0)                          <32, 0, 2>, 32                   <32, 1, 2>, 32              (32, 32)
    (32, 64, 2, 0)                          <32, 0, 2>, 64                   <64, 1, 2>, 32              (32, 64)
    (64, 32, 2, 0)                          <64, 0, 2>, 32                   <32, 1, 2>, 64              (64, 32)
    (64, 64, 2, 0)                          <64, 0, 2>, 64                   <64, 1, 2>, 64              (64, 64)
    (32, 32, 1, 1)                          <32, 1, 1>, 32                   <32, 0, 1>, 32              (32, 32)
    (32, 64, 1, 1)                          <32, 1, 1>, 64                   <64, 0, 1>, 32              (64, 32)
    (64, 32, 1, 1)                          <64, 1, 1>, 32                   <32, 0, 1>, 64              (32, 64)
    (64, 64, 1, 1)                          <64, 1, 1>, 64                   <64, 0, 1>, 64              (64, 64)
    (32, 32, 2, 1)                          <32, 1, 2>, 32                   <32, 0, 2>, 32              (32, 32)
    (32, 64, 2, 1)                          <32, 1, 2>, 64                   <64, 0, 2>, 32              (64, 32)
    (64, 32, 2, 1)                          <64, 1, 2>, 32                   <32, 0, 2>, 64              (32, 64)
    (64, 64, 2, 1)                          <64, 1, 2>, 64                   <64, 0, 2>, 64              (64, 64)

So each of the eight instantiations runs forward with co = 32 and 64 and as a data gradient with co = 32 and 64, and each of the four
(cb, cs) in both layouts.  Every row runs (test_matrix_unit_cube_is_exact_on_integers) at the smaller grid's sides 1, 3, 5 and n = 1, 3
with the epilogue act NONE, RELU and TANH forward and the prologue act' of NONE, RELU and TANH in gx, gw and gb.

The plain forms (PLAIN_CASES, test_plain_forms_are_exact_on_integers) at channel counts that are not the network's; floats on a
subset of both (test_forms_on_floats); the dense kernels at the edges of their index ranges and of VAE_DENSE_WIDE."""
import numpy as np
import pytest

import vae_ref as R
from test_vae_gpu import SENT, f32, gamma, gpu_conv, gpu_conv_grad, gpu_dense, gpu_dense_grad, within

pytestmark = pytest.mark.gpu

ACTS = (R.NONE, R.RELU, R.TANH)


def sides_of(stride, transposed, small):
    """(side_in, side_out) of a layer whose smaller grid has the side `small`"""
    if transposed:
        return small, small * stride
    return small * stride, small


# a case is (cin, cout, stride, transposed, side_in, n); these lists import without a device (tests/test_vae.py reads them)
CUBE_CASES = [(cin, cout, stride, tr, sides_of(stride, tr, small)[0], n)
              for tr in (0, 1) for stride in (1, 2) for cin in (32, 64) for cout in (32, 64) for small in (1, 3, 5) for n in (1, 3)]

# what each pair of channel counts is there for (cr is the reduced count: cin forward, cout in gx; C = cout in bgrad, whose tree
# starts with 256 / C partial rows):
#   (1, 1)    the scalar gather both ways, cr = 1; plain wgrad 1 x 1; bgrad 256 rows, every level even
#   (3, 5)    the scalar gather with cr = 3 and cr = 5; bgrad 51 -> 26 -> 13 -> 7 -> 4, one thread idle
#   (4, 3)    the float4 gather with a single group (cr = 4) forward, scalar cr = 3 in gx; bgrad 85 -> 43 -> 22 -> 11 -> 6 -> 3
#   (12, 20)  float4 at cr = 12 and cr = 20; bgrad 12 -> 6 -> 3 -> 2, 16 threads idle
#   (20, 12)  the same the other way round; bgrad 21 -> 11 -> 6 -> 3 -> 2, 4 threads idle
#   (8, 33)   float4 cr = 8 forward, scalar cr = 33 in gx; bgrad 7 -> 4 -> 2 with 25 threads idle
#   (33, 8)   scalar cr = 33 forward, float4 cr = 8 in gx; bgrad 32 rows
#   (32, 48)  cr = 32 but co % 32 != 0: the plain float4 gather where the matrix unit is refused; gx with cr = 48 and co = 32;
#             plain wgrad beside an MFMA-eligible side (32); bgrad 5 -> 3 -> 2, 16 threads idle
#   (48, 32)  cr = 48 with co = 32 forward, cr = 32 with co = 48 in gx; plain wgrad with the eligible side on the right; bgrad 8 rows
#   (63, 64)  scalar cr = 63 forward, cr = 64 with co = 63 in gx (plain float4); plain wgrad 63 x 64; bgrad 4 rows
#   (64, 63)  the same the other way round; bgrad 4 rows with 4 threads idle
PLAIN_PAIRS = ((1, 1), (3, 5), (4, 3), (12, 20), (20, 12), (8, 33), (33, 8), (32, 48), (48, 32), (63, 64), (64, 63))
PLAIN_CASES = [(cin, cout, stride, tr, sides_of(stride, tr, small)[0], n)
               for cin, cout in PLAIN_PAIRS for tr in (0, 1) for stride in (1, 2) for small, n in ((3, 3), (1, 1))]
# the plain wgrad splits n small^3 positions into at most 256 chunks, so only more than 256 positions give a chunk of L >= 2:
# 3 * 5^3 = 375 is L = 2 in 188 chunks, the last one short
PLAIN_CASES += [(3, 5, stride, tr, sides_of(stride, tr, 5)[0], 3) for tr in (0, 1) for stride in (1, 2)]


def case_id(case):
    return '%d-%d-s%d-%s-side%d-n%d' % (case[0], case[1], case[2], 'convT' if case[3] else 'conv', case[4], case[5])


def case_data(case, integer, seed):
    """x, w, b, gy of a layer; integer: |x|, |gy| <= 4 and |w|, |b| <= 3"""
    cin, cout, stride, tr, side, n = case
    so = side * stride if tr else side // stride
    rng = np.random.default_rng(seed)
    wshape = (3, 3, 3, cout, cin) if tr else (3, 3, 3, cin, cout)
    if integer:
        draw = lambda shape, m: f32(rng.integers(-m, m + 1, shape))
        return draw((n, side, side, side, cin), 4), draw(wshape, 3), draw(cout, 3), draw((n, so, so, so, cout), 4)
    draw = lambda shape: f32(rng.standard_normal(shape))
    return draw((n, side, side, side, cin)), draw(wshape) * np.float32(0.1), draw(cout), draw((n, so, so, so, cout))


# ---- exact on integers.  |x|, |gy| <= 4 and |w|, |b| <= 3; y is the forward's result for NONE and RELU (act' is 0 or 1) and an
# integer in -2..2 for TANH (the API takes y as given; 1 - y^2 is 1, 0 or -3), so |gy act'| <= 12 is an integer.  Every partial sum is
# then an integer below 2^24: forward at most 27 * 64 + 1 = 1729 terms of at most 12, gx at most 27 * 64 terms of at most 36, gw at
# most 3 * 10^3 terms of at most 48, gb at most 3 * 10^3 terms of at most 12.  So the result is the restatement's whatever the order,
# and only tanh's own rounding is left in the TANH forward: 2 ulp of the result by the header, the pre-activation being exact.
def exact_case(case, seed):
    cin, cout, stride, tr, side, n = case
    x, w, b, gy = case_data(case, True, seed)
    rng = np.random.default_rng(seed + 1)
    for act in ACTS:
        ref = R.conv(x, w, b, stride, tr, act)
        y = gpu_conv(x, w, b, stride, tr, act)
        assert np.array_equal(gpu_conv(x, w, b, stride, tr, act), y)                          # the same call, the same bits
        if act == R.TANH:
            assert (np.abs(y.astype(np.float64) - ref) <= 2.0 ** -22 * np.abs(ref)).all()
            y = f32(rng.integers(-2, 3, ref.shape))
        else:
            np.testing.assert_array_equal(y, ref)
        gx, gw, gb = gpu_conv_grad(x, w, y, gy, stride, tr, act)
        rx, rw, rb = R.conv_grad(x, w, y, gy, stride, tr, act)
        np.testing.assert_array_equal(gx, rx)
        np.testing.assert_array_equal(gw, rw)
        np.testing.assert_array_equal(gb, rb)
        gx2, gw2, gb2 = gpu_conv_grad(x, w, y, gy, stride, tr, act)
        assert np.array_equal(gx2, gx) and np.array_equal(gw2, gw) and np.array_equal(gb2, gb)
        gx0, gw0, gb0 = gpu_conv_grad(x, w, y, gy, stride, tr, act, want_gx=False)            # gx may be null
        assert (gx0 == SENT).all() and np.array_equal(gw0, gw) and np.array_equal(gb0, gb)


@pytest.mark.parametrize('case', CUBE_CASES, ids=case_id)
def test_matrix_unit_cube_is_exact_on_integers(case):
    exact_case(case, 7 + CUBE_CASES.index(case))


@pytest.mark.parametrize('case', PLAIN_CASES, ids=case_id)
def test_plain_forms_are_exact_on_integers(case):
    exact_case(case, 5000 + PLAIN_CASES.index(case))


# ---- floats: one layer for each way into the three instantiations that the network never reaches: <32, 0, 1> forward (co = 32) and
# as a data gradient (co = 64), <32, 1, 2> forward (co = 64) and as a data gradient (co = 32 and 64), <64, 0, 2> forward (co = 32 and
# 64) and as a data gradient (co = 32); and three of the plain pairs.  The smaller grid's side is 5 and n = 3.
FLOAT_LAYERS = ((32, 32, 1, 0), (64, 32, 1, 1), (32, 64, 2, 1), (32, 32, 2, 0), (64, 64, 2, 0), (64, 32, 2, 0))
FLOAT_CASES = [l + (sides_of(l[2], l[3], 5)[0], 3) for l in FLOAT_LAYERS]
FLOAT_CASES += [(cin, cout, stride, tr, sides_of(stride, tr, 5)[0], 3) for cin, cout in ((3, 5), (33, 8), (48, 32)) for tr in (0, 1) for stride in (1, 2)]


@pytest.mark.parametrize('act', [R.RELU, R.TANH], ids=['relu', 'tanh'])
@pytest.mark.parametrize('case', FLOAT_CASES, ids=case_id)
def test_forms_on_floats(case, act):
    """within gamma_(K+1) sum |terms| of float64 (include/nm_vae.h), K and the prologue's extra roundings as in
    test_vae_gpu.test_conv_layers_on_floats"""
    cin, cout, stride, tr, side, n = case
    name = case_id(case)
    x, w, b, gy = case_data(case, False, 900 + FLOAT_CASES.index(case))
    so = side * stride if tr else side // stride
    ref = R.conv(x, w, b, stride, tr, act)
    y = gpu_conv(x, w, b, stride, tr, act)
    bound = gamma(27 * cin + 2) * R.conv_abs(x, w, b, stride, tr)
    within('%s activated' % name, y, ref, bound + (2.0 ** -22 * np.abs(ref) if act == R.TANH else 0.0))
    extra = 4 if act == R.TANH else 0
    gx, gw, gb = gpu_conv_grad(x, w, y, gy, stride, tr, act)
    rx, rw, rb = R.conv_grad(x, w, y, gy, stride, tr, act)
    ax, aw, ab = R.conv_grad_abs(x, w, y, gy, stride, tr, act)
    small = min(side, so) ** 3
    within('%s gx' % name, gx, rx, gamma(27 * cout + 1 + extra) * ax)
    within('%s gw' % name, gw, rw, gamma(n * small + 1 + extra) * aw)
    within('%s gb' % name, gb, rb, gamma(n * so ** 3 + 1 + extra) * ab)


# ---- dense: din below the four waves of nm_vae_dense_kernel (the waves sl >= din add nothing), one and two workgroups of 64
# columns, a single column, and dout on both sides of VAE_DENSE_WIDE = 1024, where the data gradient changes kernel
DENSE_SIZES = ((1, 1), (2, 7), (3, 64), (5, 65), (8, 1023), (8, 1024), (8, 1025), (130, 1))


# |x|, |gy| <= 4, |w|, |b| <= 3, |gy act'| <= 12: forward at most 131 terms of 12, gx at most 1025 of 36, gw and gb 3 of 48
@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('din,dout', DENSE_SIZES)
def test_dense_edges_are_exact_on_integers(din, dout, n):
    rng = np.random.default_rng(31 * din + dout + n)
    x, w, b, gy = (f32(rng.integers(-m, m + 1, shape)) for shape, m in (((n, din), 4), ((din, dout), 3), (dout, 3), ((n, dout), 4)))
    for act in ACTS:
        ref = R.dense(x, w, b, act)
        y = gpu_dense(x, w, b, act)
        if act == R.TANH:
            assert (np.abs(y.astype(np.float64) - ref) <= 2.0 ** -22 * np.abs(ref)).all()
            y = f32(rng.integers(-2, 3, ref.shape))
        else:
            np.testing.assert_array_equal(y, ref)
        got = gpu_dense_grad(x, w, y, gy, act)
        for g, want in zip(got, R.dense_grad(x, w, y, gy, act)):
            np.testing.assert_array_equal(g, want)
        gx0, gw0, gb0 = gpu_dense_grad(x, w, y, gy, act, want_gx=False)
        assert (gx0 == SENT).all() and np.array_equal(gw0, got[1]) and np.array_equal(gb0, got[2])


@pytest.mark.parametrize('act', [R.RELU, R.TANH], ids=['relu', 'tanh'])
@pytest.mark.parametrize('din,dout', DENSE_SIZES)
def test_dense_edges_on_floats(din, dout, act):
    """the bounds of test_vae_gpu.test_dense_layers_on_floats; tanh adds its 2 ulp forward and four roundings to the prologue"""
    n = 3
    rng = np.random.default_rng(17 * din + dout)
    x, w, b, gy = (f32(rng.standard_normal(shape)) for shape in ((n, din), (din, dout), dout, (n, dout)))
    ref = R.dense(x, w, b, act)
    y = gpu_dense(x, w, b, act)
    within('dense %d->%d' % (din, dout), y, ref,
           gamma(din + 2) * (np.abs(x).astype(np.float64) @ np.abs(w) + np.abs(b)) + (2.0 ** -22 * np.abs(ref) if act == R.TANH else 0.0))
    extra = 4 if act == R.TANH else 0
    g = np.abs(gy * R.dact(y, act))
    bounds = (gamma(dout + 1 + extra) * (g @ np.abs(w.T)), gamma(n + 1 + extra) * (np.abs(x.T).astype(np.float64) @ g), gamma(n + 1 + extra) * g.sum(axis=0))
    for what, got, want, bound in zip(('gx', 'gw', 'gb'), gpu_dense_grad(x, w, y, gy, act), R.dense_grad(x, w, y, gy, act), bounds):
        within('dense %d->%d %s' % (din, dout, what), got, want, bound)
