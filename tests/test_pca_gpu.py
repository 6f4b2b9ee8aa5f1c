"""The principal component stage on the GPU (include/nm_pca.h): nm_pca_moments and nm_pca_project on sentinel-filled outputs
against tests/pca_ref.py within the header's error bounds (evaluated in longdouble), exact on integer data, at every ragged
edge of the tile, the instruction, the slice and the batch; and neuralmelting_amd.pca end to end on a synthetic grid."""
import functools
import os

import numpy as np
import pytest

import pca_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import pca, reweight

pytestmark = pytest.mark.gpu

SENT = -7.25e300
TILE, SL, SLICES, BATCH = 64, 4096, 8, 32768        # csrc/nm_pca.h: the Gram tile, the slice of a batch, the slices, the batch
LD = np.longdouble


def raw_moments(x):
    """the raw ABI on sentinel-filled outputs: rc, message, (mean, lo, hi, gram)"""
    L = B.load()
    n, d = x.shape
    out = (np.full(d, SENT), np.full(d, SENT), np.full(d, SENT), np.full((d, d), SENT))
    rc = L.nm_pca_moments(0, n, d, x.ctypes.data_as(B.c_float_p), *[o.ctypes.data_as(B.c_double_p) for o in out])
    return rc, (L.nm_pca_last_error().decode() if rc else ''), out


def raw_project(x, mean, inv, comp, want_norm2=True):
    L = B.load()
    n, d = x.shape
    z, norm2 = np.full((n, comp.shape[0]), SENT), np.full(n, SENT)
    rc = L.nm_pca_project(0, n, d, x.ctypes.data_as(B.c_float_p), mean.ctypes.data_as(B.c_double_p), inv.ctypes.data_as(B.c_double_p),
                          comp.shape[0], comp.ctypes.data_as(B.c_double_p), z.ctypes.data_as(B.c_double_p),
                          norm2.ctypes.data_as(B.c_double_p) if want_norm2 else None)
    return rc, (L.nm_pca_last_error().decode() if rc else ''), z, norm2


def moments(x):
    rc, msg, out = raw_moments(x)
    assert rc == B.NM_OK, msg
    assert all((o != SENT).all() for o in out)
    return out


def data(n, d, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray((rng.standard_normal((n, d)) * rng.uniform(0.5, 2.0, d) + rng.uniform(-1.0, 1.0, d)).astype(np.float32))


def check_moments(x):
    """mean within its bound of the longdouble mean, lo and hi exact, gram within its bound of the longdouble Gram matrix
    centred on the DEVICE's mean, symmetric bit for bit"""
    n, d = x.shape
    mean, lo, hi, gram = moments(x)
    err, bound = np.abs(LD(mean) - R.mean(x)), R.mean_bound(x)
    print('n %d d %d: mean error / bound %.3g' % (n, d, float((err / np.maximum(bound, LD(1e-300))).max())))
    assert (err <= bound).all()
    np.testing.assert_array_equal(lo, x.min(axis=0).astype(np.float64))
    np.testing.assert_array_equal(hi, x.max(axis=0).astype(np.float64))
    ref, absref = R.gram(x, mean)
    err, bound = np.abs(LD(gram) - ref), R.gram_bound(n, absref)
    print('n %d d %d: gram error / bound %.3g' % (n, d, float((err / np.maximum(bound, LD(1e-300))).max())))
    assert (err <= bound).all()
    assert np.array_equal(gram, gram.T)
    return mean, lo, hi, gram


# ---- exact data
@pytest.mark.parametrize('rows,d', ((65, 2 * TILE + 3), (SL + 3, TILE + 6), (5, 1)))
def test_integer_data_gives_the_integer_gram_matrix(rows, d):
    """every row is followed by its negation: the means are exactly 0 and every sum is one of integers below 2^53.  With more than
    one tile in each direction the off-diagonal tiles are asymmetric products: a swapped row / column map of the result cannot pass"""
    rng = np.random.default_rng(rows)
    half = rng.integers(-100, 101, (rows, d))
    xi = np.stack([half, -half], axis=1).reshape(2 * rows, d)
    mean, lo, hi, gram = moments(np.ascontiguousarray(xi, dtype=np.float32))
    assert (mean == 0.0).all()
    np.testing.assert_array_equal(gram, (xi.T.astype(np.int64) @ xi.astype(np.int64)).astype(np.float64))
    np.testing.assert_array_equal(lo, xi.min(axis=0).astype(np.float64))
    np.testing.assert_array_equal(hi, xi.max(axis=0).astype(np.float64))


# ---- ragged shapes
@pytest.mark.parametrize('d', (1, 15, 16, 17, 33, TILE - 1, TILE, TILE + 1, 2 * TILE + 3))
def test_ragged_features(d):
    check_moments(data(257, d, 100 + d))


@pytest.mark.parametrize('n', (2, 3, 4, 5, 63, 64, 65))
def test_ragged_samples(n):
    check_moments(data(n, 37, 200 + n))


@pytest.mark.parametrize('n', (SL - 1, SL, SL + 1, BATCH + 3))
def test_slice_and_batch_edges(n):
    check_moments(data(n, 5, 300 + n % 97))


# ---- cancellation
def test_offset_columns_and_a_constant_column():
    rng = np.random.default_rng(7)
    x = (50.0 + 0.1 * rng.standard_normal((1000, 7))).astype(np.float32)
    x[:, 3] = np.float32(0.1)
    x = np.ascontiguousarray(x)
    mean, lo, hi, gram = check_moments(x)
    assert mean[3] == float(np.float32(0.1)) and lo[3] == hi[3] == mean[3]
    assert (gram[3] == 0.0).all() and (gram[:, 3] == 0.0).all()
    assert (np.diag(gram)[[0, 1, 2, 4, 5, 6]] > 0.0).all()


# ---- symmetry and determinism
def test_two_calls_give_the_same_bytes_and_a_symmetric_matrix():
    x = data(SL + 77, 2 * TILE + 3, 11)
    a, b = moments(x), moments(x)
    for p, q in zip(a, b):
        assert p.tobytes() == q.tobytes()
    assert np.array_equal(a[3], a[3].T)
    mean, inv = a[0], np.full(x.shape[1], 0.5)
    comp = np.linalg.qr(np.random.default_rng(3).standard_normal((x.shape[1], 9)))[0].T.copy()
    za, zb = raw_project(x, mean, inv, comp), raw_project(x, mean, inv, comp)
    assert za[0] == zb[0] == B.NM_OK
    assert za[2].tobytes() == zb[2].tobytes() and za[3].tobytes() == zb[3].tobytes()


def test_a_resident_x_and_an_uploaded_one_give_the_same_bytes(monkeypatch):
    """x kept on the device between the two passes, or uploaded batch by batch again (NM_PCA_STREAM=1): the same batches"""
    x = data(BATCH + SL + 5, 5, 12)
    a = moments(x)
    comp = np.eye(5)[:2].copy()
    za = raw_project(x, a[0], np.ones(5), comp)
    monkeypatch.setenv('NM_PCA_STREAM', '1')
    b = moments(x)
    zb = raw_project(x, a[0], np.ones(5), comp)
    for p, q in zip(a, b):
        assert p.tobytes() == q.tobytes()
    assert za[0] == zb[0] == B.NM_OK and za[2].tobytes() == zb[2].tobytes() and za[3].tobytes() == zb[3].tobytes()


# ---- projection
@functools.lru_cache(maxsize=None)
def projection_case(d, n):
    """x, mean, inv_scale, the most components the shape allows, and the longdouble results for them: computed once per shape"""
    rng = np.random.default_rng(1000 * d + n)
    x = data(n, d, 400 + d + n)
    mean = x.mean(axis=0, dtype=np.float64) + 1e-3 * rng.standard_normal(d)
    inv = 1.0 / rng.uniform(0.5, 2.0, d)
    comp = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((d, min(d, 64))))[0].T)
    z, norm2, absz = R.project(x, mean, inv, comp)
    for a in (x, mean, inv, comp, z, norm2, absz):
        a.setflags(write=False)
    return x, mean, inv, comp, z, norm2, absz


@pytest.mark.parametrize('n', (2, 65, 4099))
@pytest.mark.parametrize('nc', (1, 8, 64))
@pytest.mark.parametrize('d', (1, 63, 64, 65, 1331))
def test_projection_within_its_bounds(d, nc, n):
    if nc > d:
        nc = d                                      # (1 feature: one component, whatever was asked)
    x, mean, inv, comp, z, norm2, absz = projection_case(d, n)
    rc, msg, gz, gn = raw_project(x, mean, inv, np.ascontiguousarray(comp[:nc]))
    assert rc == B.NM_OK, msg
    assert (gz != SENT).all() and (gn != SENT).all()
    ez, bz = np.abs(LD(gz) - z[:, :nc]), R.z_bound(d, absz[:, :nc])
    en, bn = np.abs(LD(gn) - norm2), R.norm2_bound(d, norm2)
    print('d %d nc %d n %d: z error / bound %.3g, norm2 error / bound %.3g' % (
        d, nc, n, float((ez / np.maximum(bz, LD(1e-300))).max()), float((en / np.maximum(bn, LD(1e-300))).max())))
    assert (ez <= bz).all() and (en <= bn).all()


def test_projection_without_norm2():
    x, mean, inv, comp, z, norm2, absz = projection_case(65, 65)
    rc, msg, gz, gn = raw_project(x, mean, inv, np.ascontiguousarray(comp[:8]), want_norm2=False)
    assert rc == B.NM_OK, msg
    assert (gn == SENT).all()
    assert (np.abs(LD(gz) - z[:, :8]) <= R.z_bound(65, absz[:, :8])).all()


# ---- a value that is not finite
@pytest.mark.parametrize('bad', (np.nan, np.inf))
def test_a_value_that_is_not_finite_in_the_last_sample_is_refused(bad):
    x = data(BATCH + 5, 5, 13)
    x[-1, 4] = bad
    rc, msg, out = raw_moments(x)
    assert rc == B.NM_ERR_ARG and msg.startswith('nm_pca_moments:') and 'sample %d' % (BATCH + 4) in msg, msg
    assert all((o == SENT).all() for o in out)
    rc, msg, z, norm2 = raw_project(x, np.zeros(5), np.ones(5), np.eye(5)[:2].copy())
    assert rc == B.NM_ERR_ARG and msg.startswith('nm_pca_project:') and 'sample %d' % (BATCH + 4) in msg, msg
    assert (z == SENT).all() and (norm2 == SENT).all()
    x[5, 0] = bad                                   # the first of two is named
    rc, msg, out = raw_moments(x)
    assert rc == B.NM_ERR_ARG and 'sample 5' in msg and all((o == SENT).all() for o in out)


# ---- end to end
PN, TN, SN, FEAT, NLD = 2, 4, 64, (3, 3, 3), 4


@functools.lru_cache(maxsize=None)
def grid():
    """cold columns (t = 0, 1) around one pattern, hot ones (t = 2, 3) around another, planted variances 16, 9, 4, 1 over noise 0.01"""
    rng = np.random.default_rng(21)
    d = int(np.prod(FEAT))
    q = np.linalg.qr(rng.standard_normal((d, d)))[0][:4]
    centre = np.where(np.arange(TN)[None, :, None, None] >= 2, 2.0, -2.0) * q[0] + 10.0
    g = rng.standard_normal((PN, TN, SN, 4)) * np.sqrt([16.0, 9.0, 4.0, 1.0])
    x = centre + g @ q + 0.1 * rng.standard_normal((PN, TN, SN, d))
    x = x.astype(np.float32).reshape((PN, TN, SN) + FEAT)
    x.setflags(write=False)
    return x


@pytest.mark.parametrize('scaler', pca.SCALERS)
def test_the_stage_end_to_end(scaler, tmp_path, monkeypatch, capsys):
    feat, T = grid(), np.linspace(0.5, 2.0, TN, dtype=np.float32)
    prefix = str(tmp_path / 'pc.lj.fcc.lammps')
    np.save(prefix + '.virial.trgt.npy', np.linspace(1, 2, PN, dtype=np.float32))
    np.save(prefix + '.temp.trgt.npy', T)
    pe = np.random.default_rng(2).random((PN, TN, SN)).astype(np.float32)
    np.save(prefix + '.pe.npy', pe)
    np.save(prefix + '.cdf.npy', feat)
    monkeypatch.chdir(tmp_path)
    assert pca.main(['-v', '-n', 'pc', '-sc', scaler, '-ld', str(NLD)]) == 0
    assert 'explained variance' in capsys.readouterr().out
    got = {key: np.load(prefix + '.cdf.%s.npy' % key) for key in pca.SUFFIXES}
    ref = R.pipeline(feat, T, scaler, NLD)
    d, n = int(np.prod(FEAT)), PN * TN * SN
    x = np.asarray(feat, dtype=np.float32).reshape(n, d)
    assert all(v.dtype == np.float64 for v in got.values())
    assert got['pcz'].shape == (PN, TN, SN, NLD) and got['pcr'].shape == pe.shape and got['pcc'].shape == (NLD, d) and got['pcv'].shape == (2, NLD)

    # the moments' bounds at the reference's values, and what they make of the covariance
    mb = R.mean_bound(x)
    assert (np.abs(LD(got['pcm']) - R.mean(x)) <= mb).all()
    g, absg = R.gram(x, got['pcm'])
    gb = R.gram_bound(n, absg)
    s = ref['pcs']
    ds = np.asarray(gb.diagonal() / np.maximum(g.diagonal(), LD(1e-300)) / 2 + 2 * R.U, dtype=np.float64) if scaler == 'standard' else np.zeros(d)
    if scaler == 'standard':
        assert (np.abs(got['pcs'] - s) <= ds * s).all()
    else:
        np.testing.assert_array_equal(got['pcs'], s)
    g64 = np.asarray(g, dtype=np.float64)
    ecov = (np.asarray(gb, dtype=np.float64) + np.abs(g64) * (ds[:, None] + ds[None, :])) / (np.outer(s, s) * (n - 1))
    w = np.linalg.eigvalsh(g64 / (np.outer(s, s) * (n - 1)))[::-1]
    gap = min(min(w[c - 1] - w[c] if c else np.inf, w[c] - w[c + 1]) for c in range(NLD))
    enorm = float(np.sqrt((ecov * ecov).sum()))
    tol_c = 2.0 * enorm / gap + 64 * float(R.U)
    tol_w = enorm + 64 * float(R.U) * w[0]
    print('%s: gap %.3g of %.3g, component tolerance %.3g, errors: components %.3g eigenvalues %.3g' % (
        scaler, gap, w[0], tol_c, np.abs(got['pcc'] - ref['pcc']).max(), np.abs(got['pcv'][0] - ref['pcv'][0]).max()))
    assert gap > 0.02 * w[0]
    assert np.abs(got['pcc'] - ref['pcc']).max() <= tol_c
    assert np.abs(got['pcv'][0] - ref['pcv'][0]).max() <= tol_w
    trace = w.sum()
    assert (np.abs(got['pcv'][1] - ref['pcv'][1]) <= (tol_w + ref['pcv'][1] * np.sqrt(d) * tol_w) / trace + 8 * float(R.U)).all()

    # the projections: the components' tolerance, the mean's and the scale's, and the kernel's own bound
    y = (x.astype(np.float64) - ref['pcm']) / s
    _, norm2, absz = R.project(x, ref['pcm'], 1.0 / s, ref['pcc'])
    absy = np.abs(y)
    shift = np.asarray(mb, dtype=np.float64) / s
    tol_z = (tol_c * np.sqrt((y * y).sum(axis=1))[:, None] + np.asarray(R.z_bound(d, absz), dtype=np.float64) + (shift + absy * ds) @ np.abs(ref['pcc']).T
             + 4 * float(R.U) * np.asarray(absz, dtype=np.float64))
    ez = np.abs(got['pcz'].reshape(n, NLD) - ref['pcz'].reshape(n, NLD))
    print('%s: largest projection error / tolerance %.3g' % (scaler, (ez / tol_z).max()))
    assert (ez <= tol_z).all()
    n2 = np.asarray(norm2, dtype=np.float64)
    tol_r = (np.asarray(R.norm2_bound(d, norm2), dtype=np.float64) + 2.0 * (absy * (shift + absy * ds)).sum(axis=1)
             + 2.0 * (np.abs(ref['pcz'].reshape(n, NLD)) * tol_z).sum(axis=1) + 16 * float(R.U) * n2)
    assert (np.abs(got['pcr'].reshape(n) - ref['pcr'].reshape(n)) <= tol_r).all()
    assert (got['pcr'] > -tol_r.reshape(pe.shape)).all()

    # liquid is positive, every component is a file of .pe.npy's shape that reweight takes
    pc0 = np.load(prefix + '.cdf.pc0.npy')
    assert pc0[:, 2:].mean() > pc0[:, :2].mean() and pc0[:, -1].mean() > pc0[:, 0].mean()
    for c in range(NLD):
        np.testing.assert_array_equal(np.load(prefix + '.cdf.pc%d.npy' % c), got['pcz'][..., c])
    assert not os.path.exists(prefix + '.cdf.pc%d.npy' % NLD)
    obs = reweight.load_observables(prefix, ['cdf.pc0'], pe.shape)
    np.testing.assert_array_equal(obs[0], pc0)
