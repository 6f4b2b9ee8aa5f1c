"""The manifold stage without a GPU (include/nm_tsne.h, neuralmelting_amd/manifold.py): tests/tsne_ref.py against sklearn's
_kl_divergence and _binary_search_perplexity, the restatement's rows at their root, the interface, every refusal that precedes
the device check on sentinel-filled outputs, and the command lines' checks."""
import ctypes as C
import os

import numpy as np
import pytest

import tsne_ref as R
from test_abi import declared_symbols
from neuralmelting_amd import _lib as B
from neuralmelting_amd import cluster, manifold

U = 2.0 ** -53
SENT = -77.0


def blobs(seed, n, nd, k=3):
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-4.0, 4.0, (k, nd))
    return centre[rng.integers(0, k, n)] + 0.5 * rng.standard_normal((n, nd))


N, K, PX = 300, 61, 20.0


@pytest.fixture(scope='module')
def case():
    x = blobs(1, N, 4)
    nbr, p, beta, d = R.affinities(x, PX, K)
    for a in (x, nbr, p, beta, d):
        a.setflags(write=False)
    return x, nbr, p, beta, d


# ---- the restatement is sklearn's
@pytest.mark.parametrize('exaggeration', (1.0, 12.0))
@pytest.mark.parametrize('nc', (1, 2, 3))
def test_the_gradient_and_kl_are_sklearn_s(case, nc, exaggeration):
    """Both sides form every term from the same doubles with at most 20 roundings and add N of them, each in an order of its own:
    they differ by at most 2 (N + 20) u of the sum of the terms' magnitudes, per component.  Measured at N = 300, k = 61: at most 1.9e-15 of
    the largest component and 3 % of the bound, kl equal to the last digit or the one before.  y has a spread of O(1), so sklearn's clip of Q at 2.2e-16 is far (Q is
    about 1 / N^2) and P = 0 contributes 0 on both sides."""
    tsne = pytest.importorskip('sklearn.manifold._t_sne')
    from scipy.spatial.distance import squareform
    x, nbr, p, beta, d = case
    y = np.random.default_rng(2).standard_normal((N, nc))
    grad, kl, z, mag, klmag = R.gradient(nbr, p, y, exaggeration)
    P = R.dense(nbr, p)
    assert (P == P.T).all() and P.diagonal().max() == 0.0
    skl, sgrad = tsne._kl_divergence(y.ravel(), squareform(P * exaggeration, checks=False), 1.0, N, nc)
    err = np.abs(grad - sgrad.reshape(N, nc))
    print('gradient: largest difference %.3g of the bound, %.3g of the largest component' % ((err / (2 * (N + 20) * U * mag)).max(), err.max() / np.abs(grad).max()))
    assert (err <= 2 * (N + 20) * U * mag).all()
    if exaggeration == 1.0:
        print('kl %.17g, sklearn %.17g' % (kl, skl))
        assert abs(kl - skl) <= 2 * (N + 20) * U * klmag
    assert 0.0 < kl and z > 0.0


def test_the_conditional_p_are_sklearn_s(case):
    """sklearn rounds the distances to float32 and stops at an entropy within 1e-5 of the target, so the two agree to about that
    only: measured 1.1e-5 of a row's largest p at this seed; 4 times that are allowed.  This pins the definition, not the
    arithmetic."""
    utils = pytest.importorskip('sklearn.manifold._utils')
    x, nbr, p, beta, d = case
    sk = np.asarray(utils._binary_search_perplexity(np.ascontiguousarray(d, dtype=np.float32), PX, 0), dtype=np.float64)
    rel = (np.abs(sk - p).max(axis=1) / p.max(axis=1)).max()
    print('conditional p: largest difference %.3g of a row\'s largest p' % rel)
    assert rel <= 4 * 1.1e-5


def test_the_rows_sit_at_their_root(case):
    """|H - ln px| within the header's bound B u (1 + ln k + M2); measured 4.4e-16"""
    x, nbr, p, beta, d = case
    worst = 0.0
    for i in range(N):
        t = d[i] - d[i, 0]
        h = R.entropy(t, beta[i])[0]
        m2 = float((((beta[i] * t) ** 2) * p[i]).sum())
        bound = (int(np.ceil(K / 256)) + 32) * U * (1.0 + np.log(K) + m2)
        assert abs(h - np.log(PX)) <= bound, (i, h - np.log(PX), bound)
        worst = max(worst, abs(h - np.log(PX)))
        assert abs(p[i].sum() - 1.0) <= 33 * U
    print('largest |H - ln px| %.3g' % worst)
    assert (nbr != np.arange(N)[:, None]).all() and (np.diff(d, axis=1) >= 0).all()


def test_a_row_of_equal_distances_has_no_root():
    x = np.array([[0.0, 0.0], [1.0, 0.0], [-1.0, 0.0], [0.0, 1.0], [0.0, -1.0]])           # the centre sees four at distance 1
    nbr, p, beta, d = R.affinities(x, 2.0, 4)
    assert beta[0] == 2.0 ** 200 and (p[0] == 0.25).all() and list(nbr[0]) == [1, 2, 3, 4]
    assert np.isfinite(beta).all() and (np.abs(p.sum(axis=1) - 1.0) < 1e-15).all()


def test_the_update_is_sklearn_s():
    rng = np.random.default_rng(3)
    y, up, ga, g = rng.standard_normal((4, 50, 2))
    ga = np.abs(ga) * 0.02
    y0, up0, ga0 = y.copy(), up.copy(), ga.copy()
    R.update_step(y, up, ga, g, 0.8, 200.0)
    inc = up0 * g < 0.0
    want = np.clip(np.where(inc, ga0 + 0.2, ga0 * 0.8), 0.01, np.inf)
    np.testing.assert_array_equal(ga, want)
    np.testing.assert_array_equal(up, 0.8 * up0 - 200.0 * (g * want))
    np.testing.assert_array_equal(y, y0 + up)
    assert (ga == 0.01).any() and inc.any() and (~inc).any()


# ---- the interface
def test_header_symbols_are_exported_and_bound():
    syms = declared_symbols('nm_tsne.h')
    assert syms == sorted(B.TSNE_SYMBOLS) and len(syms) == 5
    raw = C.CDLL(B.LIB_PATH)
    for s in syms:
        assert hasattr(raw, s), s
    L = B.load()
    assert len(L.nm_tsne_affinities.argtypes) == 9 and len(L.nm_tsne_gradient.argtypes) == 11 and len(L.nm_tsne_descend.argtypes) == 14
    assert L.nm_tsne_last_timing.restype is C.c_int and L.nm_tsne_last_error.restype is C.c_char_p


def _ptr(a, null, name):
    if name in null:
        return None
    return a.ctypes.data_as(B.c_int32_p if a.dtype == np.int32 else B.c_double_p)


def call_affinities(device=0, npoints=6, ndim=2, perplexity=2.0, k=4, null=()):
    L = B.load()
    arr = dict(x=np.random.default_rng(5).random((6, 2)), nbr=np.full((6, 4), int(SENT), np.int32), p=np.full((6, 4), SENT), beta=np.full(6, SENT))
    rc = L.nm_tsne_affinities(device, npoints, ndim, _ptr(arr['x'], null, 'x'), perplexity, k, *[_ptr(arr[n], null, n) for n in ('nbr', 'p', 'beta')])
    return rc, (L.nm_tsne_last_error().decode() if rc else ''), all((arr[n] == SENT).all() for n in ('nbr', 'p', 'beta'))


def _lists():
    nbr = np.array([[1, 2], [0, 2], [0, 1], [0, 1], [3, 0], [4, 0]], dtype=np.int32)
    return dict(nbr=nbr, p=np.full((6, 2), 0.5), y=np.random.default_rng(6).random((6, 2)))


def call_gradient(device=0, npoints=6, k=2, ncomp=2, exaggeration=1.0, null=()):
    L = B.load()
    arr = dict(_lists(), grad=np.full((6, 2), SENT), kl=np.full(1, SENT), z=np.full(1, SENT))
    rc = L.nm_tsne_gradient(device, npoints, k, _ptr(arr['nbr'], null, 'nbr'), _ptr(arr['p'], null, 'p'), ncomp, _ptr(arr['y'], null, 'y'),
                            exaggeration, *[_ptr(arr[n], null, n) for n in ('grad', 'kl', 'z')])
    return rc, (L.nm_tsne_last_error().decode() if rc else ''), all((arr[n] == SENT).all() for n in ('grad', 'kl', 'z'))


def call_descend(device=0, npoints=6, k=2, ncomp=2, niter=3, exaggeration=1.0, momentum=0.5, learning_rate=200.0, null=()):
    L = B.load()
    arr = dict(_lists(), update=np.full((6, 2), SENT), gains=np.full((6, 2), SENT), trace=np.full((3, 3), SENT))
    y0 = arr['y'].copy()
    rc = L.nm_tsne_descend(device, npoints, k, _ptr(arr['nbr'], null, 'nbr'), _ptr(arr['p'], null, 'p'), ncomp, _ptr(arr['y'], null, 'y'),
                           _ptr(arr['update'], null, 'update'), _ptr(arr['gains'], null, 'gains'), niter, exaggeration, momentum, learning_rate,
                           _ptr(arr['trace'], null, 'trace'))
    return rc, (L.nm_tsne_last_error().decode() if rc else ''), (all((arr[n] == SENT).all() for n in ('update', 'gains', 'trace'))
                                                                 and (arr['y'] == y0).all())


BIG = 2 ** 20 + 1
REFUSALS = {
    'aff-npoints1': (call_affinities, dict(npoints=1), 'npoints'), 'aff-npoints0': (call_affinities, dict(npoints=0), 'npoints'),
    'aff-npoints-over': (call_affinities, dict(npoints=BIG), 'npoints'), 'aff-npoints-far': (call_affinities, dict(npoints=2 ** 62), 'npoints'),
    'aff-ndim0': (call_affinities, dict(ndim=0), 'ndim'), 'aff-ndim17': (call_affinities, dict(ndim=17), 'ndim'),
    'aff-k0': (call_affinities, dict(k=0), 'k must'), 'aff-k-n': (call_affinities, dict(k=6, perplexity=2.0), 'k must'),
    'aff-k-over': (call_affinities, dict(npoints=2 ** 20, k=4097, perplexity=5.0), 'k must'),
    'aff-px1': (call_affinities, dict(perplexity=1.0), 'perplexity'), 'aff-px-k': (call_affinities, dict(perplexity=4.0), 'perplexity'),
    'aff-px-nan': (call_affinities, dict(perplexity=np.nan), 'perplexity'), 'aff-px-inf': (call_affinities, dict(perplexity=np.inf), 'perplexity'),
    'aff-px-k1': (call_affinities, dict(k=1, perplexity=1.5), 'perplexity'),
    'aff-null-x': (call_affinities, dict(null=('x',)), 'pointer'), 'aff-null-nbr': (call_affinities, dict(null=('nbr',)), 'pointer'),
    'aff-null-p': (call_affinities, dict(null=('p',)), 'pointer'), 'aff-null-beta': (call_affinities, dict(null=('beta',)), 'pointer'),
    'aff-device': (call_affinities, dict(device=-1), 'device'),
    'grad-npoints1': (call_gradient, dict(npoints=1), 'npoints'), 'grad-npoints-over': (call_gradient, dict(npoints=BIG), 'npoints'),
    'grad-k0': (call_gradient, dict(k=0), 'k must'), 'grad-k-n': (call_gradient, dict(k=6), 'k must'), 'grad-k-over': (call_gradient, dict(npoints=2 ** 20, k=4097), 'k must'),
    'grad-ncomp0': (call_gradient, dict(ncomp=0), 'ncomp'), 'grad-ncomp4': (call_gradient, dict(ncomp=4), 'ncomp'),
    'grad-ex0': (call_gradient, dict(exaggeration=0.0), 'exaggeration'), 'grad-ex-nan': (call_gradient, dict(exaggeration=np.nan), 'exaggeration'),
    'grad-null-nbr': (call_gradient, dict(null=('nbr',)), 'pointer'), 'grad-null-p': (call_gradient, dict(null=('p',)), 'pointer'),
    'grad-null-y': (call_gradient, dict(null=('y',)), 'pointer'), 'grad-null-grad': (call_gradient, dict(null=('grad',)), 'pointer'),
    'grad-null-kl': (call_gradient, dict(null=('kl',)), 'pointer'), 'grad-null-z': (call_gradient, dict(null=('z',)), 'pointer'),
    'grad-device': (call_gradient, dict(device=-1), 'device'),
    'desc-npoints1': (call_descend, dict(npoints=1), 'npoints'), 'desc-k0': (call_descend, dict(k=0), 'k must'), 'desc-ncomp4': (call_descend, dict(ncomp=4), 'ncomp'),
    'desc-niter0': (call_descend, dict(niter=0), 'niter'), 'desc-niter-over': (call_descend, dict(niter=BIG), 'niter'),
    'desc-ex-inf': (call_descend, dict(exaggeration=np.inf), 'exaggeration'), 'desc-momentum1': (call_descend, dict(momentum=1.0), 'momentum'),
    'desc-momentum-neg': (call_descend, dict(momentum=-0.1), 'momentum'), 'desc-lr0': (call_descend, dict(learning_rate=0.0), 'learning_rate'),
    'desc-lr-nan': (call_descend, dict(learning_rate=np.nan), 'learning_rate'),
    'desc-null-y': (call_descend, dict(null=('y',)), 'pointer'), 'desc-null-update': (call_descend, dict(null=('update',)), 'pointer'),
    'desc-null-gains': (call_descend, dict(null=('gains',)), 'pointer'), 'desc-null-trace': (call_descend, dict(null=('trace',)), 'pointer'),
    'desc-null-nbr': (call_descend, dict(null=('nbr',)), 'pointer'), 'desc-device': (call_descend, dict(device=-1), 'device'),
}


@pytest.mark.parametrize('case_', sorted(REFUSALS))
def test_refusals_precede_the_device_check(case_):
    fn, kw, word = REFUSALS[case_]
    rc, msg, untouched = fn(**kw)
    assert rc == B.NM_ERR_ARG, (rc, msg)
    assert msg.startswith('nm_tsne_') and word in msg, msg
    assert untouched


def test_refusals_come_in_the_header_s_order():
    bad = dict(npoints=0, ndim=0, k=0, perplexity=np.nan, null=('x', 'p'), device=-1)
    good = dict(npoints=6, ndim=2, k=4, perplexity=2.0, null=())
    for key, word in (('npoints', 'npoints'), ('ndim', 'ndim'), ('k', 'k must'), ('perplexity', 'perplexity'), ('null', 'pointer')):
        rc, msg, untouched = call_affinities(**bad)
        assert rc == B.NM_ERR_ARG and msg.startswith('nm_tsne_affinities: ') and word in msg and untouched, msg
        bad[key] = good[key]
    rc, msg, untouched = call_affinities(**bad)
    assert rc == B.NM_ERR_ARG and 'device' in msg and untouched
    L = B.load()
    assert L.nm_tsne_last_timing(None) == B.NM_ERR_ARG and L.nm_tsne_last_error().startswith(b'nm_tsne_last_timing:')


def test_lists_that_are_no_lists_are_refused_without_a_device():
    """an entry that is the row itself or no point, a p that is negative or not finite, a y that is not finite: found on the host"""
    L = B.load()
    for what, msg_part in (('self', 'point 3'), ('range', 'point 2'), ('negative', 'point 4'), ('nan', 'point 1'), ('y', 'y is not finite in point 5')):
        arr = dict(_lists(), grad=np.full((6, 2), SENT), kl=np.full(1, SENT), z=np.full(1, SENT))
        if what == 'self':
            arr['nbr'][3, 1] = 3
        elif what == 'range':
            arr['nbr'][2, 0] = 6
        elif what == 'negative':
            arr['p'][4, 1] = -0.5
        elif what == 'nan':
            arr['p'][1, 0] = np.nan
        else:
            arr['y'][5, 1] = np.inf
        rc = L.nm_tsne_gradient(0, 6, 2, _ptr(arr['nbr'], (), ''), _ptr(arr['p'], (), ''), 2, _ptr(arr['y'], (), ''), 1.0,
                                *[_ptr(arr[n], (), '') for n in ('grad', 'kl', 'z')])
        msg = L.nm_tsne_last_error().decode()
        assert rc == B.NM_ERR_ARG and msg.startswith('nm_tsne_gradient:') and msg_part in msg, msg
        assert all((arr[n] == SENT).all() for n in ('grad', 'kl', 'z'))


def test_a_valid_call_without_a_device_is_a_hip_error():
    for fn, name in ((call_affinities, 'nm_tsne_affinities'), (call_gradient, 'nm_tsne_gradient')):
        rc, msg, untouched = fn()
        assert rc in (B.NM_OK, B.NM_ERR_HIP), msg
        if rc == B.NM_ERR_HIP:
            assert msg.startswith(name + ':') and 'no HIP device' in msg and untouched
    with pytest.raises(ValueError, match='shape'):
        manifold.affinities(np.zeros(4), 2.0, 2)
    with pytest.raises(ValueError, match='one shape'):
        manifold.gradient(np.zeros((4, 2), np.int32), np.zeros((4, 3)), np.zeros((4, 2)))
    with pytest.raises(ValueError, match='float64'):
        manifold.descend(np.zeros((4, 2), np.int32), np.zeros((4, 2)), np.zeros((4, 2)), np.zeros((4, 2), np.float32), np.zeros((4, 2)), 1, 1.0, 0.5, 200.0)


# ---- the host functions of the command line
def test_the_start_and_the_number_of_neighbours():
    x = np.random.default_rng(7).standard_normal((50, 4)) * [3.0, 2.0, 1.0, 0.5]
    y = manifold.start(x, 2)
    np.testing.assert_array_equal(y, x[:, :2] / np.std(x[:, 0]) * 1e-4)
    assert y.flags.c_contiguous and abs(np.std(y[:, 0]) - 1e-4) < 1e-18
    with pytest.raises(ValueError, match='no scale'):
        manifold.start(np.ones((5, 2)), 2)
    assert manifold.neighbours(1000, 30.0) == 91 and manifold.neighbours(50, 30.0) == 49 and manifold.neighbours(1000, 1.5) == 5
    full = manifold.spread(np.arange(12.0).reshape(1, 2, 2, 3), (1, 2, 5, 3), 1, 2)
    assert np.isnan(full[:, :, [0, 2, 4]]).all() and (full[:, :, 1::2] == np.arange(12.0).reshape(1, 2, 2, 3)).all()


def test_cli_flags():
    a = manifold.parse_args([])
    assert (a.feature, a.dimensions, a.perplexity, a.exaggeration, a.learning_rate, a.iterations, a.exaggerated, a.components, a.skip, a.stride,
            a.device) == ('cdf', None, None, 24.0, 200.0, 1000, 250, 2, 0, 1, 0)
    a = manifold.parse_args(['-ft', 'rdf', '-nd', '3', '-px', '40', '-ex', '12', '-lr', '100', '-ni', '500', '-xi', '100', '-nc', '3', '-sk', '5', '-sd', '2',
                             '-dv', '1', '-n', 'x', '-e', 'Al', '-v'])
    assert (a.feature, a.dimensions, a.perplexity, a.exaggeration, a.learning_rate, a.iterations, a.exaggerated, a.components, a.skip, a.stride,
            a.device, a.name, a.element, a.verbose) == ('rdf', 3, 40.0, 12.0, 100.0, 500, 100, 3, 5, 2, 1, 'x', 'Al', True)
    for bad in (['-nd', '0'], ['-nd', '17'], ['-nc', '0'], ['-nc', '4'], ['-px', '1'], ['-px', 'nan'], ['-ex', '0'], ['-ex', 'inf'], ['-lr', '0'],
                ['-ni', '0'], ['-xi', '-1'], ['-ni', '10', '-xi', '11'], ['-sk', '-1'], ['-sd', '0']):
        with pytest.raises(SystemExit):
            manifold.parse_args(bad)
    assert cluster.parse_args(['-nc', '0.1']).embedding == 'pcz' and cluster.parse_args(['-nc', '0.1', '-em', 'mfy']).embedding == 'mfy'
    with pytest.raises(SystemExit):
        cluster.parse_args(['-nc', '0.1', '-em', 'tsne'])


def _write_grid(tmp_path, pn=2, tn=3, sn=6, ld=3):
    prefix = str(tmp_path / 'mf.lj.fcc.lammps')
    rng = np.random.default_rng(1)
    np.save(prefix + '.virial.trgt.npy', np.linspace(1, 2, pn, dtype=np.float32))
    np.save(prefix + '.temp.trgt.npy', np.linspace(1, 2, tn, dtype=np.float32))
    np.save(prefix + '.pe.npy', rng.random((pn, tn, sn)).astype(np.float32))
    np.save(prefix + '.cdf.pcz.npy', rng.random((pn, tn, sn, ld)))
    return prefix


def test_cli_refusals_leave_nothing_written(tmp_path, monkeypatch):
    prefix = _write_grid(tmp_path)
    monkeypatch.chdir(tmp_path)
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(SystemExit, match=r'manifold: .*mf\.lj\.fcc\.lammps\.rdf\.pcz\.npy is missing'):
        manifold.main(['-n', 'mf', '-ft', 'rdf'])
    with pytest.raises(SystemExit, match=r'-nd 4 is more than the 3 components'):
        manifold.main(['-n', 'mf', '-nd', '4'])
    with pytest.raises(SystemExit, match=r'-nc 2 is more than the 1 input components'):
        manifold.main(['-n', 'mf', '-nd', '1'])
    with pytest.raises(SystemExit, match=r'-sk 6 -sd 1 leave 0 samples'):
        manifold.main(['-n', 'mf', '-sk', '6'])
    with pytest.raises(SystemExit, match=r'perplexity 36 wants 35 neighbours of 36 samples'):        # PX < k fails
        manifold.main(['-n', 'mf', '-px', '36'])
    np.save(prefix + '.adf.pcz.npy', np.zeros((3, 3, 6, 4)))
    with pytest.raises(SystemExit, match=r'adf\.pcz\.npy has shape \(3, 3, 6, 4\)'):
        manifold.main(['-n', 'mf', '-ft', 'adf'])
    np.save(prefix + '.flat.pcz.npy', np.ones((2, 3, 6, 2)))
    # (a component 0 without a spread is found by the start, behind the affinities: it needs the device)
    # cluster -em: the other file is looked for, and -em pcz is the file of no flag
    with pytest.raises(SystemExit, match=r'cluster: .*cdf\.mfy\.npy is missing'):
        cluster.main(['-n', 'mf', '-nc', '0.1', '-em', 'mfy'])
    emb = np.random.default_rng(2).random((2, 3, 6, 2))
    emb[:, :, :2] = np.nan
    np.save(prefix + '.cdf.mfy.npy', emb)
    with pytest.raises(SystemExit, match=r'-sk 0 -sd 1 are not those that .*cdf\.mfy\.npy was written with'):
        cluster.main(['-n', 'mf', '-nc', '0.1', '-em', 'mfy'])
    with pytest.raises(SystemExit, match=r'-sk 3 -sd 1 are not those'):
        cluster.main(['-n', 'mf', '-nc', '0.1', '-em', 'mfy', '-sk', '3'])
    os.remove(prefix + '.pe.npy')
    with pytest.raises(SystemExit, match=r'pe\.npy is missing'):
        manifold.main(['-n', 'mf'])
    new = ['mf.lj.fcc.lammps.%s.npy' % f for f in ('adf.pcz', 'flat.pcz', 'cdf.mfy')]
    assert sorted(os.listdir(tmp_path)) == sorted(set(before + new) - {'mf.lj.fcc.lammps.pe.npy'})
