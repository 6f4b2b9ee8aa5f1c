"""Spectral clustering without a GPU (include/nm_distr.h: nm_cluster_spectral; neuralmelting_amd/cluster.py): the two symbols and their
place in the binding, every refusal of nm_cluster_spectral that precedes the device check in its pinned order on sentinel-filled outputs,
tests/spectral_ref.py against sklearn, the conditions on the inputs that tests/test_spectral_gpu.py rests on, and the command line's flags."""
import ctypes as C

import numpy as np
import pytest

import spectral_cases as K
import spectral_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import cluster


# ---- the interface
def test_the_symbols_are_exported_and_bound():
    raw = C.CDLL(B.LIB_PATH)
    assert hasattr(raw, 'nm_cluster_spectral') and hasattr(raw, 'nm_cluster_spectral_last_timing')
    at = B.DISTR_SYMBOLS.index('nm_cluster_kmeans')
    assert B.DISTR_SYMBOLS[at - 2:at] == ('nm_cluster_spectral', 'nm_cluster_spectral_last_timing')
    assert B.DISTR_SYMBOLS[at - 3] == 'nm_distr_entropy'
    assert B._ERROR_OF['nm_cluster_spectral'] == B._ERROR_OF['nm_cluster_spectral_last_timing'] == 'nm_distr_last_error'
    assert len(B.CLUSTER_SYMBOLS) == 3                                      # include/nm_cluster.h stays DBSCAN's
    L = B.load()
    assert L.nm_cluster_spectral.restype is C.c_int and len(L.nm_cluster_spectral.argtypes) == 16
    assert L.nm_cluster_spectral_last_timing.restype is C.c_int and len(L.nm_cluster_spectral_last_timing.argtypes) == 1


def call(gamma=1.0, ncomp=2, nblock=3, degree=8, max_pass=10, tol=0.0, device=0, null=(), bad_init=None, **over):
    x = np.random.default_rng(5).random((6, 2))
    init = K.start(6, 3)
    if bad_init is not None:
        init[bad_init] = np.nan
    rc, msg, out = K.raw(x, gamma, ncomp, init, degree, max_pass, tol, device, null, nblock=nblock, **over)
    return rc, msg, K.untouched(out)


REFUSALS = {
    'npoints1': (dict(npoints=1), 'npoints'), 'npoints0': (dict(npoints=0), 'npoints'), 'npoints-3': (dict(npoints=-3), 'npoints'),
    'npoints-over': (dict(npoints=2 ** 20 + 1), 'npoints'), 'npoints-far-over': (dict(npoints=2 ** 62), 'npoints'),
    'ndim0': (dict(ndim=0), 'ndim'), 'ndim-1': (dict(ndim=-1), 'ndim'), 'ndim17': (dict(ndim=17), 'ndim'),
    'gamma0': (dict(gamma=0.0), 'gamma'), 'gamma-1': (dict(gamma=-1.0), 'gamma'), 'gamma-nan': (dict(gamma=np.nan), 'gamma'),
    'gamma-inf': (dict(gamma=np.inf), 'gamma'),
    'ncomp0': (dict(ncomp=0), 'ncomp must'), 'ncomp-1': (dict(ncomp=-1), 'ncomp must'), 'ncomp9': (dict(ncomp=9, nblock=9, npoints=100), 'ncomp must'),
    'ncomp-over-npoints': (dict(ncomp=7, nblock=7), 'ncomp must'),
    'nblock-under-ncomp': (dict(ncomp=3, nblock=2), 'nblock must'), 'nblock17': (dict(nblock=17, npoints=100), 'nblock must'),
    'nblock-over-npoints': (dict(nblock=7), 'nblock must'),
    'degree0': (dict(degree=0), 'degree'), 'degree-1': (dict(degree=-1), 'degree'), 'degree65': (dict(degree=65), 'degree'),
    'max_pass0': (dict(max_pass=0), 'max_pass'), 'max_pass-1': (dict(max_pass=-1), 'max_pass'), 'max_pass-over': (dict(max_pass=100001), 'max_pass'),
    'tol-negative': (dict(tol=-1e-300), 'tol'), 'tol-nan': (dict(tol=np.nan), 'tol'), 'tol-inf': (dict(tol=np.inf), 'tol'),
    'init-nan': (dict(bad_init=(4, 1)), 'init is not finite in row 4, column 1'), 'device-1': (dict(device=-1), 'device'),
    **{'null-' + name: (dict(null=(name,)), 'pointer') for name in ('x', 'init') + K.OUTPUTS},
}


@pytest.mark.parametrize('name', sorted(REFUSALS))
def test_refusals_precede_the_device_check(name):
    kw, word = REFUSALS[name]
    rc, msg, untouched = call(**kw)
    assert rc == B.NM_ERR_ARG, (rc, msg)
    assert msg.startswith('nm_cluster_spectral: ') and word in msg, msg
    assert untouched


def test_refusals_come_in_the_header_s_order():
    """everything wrong at once, then mended from the front: each call names the first thing that is still wrong"""
    bad = dict(npoints=1, ndim=0, gamma=-1.0, ncomp=0, nblock=17, degree=0, max_pass=0, tol=-1.0, null=('x', 'info'), bad_init=(0, 2), device=-1)
    good = dict(npoints=6, ndim=2, gamma=1.0, ncomp=2, nblock=3, degree=8, max_pass=10, tol=0.0, null=(), bad_init=None)
    for key, word in (('npoints', 'npoints'), ('ndim', 'ndim'), ('gamma', 'gamma'), ('ncomp', 'ncomp must'), ('nblock', 'nblock must'),
                      ('degree', 'degree'), ('max_pass', 'max_pass'), ('tol', 'tol'), ('null', 'pointer'), ('bad_init', 'init is not finite')):
        rc, msg, untouched = call(**bad)
        assert rc == B.NM_ERR_ARG and msg.startswith('nm_cluster_spectral: ') and word in msg, msg
        assert untouched
        bad[key] = good[key]
    rc, msg, untouched = call(**bad)
    assert rc == B.NM_ERR_ARG and 'device' in msg and untouched
    L = B.load()
    assert L.nm_cluster_spectral_last_timing(None) == B.NM_ERR_ARG and L.nm_distr_last_error().startswith(b'nm_cluster_spectral_last_timing:')


def test_a_valid_call_without_a_device_is_a_hip_error():
    """NM_ERR_HIP where the library finds no device (outputs untouched, no host fallback), NM_OK where it finds one"""
    rc, msg, untouched = call()
    assert rc in (B.NM_OK, B.NM_ERR_HIP), msg
    if rc == B.NM_ERR_HIP:
        assert msg.startswith('nm_cluster_spectral:') and 'no HIP device' in msg and untouched
        with pytest.raises(RuntimeError, match='nm_cluster_spectral'):
            cluster.spectral(np.random.default_rng(1).random((4, 2)), 1.0, 2, K.start(4, 2))
    with pytest.raises(ValueError, match='shape'):
        cluster.spectral(np.zeros(4), 1.0, 2, np.zeros((4, 2)))
    with pytest.raises(ValueError, match='shape'):
        cluster.spectral(np.zeros((4, 2)), 1.0, 2, np.zeros((3, 2)))


# ---- the reference is sklearn's
def test_the_reference_is_sklearn_s_embedding_and_clustering():
    skm, skc = pytest.importorskip('sklearn.manifold'), pytest.importorskip('sklearn.cluster')
    x, which = K.blobs(300, 3)
    ref = R.dense(x, K.BLOBS_GAMMA)
    a = R.affinity(x, K.BLOBS_GAMMA)
    theirs = skm.spectral_embedding(a, n_components=3, norm_laplacian=True, drop_first=False, eigen_solver='arpack', random_state=0)
    assert ref.lam[2] - ref.lam[3] > K.BLOBS_GAP
    assert R.sine(R.embedding(ref, 3), theirs) <= 1e-9 / (ref.lam[2] - ref.lam[3])
    label = skc.SpectralClustering(n_clusters=3, affinity='rbf', gamma=K.BLOBS_GAMMA, assign_labels='kmeans', random_state=0).fit(x).labels_
    assert R.labels_agree(label, which) and R.labels_agree(R.lloyd(R.embedding(ref, 3), 3, 1), label)


def test_the_sign_rule_and_the_angle():
    e = R.signed(np.array([[1.0, -3.0, 2.0], [-2.0, 3.0, -2.0], [0.5, 1.0, 1.0]]))
    np.testing.assert_array_equal(e, [[-1.0, 3.0, 2.0], [2.0, -3.0, -2.0], [-0.5, -1.0, 1.0]])      # equal magnitudes: the first index decides
    rng = np.random.default_rng(2)
    p = np.linalg.qr(rng.standard_normal((50, 3)))[0]
    assert R.sine(p, p @ np.linalg.qr(rng.standard_normal((3, 3)))[0]) < 1e-14
    q = p.copy()
    q[:, 2] = np.cos(1e-7) * p[:, 2] + np.sin(1e-7) * np.linalg.qr(np.concatenate([p, rng.standard_normal((50, 1))], axis=1))[0][:, 3]
    assert R.sine(p, q) == pytest.approx(1e-7, rel=1e-6)


# ---- the conditions the GPU tests rest on
@pytest.mark.parametrize('n', [n for n in K.SIZES if n >= K.TILE - 1] + [1287])
def test_the_rings_have_their_gap_and_centroids_cannot_cut_them(n):
    x, inner = K.rings(n, 2000 + n) if n != 1287 else K.rings(1287, 1)
    ref = R.dense(x, K.RINGS_GAMMA)
    print('rings n %d: lambda %s, gap %.4g, smallest degree %.4g' % (n, ref.lam[:4], ref.lam[1] - ref.lam[2], float(ref.deg.min())))
    assert ref.lam[1] - ref.lam[2] >= K.RINGS_GAP and ref.deg.min() > 1.0
    raw = R.lloyd(x, 2, 1)
    wrong = min((raw == inner).mean(), (raw != inner).mean())
    assert wrong > 0.25
    assert R.labels_agree(R.lloyd(R.embedding(ref, 2), 2, 1), inner)


@pytest.mark.parametrize('nd', (2, 3, 16))
@pytest.mark.parametrize('n', [n for n in K.SIZES if n >= K.TILE - 1])
def test_the_blobs_have_their_gap(n, nd):
    x, gamma, which, ref = K.case(n, nd, 3)
    assert gamma == K.BLOBS_GAMMA and ref.lam[2] - ref.lam[3] >= K.BLOBS_GAP and ref.deg.min() > 1.0
    assert R.labels_agree(R.lloyd(R.embedding(ref, 3), 3, 1), which)


def test_the_cases_of_the_rings_are_the_generator_s():
    for n in (K.TILE + 1, 2 * K.ROWS + K.TILE + 7):
        np.testing.assert_array_equal(K.case(n, 2, 2)[0], K.rings(n, 2000 + n)[0])


def test_the_bounds_stay_small_at_the_tested_sizes():
    """the header's bound of a residual must not be able to hide a wrong one at the tolerance 1e-8 of the GPU tests"""
    for nd in (1, 2, 3, 16):
        for ncomp, nblock in K.WIDTHS:
            n = K.SIZES[-1]
            ref = K.case(n, nd, ncomp)[3]
            assert R.eps_r(ref, n, nd, nblock) < 1e-10


def test_the_restatement_predicts_the_pass_count():
    x, inner = K.rings(1287, 1)
    ref = R.dense(x, K.RINGS_GAMMA)
    passes, status, theta, resid, v = R.filtered(ref.m, K.start(1287, 16), 2, 8, 2000, 1e-8)
    print('rings 1287, block 16, degree 8: %d passes to 1e-8' % passes)
    assert status == 0 and passes < 200 and np.abs(theta[:2] - ref.lam[:2]).max() < 1e-10
    assert R.sine(v[:, :2], ref.vec[:, :2]) <= resid[:2].max() / (ref.lam[1] - ref.lam[2])
    one = R.filtered(ref.m, K.start(1287, 16), 2, 8, 1, 1e-8)
    assert one[:2] == (1, 2)


# ---- the command line
def test_cli_flags_of_spectral():
    a = cluster.parse_args(['-cl', 'spectral', '-nc', '2'])
    assert (a.clustering, a.neighbourhood, a.gamma, a.eigen_block, a.eigen_degree, a.eigen_tolerance, a.eigen_passes) == ('spectral', 2.0, 1.0, 16, 8, 1e-6, 2000)
    assert (a.restarts, a.max_iter, a.tolerance, a.seed) == (10, 300, 1e-4, 256)
    a = cluster.parse_args(['-cl', 'spectral', '-nc', '8', '-gm', '0.5', '-eb', '8', '-ed', '1', '-et', '0', '-ei', '7', '-ri', '3'])
    assert (a.neighbourhood, a.gamma, a.eigen_block, a.eigen_degree, a.eigen_tolerance, a.eigen_passes, a.restarts) == (8.0, 0.5, 8, 1, 0.0, 7, 3)
    for bad in (['-nc', '1'], ['-nc', '9'], ['-nc', '2.5'], ['-nc', 'nan'], ['-nc', '2', '-gm', '0'], ['-nc', '2', '-gm', '-1'], ['-nc', '2', '-gm', 'nan'],
                ['-nc', '2', '-gm', 'inf'], ['-nc', '3', '-eb', '2'], ['-nc', '2', '-eb', '17'], ['-nc', '2', '-ed', '0'], ['-nc', '2', '-ed', '65'],
                ['-nc', '2', '-et', '-1'], ['-nc', '2', '-et', 'nan'], ['-nc', '2', '-ei', '0'], ['-nc', '2', '-ei', '100001'], ['-nc', '2', '-ri', '0'],
                ['-nc', '2', '-mi', '0'], ['-nc', '2', '-tl', '-1'], ['-nc', '2', '-rs', '-1']):
        with pytest.raises(SystemExit):
            cluster.parse_args(['-cl', 'spectral'] + bad)


def test_the_other_parse_results_are_unchanged():
    a = cluster.parse_args(['-nc', '0.05', '-gm', '-1', '-eb', '99'])          # the spectral flags are not looked at
    assert a.clustering == 'dbscan' and a.neighbourhood == 0.05
    a = cluster.parse_args(['-cl', 'kmeans', '-nc', '256', '-ed', '0'])
    assert a.clustering == 'kmeans' and a.neighbourhood == 256.0
