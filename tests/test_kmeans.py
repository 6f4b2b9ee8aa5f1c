"""k-means without a GPU (include/nm_distr.h: nm_cluster_kmeans; neuralmelting_amd/cluster.py): tests/kmeans_ref.py against sklearn's Lloyd
iteration, its tie rule on exact data, every refusal of nm_cluster_kmeans that precedes the device check in its pinned order on
sentinel-filled outputs, the k-means++ seeds of the stage and the command line's flags."""
import ctypes as C
import functools

import numpy as np
import pytest

import kmeans_cases as K
import kmeans_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import cluster

SIZES, DIMS, KS = (255, 256, 257, 511, 513, 515, 1287, 4099), (1, 2, 3, 8, 16), (2, 3, 7)
# The largest |centre - sklearn's centre| over all cases below was measured with this restatement against sklearn 1.7.2: 6.22e-15
# at |x| < 8 (sklearn centres the data before it iterates and sums its members in chunks of threads, so the figure cannot be
# derived).  16 times it:
CENTRE_TOL = 16 * 6.22e-15


@functools.lru_cache(maxsize=None)
def case(n, nd, k):
    x = K.blobs(n, nd, 100 * nd + n)
    init = K.drawn(x, k, n + nd + k)
    x.setflags(write=False)
    return x, init, R.lloyd(x, init, 300, 0.0)


# ---- the restatement is sklearn's Lloyd iteration
@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('nd', DIMS)
@pytest.mark.parametrize('n', SIZES)
def test_the_restatement_equals_sklearn(n, nd, k):
    skc = pytest.importorskip('sklearn.cluster')
    x, init, run = case(n, nd, k)
    # conditions on the input: off ties, no cluster runs empty (sklearn would relocate it), a fixed point is reached
    assert run.status == 0 and run.empties == 0 and run.margin > 1e-9, (run.status, run.iters, run.empties, run.margin)
    sk = skc.KMeans(n_clusters=k, init=init, n_init=1, algorithm='lloyd', tol=0, max_iter=300).fit(x)
    np.testing.assert_array_equal(run.label, sk.labels_)
    print('n %d nd %d k %d: %d steps, margin %.3g, centres off by %.3g' % (n, nd, k, run.iters, run.margin,
                                                                          np.abs(run.centre - sk.cluster_centers_).max()))
    assert np.abs(run.centre - sk.cluster_centers_).max() <= CENTRE_TOL
    np.testing.assert_array_equal(run.count, np.bincount(sk.labels_, minlength=k))
    assert run.label.dtype == run.count.dtype == np.int32


@pytest.mark.parametrize('nd', DIMS)
@pytest.mark.parametrize('n', (257, 1287))
def test_ties_at_the_first_pass_go_to_the_lowest_index(n, nd):
    """on the grid 2^-5 the centres of the first pass are points and every d2 is exact: equal distances are equal bits, and the
    restatement gives such a point to the lowest index.  (A statement about one pass, not about a trajectory.)"""
    x = K.on_grid(K.blobs(n, nd, 100 * nd + n))
    init = K.drawn(x, 7, n + nd + 7)
    init[3] = init[1]                                                       # a duplicated centre never wins
    label, near, gap = R.assign(x, init)
    d2 = ((x[:, None, :] - init[None, :, :]) ** 2).sum(axis=2)              # exact in any order
    np.testing.assert_array_equal(near, d2.min(axis=1))
    for i in range(n):
        assert label[i] == np.nonzero(d2[i] == d2[i].min())[0][0]
    assert gap == 0.0 and (label != 3).all()


def test_the_restatement_s_stops():
    x = K.blobs(513, 2, 11)
    init = K.drawn(x, 3, 12)
    full = R.lloyd(x, init, 300, 0.0)
    assert full.status == 0 and full.iters >= 4 and len(full.shifts) == full.iters
    two = R.lloyd(x, init, 2, 0.0)
    assert (two.status, two.iters) == (2, 2)
    tol = 0.5 * (full.shifts[1] + full.shifts[2])
    assert full.shifts[2] < tol < full.shifts[1]
    one = R.lloyd(x, init, 300, tol)
    assert (one.status, one.iters) == (1, 3)
    for run in (full, two, one):                                            # the labels are the assignment against the centres
        np.testing.assert_array_equal(run.label, R.assign(x, run.centre)[0])
        assert run.inertia == R.assign(x, run.centre)[1].sum()


# ---- the interface
def test_the_symbols_are_exported_and_bound():
    raw = C.CDLL(B.LIB_PATH)
    assert hasattr(raw, 'nm_cluster_kmeans') and hasattr(raw, 'nm_cluster_kmeans_last_timing')
    assert B.DISTR_SYMBOLS[-4:-2] == ('nm_cluster_kmeans', 'nm_cluster_kmeans_last_timing') and B._ERROR_OF['nm_cluster_kmeans'] == 'nm_distr_last_error'
    assert len(B.CLUSTER_SYMBOLS) == 3                                      # include/nm_cluster.h stays DBSCAN's
    L = B.load()
    assert L.nm_cluster_kmeans.restype is C.c_int and len(L.nm_cluster_kmeans.argtypes) == 16


def call(device=0, max_iter=10, tol=0.0, null=(), bad_init=None, **over):
    x = np.random.default_rng(5).random((6, 2))
    init = np.stack([x[:2], x[2:4], x[4:6]])                                # 3 restarts of 2 centres
    if bad_init is not None:
        init[bad_init] = np.nan
    rc, msg, out = K.raw(x, init, max_iter, tol, device, null, **over)
    return rc, msg, K.untouched(out)


REFUSALS = {
    'npoints0': (dict(npoints=0), 'npoints'), 'npoints-3': (dict(npoints=-3), 'npoints'), 'npoints-over': (dict(npoints=2 ** 21 + 1), 'npoints'),
    'npoints-far-over': (dict(npoints=2 ** 62), 'npoints'), 'ndim0': (dict(ndim=0), 'ndim'), 'ndim-1': (dict(ndim=-1), 'ndim'),
    'ndim17': (dict(ndim=17), 'ndim'), 'k0': (dict(k=0), 'k must'), 'k-1': (dict(k=-1), 'k must'), 'k257': (dict(k=257, npoints=1000), 'k must'),
    'k-over-npoints': (dict(k=7), 'k must'), 'nrestarts0': (dict(nrestarts=0), 'nrestarts'), 'nrestarts-2': (dict(nrestarts=-2), 'nrestarts'),
    'nrestarts65': (dict(nrestarts=65), 'nrestarts'), 'centres-over': (dict(k=65, nrestarts=64, npoints=1000), 'nrestarts'),
    'max_iter0': (dict(max_iter=0), 'max_iter'), 'max_iter-1': (dict(max_iter=-1), 'max_iter'), 'max_iter-over': (dict(max_iter=10001), 'max_iter'),
    'tol-negative': (dict(tol=-1e-300), 'tol'), 'tol-nan': (dict(tol=np.nan), 'tol'), 'tol-inf': (dict(tol=np.inf), 'tol'),
    'init-nan': (dict(bad_init=(2, 1, 0)), 'init is not finite in restart 2, centre 1'), 'device-1': (dict(device=-1), 'device'),
    **{'null-' + name: (dict(null=(name,)), 'pointer') for name in ('x', 'init') + K.OUTPUTS},
}


@pytest.mark.parametrize('name', sorted(REFUSALS))
def test_refusals_precede_the_device_check(name):
    kw, word = REFUSALS[name]
    rc, msg, untouched = call(**kw)
    assert rc == B.NM_ERR_ARG, (rc, msg)
    assert msg.startswith('nm_cluster_kmeans: ') and word in msg, msg
    assert untouched


def test_refusals_come_in_the_header_s_order():
    """everything wrong at once, then mended from the front: each call names the first thing that is still wrong"""
    bad = dict(npoints=0, ndim=0, k=0, nrestarts=0, max_iter=0, tol=-1.0, null=('x', 'best'), bad_init=(0, 0, 1), device=-1)
    good = dict(npoints=6, ndim=2, k=2, nrestarts=3, max_iter=10, tol=0.0, null=(), bad_init=None)
    for key, word in (('npoints', 'npoints'), ('ndim', 'ndim'), ('k', 'k must'), ('nrestarts', 'nrestarts'), ('max_iter', 'max_iter'),
                      ('tol', 'tol'), ('null', 'pointer'), ('bad_init', 'init is not finite')):
        rc, msg, untouched = call(**bad)
        assert rc == B.NM_ERR_ARG and msg.startswith('nm_cluster_kmeans: ') and word in msg, msg
        assert untouched
        bad[key] = good[key]
    rc, msg, untouched = call(**bad)
    assert rc == B.NM_ERR_ARG and 'device' in msg and untouched
    L = B.load()
    assert L.nm_cluster_kmeans_last_timing(None) == B.NM_ERR_ARG and L.nm_distr_last_error().startswith(b'nm_cluster_kmeans_last_timing:')


def test_a_valid_call_without_a_device_is_a_hip_error():
    """NM_ERR_HIP where the library finds no device (outputs untouched, no host fallback), NM_OK where it finds one"""
    rc, msg, untouched = call()
    assert rc in (B.NM_OK, B.NM_ERR_HIP), msg
    if rc == B.NM_ERR_HIP:
        assert msg.startswith('nm_cluster_kmeans:') and 'no HIP device' in msg and untouched
        with pytest.raises(RuntimeError, match='nm_cluster_kmeans'):
            cluster.kmeans(np.zeros((4, 2)), np.zeros((1, 2, 2)))
    with pytest.raises(ValueError, match='shape'):
        cluster.kmeans(np.zeros(4), np.zeros((1, 2, 2)))
    with pytest.raises(ValueError, match='shape'):
        cluster.kmeans(np.zeros((4, 2)), np.zeros((2, 3)))


# ---- the seeds
def test_seeds_are_distinct_points_of_x():
    x = K.on_grid(K.blobs(300, 2, 3))
    x[100:200] = x[:100]                                                    # duplicated points: a restart still draws k distinct ones
    s = cluster.seeds(x, 7, 5, 256)
    assert s.shape == (5, 7, 2) and s.dtype == np.float64
    for r in range(5):
        assert len(np.unique(s[r], axis=0)) == 7
        assert all((x == c).all(axis=1).any() for c in s[r])
    assert len(np.unique(s.reshape(5, -1), axis=0)) > 1                     # the restarts differ
    np.testing.assert_array_equal(s, cluster.seeds(x, 7, 5, 256))
    assert not np.array_equal(s, cluster.seeds(x, 7, 5, 257))


def test_seeds_want_k_distinct_points():
    x = np.repeat(np.array([[0.0, 1.0], [2.0, 3.0], [4.0, 5.0]]), 5, axis=0)
    assert len(np.unique(cluster.seeds(x, 3, 4, 1)[2], axis=0)) == 3
    with pytest.raises(ValueError, match='3 distinct points'):
        cluster.seeds(x, 4, 1, 1)


def test_seeds_prefer_far_points():
    """two tight blobs far apart: the second centre lies in the other blob"""
    rng = np.random.default_rng(2)
    x = np.concatenate([rng.normal(0.0, 0.01, (200, 2)), rng.normal(100.0, 0.01, (200, 2))])
    s = cluster.seeds(x, 2, 20, 9)
    assert ((s[:, 0, 0] < 50.0) != (s[:, 1, 0] < 50.0)).all()


# ---- the command line
def test_cli_flags_of_kmeans():
    a = cluster.parse_args(['-cl', 'kmeans', '-nc', '2'])
    assert (a.clustering, a.neighbourhood, a.restarts, a.max_iter, a.tolerance, a.seed) == ('kmeans', 2.0, 10, 300, 1e-4, 256)
    a = cluster.parse_args(['-cl', 'kmeans', '-nc', '256', '-ri', '16', '-mi', '7', '-tl', '0', '-rs', '3', '-ms', '99'])
    assert (a.neighbourhood, a.restarts, a.max_iter, a.tolerance, a.seed) == (256.0, 16, 7, 0.0, 3)
    for bad in (['-nc', '2.5'], ['-nc', '0.5'], ['-nc', '257'], ['-nc', '0'], ['-nc', '-2'], ['-nc', 'nan'], ['-nc', '2', '-ri', '0'],
                ['-nc', '2', '-ri', '65'], ['-nc', '128', '-ri', '33'], ['-nc', '2', '-mi', '0'], ['-nc', '2', '-mi', '10001'],
                ['-nc', '2', '-tl', '-1'], ['-nc', '2', '-tl', 'nan'], ['-nc', '2', '-rs', '-1']):
        with pytest.raises(SystemExit):
            cluster.parse_args(['-cl', 'kmeans'] + bad)
    with pytest.raises(SystemExit):
        cluster.parse_args(['-cl', 'ward', '-nc', '2'])


def test_the_dbscan_parse_result_is_unchanged():
    a = cluster.parse_args(['-nc', '0.05'])
    assert a.clustering == 'dbscan'
    assert (a.feature, a.dimensions, a.neighbourhood, a.min_samples, a.clusters_kept, a.skip, a.stride, a.device) == ('cdf', 2, 0.05, 5, 2, 0, 1, 0)
    assert cluster.parse_args(['-cl', 'dbscan', '-nc', '2.5', '-ri', '0']).neighbourhood == 2.5     # the k-means flags are not looked at


def test_the_table_of_kmeans_labels():
    label, count = np.array([0, 2, 2, 0, 2], dtype=np.int32), np.array([2, 0, 3], dtype=np.int32)
    temp, z = np.array([1.0, 2.0, 4.0, 3.0, 6.0]), np.arange(10.0).reshape(5, 2)
    tab = cluster.kmeans_table(label, count, temp, z)
    np.testing.assert_array_equal(tab[:, 0], count)
    np.testing.assert_array_equal(tab[:, 1], count)                         # every member is a core member
    np.testing.assert_array_equal(tab[:, 2], [2.0, 0.0, 4.0])
    np.testing.assert_array_equal(tab[2, 3:], z[[1, 2, 4]].mean(axis=0))
    assert (tab[1] == 0.0).all()
