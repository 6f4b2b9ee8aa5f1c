"""The cluster stage without a GPU (include/nm_cluster.h, neuralmelting_amd/cluster.py): tests/cluster_ref.py against sklearn's
brute-force DBSCAN, the interface, every refusal that precedes the device check in its pinned order on sentinel-filled outputs,
the stage's own error channel, the host functions of the command line, and the command line's refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import cluster_ref as R
from test_abi import declared_symbols
from neuralmelting_amd import _lib as B
from neuralmelting_amd import cluster

SENT = -77


def blobs(seed, n, nd, k):
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-4.0, 4.0, (k, nd))
    x = centre[rng.integers(0, k, n)] + 0.5 * rng.standard_normal((n, nd))
    x[: n // 10] = rng.uniform(-6.0, 6.0, (n // 10, nd))                          # a tenth is scattered: noise and borders
    return x[rng.permutation(n)]


# ---- the restatement is sklearn's DBSCAN
@pytest.mark.parametrize('seed', range(12))
def test_the_restatement_equals_sklearn(seed):
    skc = pytest.importorskip('sklearn.cluster')
    rng = np.random.default_rng(1000 + seed)
    n, nd, k = int(rng.integers(40, 400)), int(rng.integers(1, 5)), int(rng.integers(2, 5))
    x = blobs(seed, n, nd, k)
    eps, min_pts = float(rng.uniform(0.2, 0.6)) * nd ** 0.5, int(rng.integers(1, 9))
    assert R.margin(x, eps) > 1e-12                                               # off ties: sklearn forms its distances another way
    label, degree, ncl = R.dbscan(x, eps, min_pts)
    sk = skc.DBSCAN(eps=eps, min_samples=min_pts, algorithm='brute').fit(x)
    np.testing.assert_array_equal(label, sk.labels_)
    assert ncl == sk.labels_.max() + 1
    core = np.zeros(n, dtype=bool)
    core[sk.core_sample_indices_] = True
    np.testing.assert_array_equal(degree >= min_pts, core)
    assert label.dtype == degree.dtype == np.int32


def test_the_margin_helper():
    x = np.array([[0.0, 0.0], [3.0, 4.0], [3.0, 4.0]])
    assert R.margin(x, 5.0) == 0.0                                                # a pair at exactly eps
    assert R.margin(x, 4.0) == pytest.approx(9.0 / 16.0)                          # 25 is nearer to 16 than 0 is
    assert R.margin(x, 10.0) == pytest.approx(0.75)


# ---- the interface
def test_header_symbols_are_exported_and_bound():
    syms = declared_symbols('nm_cluster.h')
    assert syms == sorted(B.CLUSTER_SYMBOLS) and len(syms) == 3
    raw = C.CDLL(B.LIB_PATH)
    for s in syms:
        assert hasattr(raw, s), s
    L = B.load()
    assert L.nm_cluster_dbscan.restype is C.c_int and len(L.nm_cluster_dbscan.argtypes) == 9
    assert L.nm_cluster_last_timing.restype is C.c_int and L.nm_cluster_last_error.restype is C.c_char_p


def call(device=0, npoints=6, ndim=2, eps=0.5, min_pts=2, null=()):
    L = B.load()
    x = np.random.default_rng(5).random((6, 2))
    out = dict(label=np.full(6, SENT, np.int32), degree=np.full(6, SENT, np.int32), nclusters=np.full(1, SENT, np.int32))
    rc = L.nm_cluster_dbscan(device, npoints, ndim, None if 'x' in null else x.ctypes.data_as(B.c_double_p), eps, min_pts,
                             *[None if k in null else v.ctypes.data_as(B.c_int32_p) for k, v in out.items()])
    return rc, (L.nm_cluster_last_error().decode() if rc else ''), all((v == SENT).all() for v in out.values())


REFUSALS = {
    'npoints0': (dict(npoints=0), 'npoints'), 'npoints-3': (dict(npoints=-3), 'npoints'), 'npoints-over': (dict(npoints=2 ** 21 + 1), 'npoints'),
    'npoints-far-over': (dict(npoints=2 ** 62), 'npoints'), 'ndim0': (dict(ndim=0), 'ndim'), 'ndim-1': (dict(ndim=-1), 'ndim'),
    'ndim17': (dict(ndim=17), 'ndim'), 'eps0': (dict(eps=0.0), 'eps'), 'eps-negative': (dict(eps=-0.5), 'eps'), 'eps-nan': (dict(eps=np.nan), 'eps'),
    'eps-inf': (dict(eps=np.inf), 'eps'), 'min_pts0': (dict(min_pts=0), 'min_pts'), 'min_pts-2': (dict(min_pts=-2), 'min_pts'),
    'null-x': (dict(null=('x',)), 'pointer'), 'null-label': (dict(null=('label',)), 'pointer'), 'null-degree': (dict(null=('degree',)), 'pointer'),
    'null-nclusters': (dict(null=('nclusters',)), 'pointer'), 'device-1': (dict(device=-1), 'device'),
}


@pytest.mark.parametrize('case', sorted(REFUSALS))
def test_refusals_precede_the_device_check(case):
    kw, word = REFUSALS[case]
    rc, msg, untouched = call(**kw)
    assert rc == B.NM_ERR_ARG, (rc, msg)
    assert msg.startswith('nm_cluster_dbscan: ') and word in msg, msg
    assert untouched


def test_refusals_come_in_the_header_s_order():
    """everything wrong at once, then mended from the front: each call names the first thing that is still wrong"""
    bad = dict(npoints=0, ndim=0, eps=-1.0, min_pts=0, null=('x', 'label'), device=-1)
    good = dict(npoints=6, ndim=2, eps=0.5, min_pts=2, null=())
    for key, word in (('npoints', 'npoints'), ('ndim', 'ndim'), ('eps', 'eps'), ('min_pts', 'min_pts'), ('null', 'pointer')):
        rc, msg, untouched = call(**bad)
        assert rc == B.NM_ERR_ARG and msg.startswith('nm_cluster_dbscan: ') and word in msg, msg
        assert untouched
        bad[key] = good[key]
    rc, msg, untouched = call(**bad)
    assert rc == B.NM_ERR_ARG and 'device' in msg and untouched
    L = B.load()
    assert L.nm_cluster_last_timing(None) == B.NM_ERR_ARG and L.nm_cluster_last_error().startswith(b'nm_cluster_last_timing:')


def test_the_stage_has_an_error_channel_of_its_own():
    L = B.load()
    d = np.zeros(4)
    dp = d.ctypes.data_as(B.c_double_p)
    assert L.nm_pca_moments(0, 1, 1, None, dp, dp, dp, dp) == B.NM_ERR_ARG
    theirs = L.nm_pca_last_error()
    assert theirs.startswith(b'nm_pca_moments:')
    assert call(ndim=0)[0] == B.NM_ERR_ARG
    mine = L.nm_cluster_last_error()
    assert mine.startswith(b'nm_cluster_dbscan:')
    assert L.nm_pca_last_error() == theirs                                # it left the other stage's message alone
    assert L.nm_pca_project(0, 1, 1, None, dp, dp, 1, dp, dp, None) == B.NM_ERR_ARG
    assert L.nm_pca_last_error().startswith(b'nm_pca_project:')
    assert L.nm_cluster_last_error() == mine                              # and the other stage left this one's alone


def test_a_valid_call_without_a_device_is_a_hip_error():
    """NM_ERR_HIP where the library finds no device (outputs untouched, no host fallback), NM_OK where it finds one"""
    rc, msg, untouched = call()
    assert rc in (B.NM_OK, B.NM_ERR_HIP), msg
    if rc == B.NM_ERR_HIP:
        assert msg.startswith('nm_cluster_dbscan:') and 'no HIP device' in msg and untouched
        with pytest.raises(RuntimeError, match='nm_cluster_dbscan'):
            cluster.dbscan(np.zeros((4, 2)), 0.5, 2)
    with pytest.raises(ValueError, match='shape'):
        cluster.dbscan(np.zeros(4), 0.5, 2)


# ---- the host functions of the command line
def test_scaling_by_the_range_of_component_0():
    z = np.array([[1.0, 10.0], [5.0, -30.0], [3.0, 0.0]])
    np.testing.assert_array_equal(cluster.scaled(z), z / 4.0)             # one factor for every component: the geometry is unchanged
    with pytest.raises(ValueError, match='no unit'):
        cluster.scaled(np.array([[2.0, 1.0], [2.0, 5.0]]))


def test_the_cluster_table():
    label = np.array([0, 0, 1, -1, 1, 1, 2], dtype=np.int32)
    degree = np.array([3, 1, 3, 1, 3, 2, 5], dtype=np.int32)
    temp = np.array([1.0, 2.0, 4.0, 9.0, 4.0, 7.0, 0.5])
    z = np.arange(14.0).reshape(7, 2)
    tab = cluster.table(label, degree, 3, temp, z)
    assert tab.shape == (3, 5) and tab.dtype == np.float64
    np.testing.assert_array_equal(tab[:, 0], [2, 3, 1])                   # members
    np.testing.assert_array_equal(tab[:, 1], [1, 2, 1])                   # core members
    np.testing.assert_array_equal(tab[:, 2], [1.5, 5.0, 0.5])             # mean target temperature
    np.testing.assert_array_equal(tab[1, 3:], z[[2, 4, 5]].mean(axis=0))  # centroid
    assert cluster.table(np.full(3, -1, np.int32), np.ones(3, np.int32), 2, np.ones(3), np.ones((3, 2))).shape == (0, 5)


def _tab(members, temps):
    return np.stack([members, members, temps], axis=1).astype(np.float64)


def test_phase_order_by_size_then_by_temperature():
    # four clusters; the two largest are 1 (hot) and 3 (cold): cl0 is the cold one
    assert cluster.phases(_tab([5, 90, 7, 80], [1.0, 3.0, 0.1, 2.0]), 2) == [3, 1]
    assert cluster.phases(_tab([5, 90, 7, 80], [1.0, 3.0, 0.1, 2.0]), 3) == [2, 3, 1]
    # a tie in members at the cut: the smaller label is kept
    assert cluster.phases(_tab([50, 9, 9, 9], [2.0, 5.0, 1.0, 0.5]), 2) == [0, 1]
    assert cluster.phases(_tab([9, 9, 9], [3.0, 2.0, 1.0]), 2) == [1, 0]
    # a tie in temperature: the smaller label first
    assert cluster.phases(_tab([10, 20], [1.5, 1.5]), 2) == [0, 1]
    # fewer clusters than asked for, and none
    assert cluster.phases(_tab([4], [1.0]), 2) == [0]
    assert cluster.phases(np.zeros((0, 5)), 2) == []


def test_samples_left_out_are_filled():
    kept = np.arange(2 * 3 * 3).reshape(2, 3, 3).astype(np.int32) + 1
    full = cluster.spread(kept, (2, 3, 8), 1, 3, -1)                      # samples 1, 4, 7 of 8
    assert full.dtype == np.int32 and full.shape == (2, 3, 8)
    np.testing.assert_array_equal(full[:, :, 1::3], kept)
    mask = np.ones(8, dtype=bool)
    mask[1::3] = False
    assert (full[:, :, mask] == -1).all()
    np.testing.assert_array_equal(cluster.spread(kept, (2, 3, 3), 0, 1, 0), kept)


# ---- the command line
def _write_grid(tmp_path, pn=2, tn=3, sn=6, ld=3):
    prefix = str(tmp_path / 'cl.lj.fcc.lammps')
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
    with pytest.raises(SystemExit, match=r'cluster: .*cl\.lj\.fcc\.lammps\.rdf\.pcz\.npy is missing'):
        cluster.main(['-n', 'cl', '-ft', 'rdf', '-nc', '0.1'])
    np.save(prefix + '.adf.pcz.npy', np.zeros((3, 3, 6, 4)))
    with pytest.raises(SystemExit, match=r'adf\.pcz\.npy has shape \(3, 3, 6, 4\)'):
        cluster.main(['-n', 'cl', '-ft', 'adf', '-nc', '0.1'])
    np.save(prefix + '.sf.pcz.npy', np.zeros((2, 3, 6)))                  # no component axis
    with pytest.raises(SystemExit, match=r'sf\.pcz\.npy has shape'):
        cluster.main(['-n', 'cl', '-ft', 'sf', '-nc', '0.1'])
    with pytest.raises(SystemExit, match=r'-nd 4 is more than the 3 components of .*cdf\.pcz\.npy'):
        cluster.main(['-n', 'cl', '-nd', '4', '-nc', '0.1'])
    with pytest.raises(SystemExit, match=r'-sk 6 -sd 1 leave 0 samples of .*cdf\.pcz\.npy'):
        cluster.main(['-n', 'cl', '-sk', '6', '-nc', '0.1'])
    np.save(prefix + '.flat.pcz.npy', np.ones((2, 3, 6, 2)))              # component 0 without a range
    with pytest.raises(SystemExit, match=r'flat\.pcz\.npy: component 0 is 1 in every clustered sample'):
        cluster.main(['-n', 'cl', '-ft', 'flat', '-nc', '0.1'])
    os.remove(prefix + '.pe.npy')
    with pytest.raises(SystemExit, match=r'pe\.npy is missing'):
        cluster.main(['-n', 'cl', '-nc', '0.1'])
    new = ['cl.lj.fcc.lammps.%s.pcz.npy' % f for f in ('adf', 'sf', 'flat')]
    assert sorted(os.listdir(tmp_path)) == sorted(set(before + new) - {'cl.lj.fcc.lammps.pe.npy'})


def test_cli_flags():
    a = cluster.parse_args(['-nc', '0.05'])
    assert (a.feature, a.dimensions, a.neighbourhood, a.min_samples, a.clusters_kept, a.skip, a.stride, a.device) == ('cdf', 2, 0.05, 5, 2, 0, 1, 0)
    a = cluster.parse_args(['-ft', 'rdf', '-nd', '3', '-nc', '1e-2', '-ms', '9', '-nk', '4', '-sk', '5', '-sd', '2', '-dv', '1', '-n', 'x', '-e', 'Al', '-v'])
    assert (a.feature, a.dimensions, a.neighbourhood, a.min_samples, a.clusters_kept, a.skip, a.stride, a.device, a.name, a.element, a.verbose) == (
        'rdf', 3, 0.01, 9, 4, 5, 2, 1, 'x', 'Al', True)
    for bad in ([], ['-nc', '0'], ['-nc', '-1'], ['-nc', 'nan'], ['-nc', '0.1', '-nd', '0'], ['-nc', '0.1', '-nd', '17'], ['-nc', '0.1', '-nk', '0'],
                ['-nc', '0.1', '-nk', '9'], ['-nc', '0.1', '-ms', '0'], ['-nc', '0.1', '-sk', '-1'], ['-nc', '0.1', '-sd', '0']):
        with pytest.raises(SystemExit):
            cluster.parse_args(bad)
