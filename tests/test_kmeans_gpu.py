"""k-means on the GPU (include/nm_distr.h: nm_cluster_kmeans): nm_cluster_kmeans on sentinel-filled outputs against tests/kmeans_ref.py on ragged
sizes around every edge of the kernels' shapes, exact data with ties in one step, an empty cluster, the three stops, batches of
restarts against single calls, a permutation of the centres, two calls, values that are not finite, a size of many chunks; and
neuralmelting_amd.cluster -cl kmeans end to end on the synthetic two-phase grid, through reweight."""
import functools
import os
import re

import numpy as np
import pytest

import kmeans_cases as K
import kmeans_ref as R
from test_cluster_gpu import NATOMS, PN, SN, TN, two_phase_grid
from neuralmelting_amd import _lib as B
from neuralmelting_amd import cluster, reweight

pytestmark = pytest.mark.gpu

T, ROWS, PIECE, CHUNK = 256, 512, 64, 4096      # csrc/nm_kmeans.h: centres of a tile, rows of a workgroup, points of a lane and of a tree
U = 2.0 ** -53


def test_the_tile_is_what_the_cases_assume():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'neuralmelting_amd', 'csrc', 'nm_kmeans.h')).read()
    const = {k: v for k, v in re.findall(r'constexpr int (KM_\w+) = ([^;]+);', src)}
    assert int(const['KM_TILE']) == T and int(const['KM_BLOCK']) == 256 and int(const['KM_RPT']) == 2 and const['KM_ROWS'] == 'KM_RPT * KM_BLOCK'
    assert int(const['KM_PIECE']) == PIECE and const['KM_CHUNK'] == '64 * KM_PIECE' and CHUNK == 64 * PIECE and ROWS == 2 * 256


def check(x, init, max_iter=300, tol=0.0, run=None, off_ties=True):
    """the device's outputs of one restart, after they have been found equal to the restatement's (run, where the caller holds it)"""
    rc, msg, out = K.raw(x, init, max_iter, tol)
    assert rc == B.NM_OK, msg
    run = run or R.lloyd(x, init, max_iter, tol)
    if off_ties:        # d2's error is (ndim + 2) u of itself, the nearest two centres of every point of every pass differ by 1e-9 of it
        assert run.margin > 1e-9 and run.empties == 0, 'the input has a near tie or an empty cluster: choose another seed'
    np.testing.assert_array_equal(out['label'], run.label)
    np.testing.assert_array_equal(out['count'], run.count)
    assert (out['iters'][0], out['status'][0], out['best'][0]) == (run.iters, run.status, 0)
    # with the same members, the two centres are means of the same terms in two orders
    bound = (run.count[:, None] + 2) * U * np.abs(x).max()
    print('centres off by %.3g of their bound, inertia by %.3g of its' % (
        (np.abs(out['centre'] - run.centre) / bound).max(), abs(out['inertia'][0] - run.inertia) / ((x.shape[0] + x.shape[1] + 2) * U * max(run.inertia, 1e-300))))
    assert (np.abs(out['centre'] - run.centre) <= bound).all()
    assert abs(out['inertia'][0] - run.inertia) <= (x.shape[0] + x.shape[1] + 2) * U * run.inertia       # positive terms in any order
    return out, run


# ---- ragged sizes: the edges of a piece, a tile, a row block and a chunk
@functools.lru_cache(maxsize=None)
def ragged(n, nd, k):
    x = K.blobs(n, nd, 100 * nd + n)
    init = K.drawn(x, k, n + nd + k + (1000 if (n, nd, k) == (PIECE + 1, 16, 7) else 0))      # (that case ran a cluster empty from its seed)
    x.setflags(write=False)
    return x, init, R.lloyd(x, init, 300, 0.0)


SIZES = (1, 2, PIECE - 1, PIECE + 1, T - 1, T, T + 1, 2 * T + 3, ROWS - 1, ROWS + 1, 2 * ROWS + T + 7, CHUNK - 1, CHUNK + 1, 2 * CHUNK + PIECE + 7)


@pytest.mark.parametrize('n,nd,k', [(n, nd, k) for n in SIZES for nd in (1, 2, 3, 8, 16) for k in (1, 2, 3, 7) if k <= n])
def test_ragged_sizes(n, nd, k):
    x, init, run = ragged(n, nd, k)
    out, run = check(x, init, run=run)
    assert run.status == (0 if k < n else 1)                                # with k = n the first update moves nothing


# ---- exact data, one step
def exact_case():
    """centres (0,0), (4,0), (0,4) and (4,0) again; around each of the first three the 33 x 33 grid points within 1/2; a point at
    equal distance from centres 0 and 1, twice; one from 0, 1 and 2; one from 1 and 2 and its mirror image in centre 1, so that
    cluster 1 is symmetric about its centre and its mean is that centre again, bit for bit; and a point of cluster 2 alone, which
    moves centre 2, so that the assignment against the new centres has no tie but those with the copy of centre 1"""
    init = np.array([[0.0, 0.0], [4.0, 0.0], [0.0, 4.0], [4.0, 0.0]])
    off = np.arange(-16, 17) * K.G
    patch = np.stack(np.meshgrid(off, off), axis=-1).reshape(-1, 2)
    ties = np.array([[2.0, -1.0], [2.0, -1.0], [2.0, 2.0], [4.0, 4.0], [4.0, -4.0], [0.0, 6.0]])
    x = np.concatenate([ties] + [patch + c for c in init[:3]]) + 0.0
    first = np.array([0, 0, 0, 1, 1, 2] + [0] * len(patch) + [1] * len(patch) + [2] * len(patch))
    p = np.random.default_rng(6).permutation(x.shape[0])
    return x[p], init, first[p]


def test_one_step_on_exact_data():
    x, init, first = exact_case()
    assert x.shape[0] <= 4096 and np.abs(x).max() <= 64 and (x / K.G == np.round(x / K.G)).all()
    d2 = ((x[:, None, :] - init[None, :, :]) ** 2).sum(axis=2)              # exact in any order
    assert ((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) >= 2).sum() >= 5 + 1089       # the ties, and cluster 1 against its copy
    np.testing.assert_array_equal(first, [np.nonzero(row == row.min())[0][0] for row in d2])    # tied points go to the lowest index
    rc, msg, out = K.raw(x, init, max_iter=1)
    assert rc == B.NM_OK, msg
    assert (out['iters'][0], out['status'][0]) == (1, 2)
    want = np.stack([x[first == j].sum(axis=0) / (first == j).sum() for j in range(3)])    # exact sums, one division
    assert out['centre'][:3].tobytes() == want.tobytes()
    assert out['centre'][3].tobytes() == init[3].tobytes() == out['centre'][1].tobytes()   # the copy kept its bits, cluster 1 its place
    # the labels are the assignment against these centres: centre 3 is centre 1 again and loses every tie
    label, near, gap = R.assign(x, out['centre'])
    assert R.assign(x, out['centre'][:3])[2] > 1e-9
    np.testing.assert_array_equal(out['label'], label)
    np.testing.assert_array_equal(out['count'], np.bincount(label, minlength=4))
    assert out['count'][3] == 0 and out['count'].sum() == x.shape[0]
    assert out['inertia'][0] == pytest.approx(near.sum(), rel=1e-12)


def test_an_empty_cluster_keeps_its_centre():
    x = K.blobs(2 * ROWS + T + 7, 3, 21)
    init = np.concatenate([K.drawn(x, 2, 22), [[1e3, -1e3, 1e3]], K.drawn(x, 1, 23)])
    run = R.lloyd(x, init, 300, 0.0)
    assert run.empties > 0 and run.margin > 1e-9 and run.iters > 2
    out, run = check(x, init, run=run, off_ties=False)
    assert out['count'][2] == 0 and out['status'][0] == 0 and out['centre'][2].tobytes() == init[2].tobytes()
    assert (out['label'] != 2).all()


# ---- the three stops
def test_stops():
    x = K.blobs(513, 2, 11)
    init = K.drawn(x, 3, 12)
    full = R.lloyd(x, init, 300, 0.0)
    assert full.status == 0 and full.iters >= 4 and full.shifts[2] < full.shifts[1]
    tol = 0.5 * (full.shifts[1] + full.shifts[2])
    for max_iter, tl, status, iters in ((2, 0.0, 2, 2), (300, tol, 1, 3), (300, 0.0, 0, full.iters)):
        out, run = check(x, init, max_iter, tl)
        assert (run.status, run.iters) == (status, iters)
        label, near, gap = R.assign(x, out['centre'])                       # the labels are the assignment against the returned centres
        assert gap > 1e-9
        np.testing.assert_array_equal(out['label'], label)


# ---- batches of restarts
@pytest.mark.parametrize('nr,k', ((7, 3), (64, 1), (64, 64), (40, 7)))
def test_a_batch_is_its_single_restarts(nr, k):
    """(64, 64) is k * nrestarts = 4096; (40, 7) has a restart across the edge of a tile of centres"""
    x = K.blobs(601, 3, 31)
    init = K.drawn(x, k, 32, nr)
    rc, msg, out = K.raw(x, init)
    assert rc == B.NM_OK, msg
    single = [K.raw(x, init[r])[2] for r in range(nr)]
    for name in ('inertia', 'iters', 'status'):
        assert out[name].tobytes() == np.concatenate([s[name] for s in single]).tobytes(), name
    if k > 1:
        assert len(set(out['iters'])) > 1                                   # they finished at different steps
    best = int(out['best'][0])
    assert best == np.argmin(out['inertia'])
    for name in ('label', 'centre', 'count'):
        assert out[name].tobytes() == single[best][name].tobytes(), name
    # the best twice: the lower index
    order = [r for r in range(nr) if r != best]
    pick = order[:2] + [best] + order[2:4] + [best] + order[4:nr - 2]
    rc, msg, again = K.raw(x, init[pick])
    assert rc == B.NM_OK and len(pick) == nr and again['inertia'].tobytes() == out['inertia'][pick].tobytes()
    first = int(again['best'][0])
    assert first == np.argmin(again['inertia']) <= 2 and again['inertia'][5] == again['inertia'][first]
    assert again['label'].tobytes() == single[pick[first]]['label'].tobytes()


def test_a_permutation_of_the_centres_permutes_the_result():
    x = K.blobs(2 * ROWS + T + 7, 8, 41)
    init = K.drawn(x, 7, 42, 3)
    p = np.random.default_rng(43).permutation(7)
    other = init.copy()
    other[1] = init[1][p]
    (rc, msg, a), (rc2, msg2, b) = K.raw(x, init), K.raw(x, other)
    assert rc == rc2 == B.NM_OK
    for name in ('inertia', 'iters', 'status', 'best'):
        assert a[name].tobytes() == b[name].tobytes(), name
    one = K.raw(x, init[1])[2], K.raw(x, other[1])[2]
    np.testing.assert_array_equal(p[one[1]['label']], one[0]['label'])
    assert one[1]['centre'].tobytes() == one[0]['centre'][p].tobytes() and one[1]['count'].tobytes() == one[0]['count'][p].tobytes()
    assert one[1]['inertia'].tobytes() == one[0]['inertia'].tobytes() and one[1]['iters'][0] == one[0]['iters'][0]


def test_two_calls_give_the_same_bytes():
    x = K.blobs(4099, 16, 51)
    init = K.drawn(x, 7, 52, 10)
    L = B.load()
    dbscan = np.full(5, -1.0)
    assert L.nm_cluster_last_timing(dbscan) == B.NM_OK
    one, two = K.raw(x, init), K.raw(x, init)
    assert one[0] == two[0] == B.NM_OK
    for name in K.OUTPUTS:
        assert one[2][name].tobytes() == two[2][name].tobytes(), name
    ms, after = np.full(3, -1.0), np.full(5, -1.0)
    assert L.nm_cluster_kmeans_last_timing(ms) == B.NM_OK and L.nm_cluster_last_timing(after) == B.NM_OK
    assert (ms >= 0.0).all() and ms[1] > 0.0 and ms[2] > 0.0
    assert after.tobytes() == dbscan.tobytes()                              # the DBSCAN slots are left alone


# ---- values that are not finite
@pytest.mark.parametrize('bad', (np.nan, np.inf, -np.inf))
def test_a_value_that_is_not_finite_is_refused(bad):
    x = np.array(K.blobs(2 * T + 3, 2, 61))
    init = K.drawn(x, 2, 62, 3)
    x[-1, 1] = bad
    rc, msg, out = K.raw(x, init)
    assert rc == B.NM_ERR_ARG and msg.startswith('nm_cluster_kmeans:') and msg.endswith('point %d' % (x.shape[0] - 1)), msg
    assert K.untouched(out)
    x[T + 5, 0] = bad                                                       # the first of two is named
    rc, msg, out = K.raw(x, init)
    assert rc == B.NM_ERR_ARG and msg.endswith('point %d' % (T + 5)) and K.untouched(out), msg
    x = K.blobs(2 * T + 3, 2, 61)
    init[1, 0, 1] = bad
    rc, msg, out = K.raw(x, init)
    assert rc == B.NM_ERR_ARG and msg.startswith('nm_cluster_kmeans:') and msg.endswith('restart 1, centre 0') and K.untouched(out), msg


# ---- many chunks, the batch against the restatement
def test_a_size_of_many_chunks():
    x = K.blobs(70001, 2, 71, k=2)
    init = K.drawn(x, 2, 72, 10)
    runs = [R.lloyd(x, init[r], 300, 0.0) for r in range(10)]
    assert all(run.margin > 1e-9 and run.empties == 0 and run.status == 0 for run in runs)
    rc, msg, out = K.raw(x, init)
    assert rc == B.NM_OK, msg
    np.testing.assert_array_equal(out['iters'], [run.iters for run in runs])
    np.testing.assert_array_equal(out['status'], [run.status for run in runs])
    inertia = np.array([run.inertia for run in runs])
    assert (np.abs(out['inertia'] - inertia) <= (70001 + 2 + 2) * U * inertia).all()
    best = int(out['best'][0])
    assert best == np.argmin(out['inertia']) and inertia[best] <= inertia.min() * (1 + 1e-10)
    np.testing.assert_array_equal(out['label'], runs[best].label)
    np.testing.assert_array_equal(out['count'], runs[best].count)
    assert (np.abs(out['centre'] - runs[best].centre) <= (runs[best].count[:, None] + 2) * U * np.abs(x).max()).all()


# ---- end to end
def test_the_stage_end_to_end(tmp_path, monkeypatch, capsys):
    temp, z, hot, pe, vol = two_phase_grid()
    prefix = str(tmp_path / 'cl.lj.fcc.lammps')
    np.save(prefix + '.virial.trgt.npy', np.linspace(1, 2, PN, dtype=np.float32))
    np.save(prefix + '.temp.trgt.npy', temp)
    np.save(prefix + '.pe.npy', pe.astype(np.float32))
    np.save(prefix + '.vol.npy', vol.astype(np.float32))
    np.save(prefix + '.natoms.npy', np.full(hot.shape, NATOMS, dtype=np.uint16))
    np.save(prefix + '.cdf.pcz.npy', z)
    monkeypatch.chdir(tmp_path)
    assert cluster.main(['-v', '-n', 'cl', '-cl', 'kmeans', '-nc', '2']) == 0
    said = capsys.readouterr().out
    assert 'best restart' in said and 'warning' not in said
    assert not os.path.exists(prefix + '.cdf.cld.npy')
    out = {key: np.load(prefix + '.cdf.%s.npy' % key) for key in ('cll', 'cls', 'clr', 'cl0', 'cl1')}
    assert out['cll'].shape == hot.shape and out['cll'].dtype == np.int32 and out['clr'].shape == (10, 3) and out['clr'].dtype == np.float64
    assert out['cls'].shape == (2, 5) and (out['cls'][:, 0] == out['cls'][:, 1]).all() and out['cls'][:, 0].sum() == hot.size
    assert (out['clr'][:, 2] <= 1).all() and (out['clr'][:, 1] >= 1).all() and (out['clr'][:, 0] > 0).all()
    # cl0 is the cold blob and cl1 the hot one, whichever cluster began where
    np.testing.assert_array_equal(out['cl0'], (~hot).astype(np.float64))
    np.testing.assert_array_equal(out['cl1'], hot.astype(np.float64))
    np.testing.assert_array_equal(out['cll'] == out['cll'][0, 0, 0], hot == hot[0, 0, 0])
    # the labels are the restatement's from the same seeds on the same scaled points
    zs = cluster.scaled(z[..., :2].reshape(-1, 2))
    tol = 1e-4 * zs.var(axis=0).mean()
    runs = [R.lloyd(zs, s, 300, tol) for s in cluster.seeds(zs, 2, 10, 256)]
    assert all(run.margin > 1e-9 for run in runs)
    np.testing.assert_array_equal(out['clr'][:, 1:], [[run.iters, run.status] for run in runs])
    np.testing.assert_allclose(out['clr'][:, 0], [run.inertia for run in runs], rtol=1e-12)
    # the liquid's indicator through reweight: the weight at or above 0.5 crosses 1/2 between the two mixed columns
    assert reweight.main(['-n', 'cl', '-e', 'LJ', '-tg', '33', '-ob', 'cdf.cl1', '-hq', 'cdf.cl1', '-hx', '0.5']) == 0
    rwe = np.load(prefix + '.rwe.npy')
    assert rwe.shape == (PN,) and ((temp[1] < rwe) & (rwe < temp[2])).all()
    # DBSCAN as before: the files it writes today, .F.clr.npy is not among them
    os.remove(prefix + '.cdf.clr.npy')
    assert cluster.main(['-n', 'cl', '-cl', 'dbscan', '-nc', '0.1', '-ms', '5']) == 0
    assert all(os.path.exists(prefix + '.cdf.%s.npy' % key) for key in ('cll', 'cld', 'cls', 'cl0', 'cl1'))
    assert not os.path.exists(prefix + '.cdf.clr.npy') and np.load(prefix + '.cdf.cld.npy').shape == hot.shape
