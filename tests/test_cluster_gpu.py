"""The cluster stage on the GPU (include/nm_cluster.h): nm_cluster_dbscan on sentinel-filled outputs, label, degree and nclusters
equal to tests/cluster_ref.py on every case: ragged sizes around the tile and the row block, exact data with pairs on the bound, a
chain across every tile, borders between two clusters, both extremes of min_pts, random blobs off ties, a relabelling, two calls,
values that are not finite; and neuralmelting_amd.cluster end to end on a synthetic two-phase grid, through reweight."""
import functools
import os
import re

import numpy as np
import pytest

import cluster_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import cluster, reweight

pytestmark = pytest.mark.gpu

SENT = -77
T, ROWS = 256, 512          # csrc/nm_cluster.h: the columns of a tile, the rows of a workgroup (pinned below)
G = 2.0 ** -8               # the grid of the exact data: coordinates are multiples of it, |x| <= 64, so d2 and eps^2 are exact


def test_the_tile_is_what_the_cases_assume():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'neuralmelting_amd', 'csrc', 'nm_cluster.h')).read()
    const = {k: v for k, v in re.findall(r'constexpr int (CL_\w+) = ([^;]+);', src)}
    assert int(const['CL_TILE']) == T and int(const['CL_BLOCK']) == 256 and int(const['CL_RPT']) == 2 and const['CL_ROWS'] == 'CL_RPT * CL_BLOCK'
    assert ROWS == 2 * 256


def raw(x, eps, min_pts):
    """the raw ABI on sentinel-filled outputs: rc, message, (label, degree, nclusters)"""
    L = B.load()
    x = np.ascontiguousarray(x, dtype=np.float64)
    n, nd = x.shape
    out = (np.full(n, SENT, np.int32), np.full(n, SENT, np.int32), np.full(1, SENT, np.int32))
    rc = L.nm_cluster_dbscan(0, n, nd, x.ctypes.data_as(B.c_double_p), eps, min_pts, *[o.ctypes.data_as(B.c_int32_p) for o in out])
    return rc, (L.nm_cluster_last_error().decode() if rc else ''), out


def check(x, eps, min_pts, ref=None):
    """the device's results, after they have been found equal to the restatement's (ref, where the caller holds them already)"""
    rc, msg, (label, degree, ncl) = raw(x, eps, min_pts)
    assert rc == B.NM_OK, msg
    rl, rd, rn = ref or R.dbscan(x, eps, min_pts)
    np.testing.assert_array_equal(degree, rd)
    np.testing.assert_array_equal(label, rl)
    assert ncl[0] == rn
    return label, degree, int(ncl[0])


def grid_blobs(n, nd, seed, k=3):
    """k blobs and a scattered tenth, rounded to the grid: every distance is exact, pairs on the bound and duplicates occur"""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-3.0, 3.0, (k, nd))
    x = centre[rng.integers(0, k, n)] + 0.4 * rng.standard_normal((n, nd))
    x[: n // 10] = rng.uniform(-5.0, 5.0, (n // 10, nd))
    return np.round(x[rng.permutation(n)] / (8 * G)) * (8 * G)


# ---- ragged sizes: the tile's and the row block's edges, one column slice and several, one row block and several
@pytest.mark.parametrize('nd', (1, 2, 3, 8, 16))
@pytest.mark.parametrize('n', (1, 2, T - 1, T, T + 1, 2 * T + 3, ROWS - 1, ROWS + 1, 2 * ROWS + T + 7))
def test_ragged_sizes(n, nd):
    x = grid_blobs(n, nd, 100 * nd + n)
    eps = round(0.45 * nd ** 0.5 / (8 * G)) * (8 * G)
    label, degree, ncl = check(x, eps, 4)
    if n > T:
        assert ncl >= 1 and (degree < 4).any() and degree.max() >= 4         # the case holds cores and points that are not


# ---- exact data
def test_pairs_on_the_bound_are_neighbours_and_a_grid_step_beyond_they_are_not():
    """a 3-4-5 triangle scaled by 1/4: B lies at exactly eps = 1.25 from A, C one grid step beyond; E and F the same along an axis;
    D is A again"""
    a = np.array([37.5, -12.25])
    pts = np.array([[0.0, 0.0], [0.75, 1.0], [0.75 + G, 1.0], [0.0, 0.0], [-1.25, 0.0], [-1.25 - G, 0.0]]) + a
    assert R.margin(pts, 1.25) == 0.0
    label, degree, ncl = check(pts, 1.25, 4)
    np.testing.assert_array_equal(degree, [4, 4, 2, 4, 4, 2])               # A: A D B E; B: B C A D; C: C B; E: E F A D; F: F E
    np.testing.assert_array_equal(label, [0, 0, 0, 0, 0, 0])                # C and F are borders
    assert ncl == 1
    label, degree, ncl = check(pts, 1.25 + G, 4)                            # the step wider: C and F reach A and D
    np.testing.assert_array_equal(degree, [6, 4, 4, 6, 4, 4])
    label, degree, ncl = check(pts, 1.25 - G, 3)                            # the step narrower: three pairs apart
    np.testing.assert_array_equal(degree, [2, 2, 2, 2, 2, 2])
    np.testing.assert_array_equal(label, [-1] * 6)


def test_duplicated_points():
    x = np.repeat(grid_blobs(300, 2, 7), 3, axis=0)[np.random.default_rng(8).permutation(900)]
    label, degree, ncl = check(x, 32 * G, 6)
    assert (degree % 3 == 0).all()                                          # every neighbour comes three times
    label, degree, ncl = check(x, G / 2, 3)                                 # nothing but the copies of a point within eps
    assert (degree >= 3).all() and (label >= 0).all() and ncl == len(np.unique(x, axis=0))


# ---- a chain across every tile: one component whose diameter is its length
def chain(shuffled, stretched, n=3001):
    pos = np.arange(n) / 64.0                                               # spaced exactly eps = 1 / 64
    if stretched:
        pos[n // 2 + 13:] += G                                              # one link a grid step longer
    x = np.stack([pos, np.full(n, 0.5)], axis=1)
    return x[np.random.default_rng(3).permutation(n)] if shuffled else x


@pytest.mark.parametrize('stretched', (False, True))
@pytest.mark.parametrize('min_pts', (2, 3))
@pytest.mark.parametrize('shuffled', (True, False))
def test_chain(shuffled, min_pts, stretched):
    x = chain(shuffled, stretched)
    assert x[:, 0].max() <= 64.0 and R.margin(x, 1.0 / 64) == 0.0
    label, degree, ncl = check(x, 1.0 / 64, min_pts)
    assert ncl == (2 if stretched else 1) and (label >= 0).all()
    assert sorted(np.bincount(degree)[1:].nonzero()[0] + 1) == [2, 3]       # the ends have one neighbour, the others two
    assert (degree == 2).sum() == (4 if stretched else 2)


# ---- borders and noise
def test_a_border_between_two_clusters_takes_the_lower_number():
    """1-D, eps 1, min_pts 4: two groups of four cores, b = 2 within eps of a core of each and itself not core (b, 1, 3: three);
    two points far off with each other only: noise"""
    low, high, b, far = [0.0, 0.25, 0.5, 1.0], [3.0, 3.5, 3.75, 4.0], [2.0], [10.0, 10.5]
    x = np.array(high + b + low + far)[:, None]                             # the high group holds the smallest index: cluster 0
    label, degree, ncl = check(x, 1.0, 4)
    np.testing.assert_array_equal(label, [0, 0, 0, 0, 0, 1, 1, 1, 1, -1, -1])
    assert degree[4] == 3 and list(degree[-2:]) == [2, 2] and ncl == 2
    x = np.array(far + low + b + high)[:, None]                             # now the low group does
    label, degree, ncl = check(x, 1.0, 4)
    np.testing.assert_array_equal(label, [-1, -1, 0, 0, 0, 0, 0, 1, 1, 1, 1])


def test_borders_across_tiles():
    """the same groups T + 1 times over, at shuffled indices: a border's two clusters lie in other tiles and other row blocks"""
    unit = np.array([0.0, 0.25, 0.5, 1.0, 2.0, 3.0, 3.5, 3.75, 4.0])
    x = (unit[None, :] + 8.0 * np.arange(T + 1)[:, None] - 1000.0).reshape(-1, 1) / 32
    x = x[np.random.default_rng(4).permutation(x.shape[0])]
    label, degree, ncl = check(x, 1.0 / 32, 4)
    assert ncl == 2 * (T + 1) and (label >= 0).all() and (degree == 3).sum() == T + 1


# ---- both extremes of min_pts
def test_min_pts_extremes():
    x = grid_blobs(2 * T + 3, 3, 17)
    eps = 48 * G
    label, degree, ncl = check(x, eps, 1)                                   # every point is core: the labels are the components
    assert (label >= 0).all() and ncl == label.max() + 1
    first = np.array([np.nonzero(label == c)[0][0] for c in range(ncl)])
    assert (np.diff(first) > 0).all()                                       # numbered by their smallest index
    label, degree, ncl = check(x, eps, x.shape[0] + 1)                      # nobody is
    assert (label == -1).all() and ncl == 0
    label, degree, ncl = check(x, 1e3, x.shape[0])                          # everybody sees everybody
    assert (degree == x.shape[0]).all() and (label == 0).all() and ncl == 1


# ---- random blobs, off ties
BLOBS = {'2-blobs-2d': (1500, 2, 2, 0.25, 5, 31), '3-blobs-3d': (2500, 3, 3, 0.5, 6, 32), '4-blobs-8d': (3000, 8, 4, 1.6, 8, 33),
         '3-blobs-16d': (1100, 16, 3, 2.6, 5, 34), '2-blobs-1d': (700, 1, 2, 0.05, 4, 35)}


@functools.lru_cache(maxsize=None)
def blobs(case):
    n, nd, k, eps, min_pts, seed = BLOBS[case]
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-4.0, 4.0, (k, nd))
    x = centre[rng.integers(0, k, n)] + 0.5 * rng.standard_normal((n, nd))
    x[: n // 10] = rng.uniform(-6.0, 6.0, (n // 10, nd))
    x = x[rng.permutation(n)]
    x.setflags(write=False)
    return x, eps, min_pts


@functools.lru_cache(maxsize=None)
def blobs_reference(case):
    """the restatement's results for a case and the margin of its input: computed once"""
    x, eps, min_pts = blobs(case)
    return R.dbscan(x, eps, min_pts), R.margin(x, eps)


@pytest.mark.parametrize('case', sorted(BLOBS))
def test_random_blobs(case):
    """d2's error is below 18 u = 2e-15 of itself; the nearest pair stands 1e-12 of eps^2 off the bound, three orders above that:
    the device and the restatement put every pair on the same side, however each rounds"""
    x, eps, min_pts = blobs(case)
    ref, margin = blobs_reference(case)
    assert margin > 1e-12, 'the input of %s has a pair on the bound: choose another seed' % case
    label, degree, ncl = check(x, eps, min_pts, ref)
    assert 2 <= ncl and (label == -1).any() and ((label >= 0) & (degree < min_pts)).any()       # clusters, noise and borders


# ---- relabelling and determinism
def test_a_permutation_of_the_points_permutes_the_result():
    x, eps, min_pts = blobs('3-blobs-3d')
    label, degree, ncl = check(x, eps, min_pts, blobs_reference('3-blobs-3d')[0])
    p = np.random.default_rng(9).permutation(x.shape[0])
    pl, pd, pn = check(x[p], eps, min_pts)                                  # and so the numbering follows the smallest core index
    assert pn == ncl
    np.testing.assert_array_equal(pd, degree[p])
    core = degree >= min_pts
    np.testing.assert_array_equal(pl < 0, (label < 0)[p])
    # the cores' partition is the same (a border between two clusters may change sides with the numbering)
    pairs = set(zip(label[p][core[p]].tolist(), pl[core[p]].tolist()))
    assert len(pairs) == ncl == len({a for a, _ in pairs}) == len({b for _, b in pairs})


def test_two_calls_give_the_same_bytes():
    x, eps, min_pts = blobs('4-blobs-8d')
    one, two = raw(x, eps, min_pts), raw(x, eps, min_pts)
    assert one[0] == two[0] == B.NM_OK
    for a, b in zip(one[2], two[2]):
        assert a.tobytes() == b.tobytes()
    ms = np.full(5, -1.0)
    assert B.load().nm_cluster_last_timing(ms.ctypes.data_as(B.c_double_p)) == B.NM_OK
    assert (ms >= 0.0).all() and ms[1] > 0.0 and ms[2] > 0.0 and ms[4] > 0.0


# ---- a value that is not finite
@pytest.mark.parametrize('bad', (np.nan, np.inf, -np.inf))
def test_a_value_that_is_not_finite_is_refused(bad):
    x = np.array(blobs('2-blobs-2d')[0])
    x[-1, 1] = bad
    rc, msg, out = raw(x, 0.25, 5)
    assert rc == B.NM_ERR_ARG and msg.startswith('nm_cluster_dbscan:') and msg.endswith('point %d' % (x.shape[0] - 1)), msg
    assert all((o == SENT).all() for o in out)
    x[T + 5, 0] = bad                                                       # the first of two is named
    rc, msg, out = raw(x, 0.25, 5)
    assert rc == B.NM_ERR_ARG and msg.endswith('point %d' % (T + 5)) and all((o == SENT).all() for o in out), msg


# ---- end to end
PN, TN, SN, LD, NATOMS = 2, 4, 100, 3, 32
HOT_SHARE = (0.0, 0.25, 0.75, 1.0)          # of the samples of a temperature column: the two in the middle are mixed


def two_phase_grid():
    """pcz: a cold blob at pc0 = -1 and a hot one at +1, both 0.15 wide; hot (PN, TN, SN) says which sample lies in which.  The
    energy of a hot sample is higher by NATOMS / 2, as a latent heat would make it."""
    rng = np.random.default_rng(41)
    temp = np.linspace(1, 2, TN, dtype=np.float32)
    hot = np.stack([np.stack([rng.permutation(SN) < round(share * SN) for share in HOT_SHARE]) for _ in range(PN)])
    z = 0.15 * rng.standard_normal((PN, TN, SN, LD))
    z[..., 0] += np.where(hot, 1.0, -1.0)
    z[..., 2] *= 20.0                                                       # a component that -nd 2 leaves out
    pe = -5.0 * NATOMS + 1.5 * NATOMS * temp[None, :, None] + 0.5 * NATOMS * hot + np.sqrt(1.5 * NATOMS) * temp[None, :, None] * rng.normal(size=hot.shape)
    vol = NATOMS * (1.0 + 0.1 * temp[None, :, None]) + rng.normal(size=hot.shape)
    return temp, z, hot, pe, vol


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
    assert cluster.main(['-v', '-n', 'cl', '-nc', '0.1', '-ms', '5', '-nk', '3']) == 0
    said = capsys.readouterr().out
    assert '2 clusters' in said and 'cl2 .. cl2 are all zero' in said
    out = {key: np.load(prefix + '.cdf.%s.npy' % key) for key in ('cll', 'cld', 'cls', 'cl0', 'cl1', 'cl2')}
    assert out['cll'].shape == out['cld'].shape == hot.shape and out['cll'].dtype == out['cld'].dtype == np.int32
    assert out['cls'].shape == (2, 5) and out['cls'].dtype == np.float64
    assert all(out[k].shape == hot.shape and out[k].dtype == np.float64 for k in ('cl0', 'cl1', 'cl2'))
    # the labels are the restatement's on the same scaled points
    zs = cluster.scaled(z[..., :2].reshape(-1, 2))
    rl, rd, rn = R.dbscan(zs, 0.1, 5)
    assert R.margin(zs, 0.1) > 1e-12 and rn == 2
    np.testing.assert_array_equal(out['cll'].reshape(-1), rl)
    np.testing.assert_array_equal(out['cld'].reshape(-1), rd)
    # cl0 is the cold blob and cl1 the hot one, whichever was numbered first; at most a few stragglers are noise
    noise = out['cll'] < 0
    assert noise.mean() < 0.02
    np.testing.assert_array_equal(out['cl0'], (~hot & ~noise).astype(np.float64))
    np.testing.assert_array_equal(out['cl1'], (hot & ~noise).astype(np.float64))
    assert (out['cl2'] == 0.0).all() and not os.path.exists(prefix + '.cdf.cl3.npy')
    cold_label = int(out['cll'][0, 0][~noise[0, 0]][0])
    tab = out['cls']
    assert tab[cold_label, 2] < tab[1 - cold_label, 2] and tab[cold_label, 3] < 0.0 < tab[1 - cold_label, 3]      # centroids as written, unscaled
    assert tab[:, 0].sum() == (~noise).sum() and (tab[:, 1] <= tab[:, 0]).all()
    # the liquid's indicator through the existing stage: the weight at or above 0.5 crosses 1/2 between the two mixed columns
    np.testing.assert_array_equal(reweight.load_observables(prefix, ['cdf.cl1'], hot.shape)[0], out['cl1'])
    assert reweight.main(['-n', 'cl', '-e', 'LJ', '-tg', '33', '-ob', 'cdf.cl1', '-hq', 'cdf.cl1', '-hx', '0.5']) == 0
    rwe = np.load(prefix + '.rwe.npy')
    print('equal weight at T = %s, the mixed columns at %g and %g' % (rwe, temp[1], temp[2]))
    assert rwe.shape == (PN,) and ((temp[1] < rwe) & (rwe < temp[2])).all()


def test_samples_left_out_of_the_clustering(tmp_path, monkeypatch):
    temp, z, hot, pe, vol = two_phase_grid()
    prefix = str(tmp_path / 'cl.lj.fcc.lammps')
    np.save(prefix + '.virial.trgt.npy', np.linspace(1, 2, PN, dtype=np.float32))
    np.save(prefix + '.temp.trgt.npy', temp)
    np.save(prefix + '.pe.npy', pe.astype(np.float32))
    np.save(prefix + '.cdf.pcz.npy', z)
    monkeypatch.chdir(tmp_path)
    assert cluster.main(['-n', 'cl', '-nc', '0.15', '-ms', '4', '-sk', '10', '-sd', '3', '-nd', '1']) == 0
    cll, cld, cl0, cl1 = (np.load(prefix + '.cdf.%s.npy' % k) for k in ('cll', 'cld', 'cl0', 'cl1'))
    zs = cluster.scaled(np.ascontiguousarray(z[:, :, 10::3, :1]).reshape(-1, 1))
    rl, rd, rn = R.dbscan(zs, 0.15, 4)
    assert R.margin(zs, 0.15) > 1e-12
    np.testing.assert_array_equal(cll[:, :, 10::3].reshape(-1), rl)
    np.testing.assert_array_equal(cld[:, :, 10::3].reshape(-1), rd)
    out = np.ones(SN, dtype=bool)
    out[10::3] = False
    assert (cll[:, :, out] == -1).all() and (cld[:, :, out] == 0).all() and (cl0[:, :, out] == 0).all() and (cl1[:, :, out] == 0).all()
    assert cl0[:, :, 10::3].sum() > 0 and cl1[:, :, 10::3].sum() > 0 and not os.path.exists(prefix + '.cdf.cl2.npy')
