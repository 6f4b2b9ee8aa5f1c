"""What tests/test_scan_big_gpu.py stands on, without a GPU.

The references of tests/scan_big_ref.py (a KD-tree for the pairs, grouped sums for the gradient) equal the dense restatements
tests/cluster_ref.py and tests/tsne_ref.py at the sizes those reach, so the two families cannot be wrong together with the kernels.

The regimes.  csrc/nm_scan.h's scan_grid gives one column slice per tile for every N up to 16384 (cluster) and 11520 (manifold):
every size the suite ran before these tests lies there, and a workgroup walked exactly one tile.  Each case of
tests/scan_big_cases.py is asserted to lie where it claims: the term of scan_grid that sets its slices and the fewest and the most
tiles that a slice walks, for the border pass too (its rows are the points that are not core, counted by the reference)."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import cluster_ref
import scan_big_cases as C
import scan_big_ref as K
import scan_cases
import tsne_ref
from test_cluster_gpu import BLOBS, grid_blobs
from test_tsne_gpu import grid_points

U = 2.0 ** -53
G = C.G
SIZES = (1, 2, 255, 257, 513, 1287)
NDS = (1, 2, 3, 16)


# ---- the references against the dense ones
@pytest.mark.parametrize('nd', NDS)
@pytest.mark.parametrize('n', SIZES)
def test_dbscan_kd_is_the_dense_restatement(n, nd):
    x = grid_blobs(n, nd, 100 * nd + n)
    eps = round(0.45 * nd ** 0.5 / (8 * G)) * (8 * G)           # test_ragged_sizes' choice: pairs on the bound occur
    for min_pts in (1, 4, 9):
        label, degree, ncl = K.dbscan_kd(x, eps, min_pts)
        rl, rd, rn = cluster_ref.dbscan(x, eps, min_pts)
        assert label.dtype == rl.dtype and degree.dtype == rd.dtype
        np.testing.assert_array_equal(degree, rd)
        np.testing.assert_array_equal(label, rl)
        assert ncl == rn
    if n >= 255:
        assert cluster_ref.margin(x, eps) == 0.0
        core = rd >= 9
        assert core.any() and (~core & (rl >= 0)).any() and (rl < 0).any()      # cores, borders and noise


def test_dbscan_kd_on_the_plane_in_sixteen_dimensions():
    """the kind of input of the nd = 16 case, at a size the dense restatement reaches"""
    rng = np.random.default_rng(5)
    z = np.round(40.0 * rng.standard_normal((1287, 2)))
    x = (z @ rng.integers(-1, 2, (2, 16)).astype(np.float64)) * G
    label, degree, ncl = K.dbscan_kd(x, 12 * G, 5)
    rl, rd, rn = cluster_ref.dbscan(x, 12 * G, 5)
    np.testing.assert_array_equal(degree, rd)
    np.testing.assert_array_equal(label, rl)
    assert ncl == rn >= 2 and (rl < 0).any()


@pytest.mark.parametrize('nd', NDS)
@pytest.mark.parametrize('n', SIZES[1:])
def test_neighbours_kd_is_the_dense_restatement(n, nd):
    x = grid_points(n, nd, 7 * n + nd)
    d2 = cluster_ref.d2_matrix(x)
    for k in sorted({1, min(9, n - 1), min(65, n - 1)}):
        nbr, complete, tied = K.neighbours_kd(x, k, extra=n)     # every point a candidate: complete by construction
        assert complete.all() and nbr.dtype == np.int32
        np.testing.assert_array_equal(nbr, tsne_ref.neighbours(d2, k))
        if n > k + 1:
            order = np.sort(d2 + np.diag(np.full(n, -1.0)), axis=1)            # the row itself in front
            np.testing.assert_array_equal(tied, order[:, k] == order[:, k + 1])
        # with the candidates the large cases use: where the flag holds the rows are the same
        few, flag, _ = K.neighbours_kd(x, k)
        np.testing.assert_array_equal(few[flag], nbr[flag])


def test_neighbours_kd_says_where_its_candidates_do_not_suffice():
    """40 copies of one point: 25 candidates cannot hold the ties of k = 3; a point far off sees them all at one distance"""
    x = np.concatenate([np.zeros((40, 2)), [[1.0, 0.0]], [[5.0, 5.0]]])
    nbr, complete, tied = K.neighbours_kd(x, 3, extra=21)
    assert not complete.any() and tied[:40].all()
    nbr, complete, tied = K.neighbours_kd(x, 3, extra=64)
    assert complete.all()
    np.testing.assert_array_equal(nbr, tsne_ref.neighbours(cluster_ref.d2_matrix(x), 3))


@pytest.mark.parametrize('nc', (1, 2, 3))
@pytest.mark.parametrize('n', (257, 1287))
def test_gradient_grouped_is_the_dense_restatement(n, nc):
    """Both add the same terms in float64 in another order.  The dense one adds a row's N terms in sequence (numpy adds pairwise
    along the contiguous axis only, and a row's terms lie along the other one): at most N roundings of the sum of their magnitudes,
    mag, and about sqrt(N) of them in practice.  The grouped one adds LOCATIONS repulsive terms and a row's attractive ones in
    sequence; each term carries a multiplicity or a division by Z rounded apart: 8 roundings cover those.  So the difference is the
    dense restatement's own error, which the figures printed below show: the grouped sums are the more exact of the two."""
    k = 9
    x = grid_points(n, 2, 7 * n)
    nbr, complete, _ = K.neighbours_kd(x, k, extra=n)
    rng = np.random.default_rng(n + nc)
    p = rng.random((n, k)) + 0.01
    p /= p.sum(axis=1, keepdims=True)
    p[rng.random((n, k)) < 0.05] = 0.0                           # a listed pair may carry no weight
    deg = np.bincount(K.symmetric(nbr, p)[0], minlength=n).max()
    for name, scale in C.SCALES.items():
        centres, member = C.grouped_embedding(n, nc, scale, 11 * nc)
        assert len(np.unique(member)) == C.LOCATIONS and np.bincount(member).max() > 1          # coincident points: w = 1
        for ex in (1.0, 12.0):
            grad, kl, z, mag, klmag = K.gradient_grouped(nbr, p, centres, member, ex)
            rg, rkl, rz, rmag, rklmag = tsne_ref.gradient(nbr, p, centres[member], ex)
            c = (n + C.LOCATIONS + deg + 8) * U
            worst = (np.abs(grad - rg) / (c * rmag)).max()
            print('%s, N %d, ncomp %d, exaggeration %g: largest difference %.3g of the bound' % (name, n, nc, ex, worst))
            assert worst <= 1.0
            assert (np.abs(mag - rmag) <= c * rmag).all()
            assert abs(z - rz) <= c * rz
            assert abs(kl - rkl) <= c * rklmag and abs(klmag - rklmag) <= c * rklmag


# ---- the regimes
def test_scan_grid_restated():
    assert C.shape('cluster') == dict(ROWS=512, TILE=256, GRID=2048, SPAN=128)
    assert C.shape('tsne') == dict(ROWS=512, TILE=128, GRID=2048, SPAN=256)
    g = C.scan_grid('cluster', 1287, 1287)
    assert (g['blocks'], g['tiles'], g['slices'], g['limb'], g['walk']) == (3, 6, 6, 'TILES', (1, 1))
    g = C.scan_grid('tsne', 1159, 1159)
    assert (g['blocks'], g['tiles'], g['slices'], g['limb'], g['walk']) == (3, 10, 10, 'TILES', (1, 1))
    g = C.scan_grid('cluster', 100000, 100000)                  # production: about 36 tiles per workgroup
    assert g['limb'] == 'GRID' and g['walk'] == (35, 36)


def test_every_size_before_these_tests_walks_one_tile():
    """the whole range, so also every size of test_cluster_gpu.py, test_tsne_gpu.py and scan_cases.py; the border pass has fewer
    row blocks than the others and so at least as many slices"""
    for stage, last in (('cluster', 16384), ('tsne', 11520)):
        for n in range(1, last + 1):
            g = C.scan_grid(stage, n, n)
            assert g['limb'] == 'TILES' and g['walk'] == (1, 1), (stage, n)
        assert C.scan_grid(stage, last + 1, last + 1)['walk'] == (1, 2)
    before = [n for n, *_ in BLOBS.values()] + list(scan_cases.CL_N) + [3001, 900, 9 * 257, 2 * 512 + 256 + 7]
    assert max(before) == 3001 <= 16384
    for n in before:
        for nopen in (1, max(1, n // 2), n):
            assert C.scan_grid('cluster', nopen, n)['walk'] == (1, 1)
    assert max(scan_cases.AF_N + scan_cases.GR_N + (2 * 512 + 128 + 7, 2 * 128 + 3 + 2 * (64 + 1))) == 1159 <= 11520


@pytest.mark.parametrize('n', sorted(C.CLUSTER_REGIME))
def test_the_cluster_cases_lie_where_they_claim(n):
    blocks, tiles, slices, limb, walk, last, nopen_min = C.CLUSTER_REGIME[n]
    g = C.scan_grid('cluster', n, n)
    assert (g['blocks'], g['tiles'], g['slices'], g['limb'], g['walk'], g['last']) == (blocks, tiles, slices, limb, walk, last)
    assert walk[0] < walk[1] and last < C.shape('cluster')['TILE']              # ragged: unequal slices, a partial last tile
    # the union pass walks the tiles up to a row block's own: row block 0 has fewer of them than there are slices (blockIdx.y >= tend)
    assert g['slices'] > C.shape('cluster')['ROWS'] // C.shape('cluster')['TILE']
    for (cn, nd) in sorted(C.CLUSTER_CASES):
        if cn != n:
            continue
        x, eps, min_pts = C.cluster_points(n, nd)
        label, degree, ncl = C.cluster_reference(n, nd)
        core = degree >= min_pts
        nopen = int((~core).sum())
        shares = core.mean(), (~core & (label >= 0)).mean(), (label < 0).mean()
        print('N %d, nd %d: %d clusters, core %.3f, border %.3f, noise %.3f, %d points that are not core' % ((n, nd, ncl) + shares + (nopen,)))
        assert x.shape == (n, nd) and ncl >= 2 and min(shares) >= 0.02
        assert len(np.unique(x, axis=0)) < n                                    # duplicated points
        if nopen_min is not None:                                               # the border pass walks several tiles too
            assert nopen >= nopen_min
            b = C.scan_grid('cluster', nopen, n)
            assert b['slices'] < b['tiles'] and b['limb'] in ('GRID', 'SPAN') and b['walk'][1] >= 2
            assert b['walk'] == walk or n == 40007                              # at 196616 as many tiles as in the other passes
    if nopen_min is not None:
        assert C.scan_grid('cluster', nopen_min, n)['slices'] < tiles


def test_the_cluster_cases_have_pairs_on_the_bound():
    """at the smallest size, where the candidates are few: pairs at exactly eps exist (eps is a whole number of grid steps)"""
    for nd in (1, 2, 3, 16):
        x, eps, min_pts = C.cluster_points(16392, nd)
        pairs = cKDTree(x).query_pairs(eps * (1 + 2.0 ** -20), output_type='ndarray')
        d2 = K.d2_pairs(x, pairs[:, 0], pairs[:, 1])
        assert (d2 == eps * eps).sum() >= 16, nd


@pytest.mark.parametrize('n', sorted(C.TSNE_REGIME))
def test_the_manifold_cases_lie_where_they_claim(n):
    blocks, tiles, slices, limb, walk = C.TSNE_REGIME[n]
    g = C.scan_grid('tsne', n, n)
    assert (g['blocks'], g['tiles'], g['slices'], g['limb'], g['walk']) == (blocks, tiles, slices, limb, walk)
    assert walk[0] < walk[1] and g['last'] < C.shape('tsne')['TILE']
    own = C.shape('tsne')['ROWS'] // C.shape('tsne')['TILE']
    if walk[0] >= 2:                            # a slice holds own and foreign tiles of a row block together
        assert slices > own or walk[0] > own


@pytest.mark.parametrize('k', C.AF_K)
@pytest.mark.parametrize('nd', C.AF_ND)
@pytest.mark.parametrize('n', C.AF_N)
def test_the_neighbour_lists_of_the_large_cases_are_complete(n, nd, k):
    """the condition on the reference: the tree's candidates decide every row.  Duplicates and ties at the k-th distance abound."""
    x = C.affinity_points(n, nd)
    nbr, complete, tied = C.affinity_reference(n, nd, k)
    assert complete.all(), (~complete).sum()
    assert nbr.shape == (n, k) and (nbr != np.arange(n)[:, None]).all()
    assert len(np.unique(x, axis=0)) <= n - n // 100 and tied.mean() >= 0.25
    rows = np.arange(n)[:, None]
    d = K.d2_pairs(x, rows, nbr.astype(np.int64))
    assert (np.diff(d, axis=1) >= 0).all()
    same = np.diff(d, axis=1) == 0
    assert (np.diff(nbr.astype(np.int64), axis=1)[same] > 0).all()              # ties in ascending index
