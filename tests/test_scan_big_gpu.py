"""The all-pairs scans of the cluster and the manifold stage (csrc/nm_scan.h, cl_scan, ts_scan) where a workgroup walks several
tiles: the second and every later trip of the tile loop, the barrier in front of a tile that protects the one before, the stride
of a slice, a wave that has nothing to do with tiles behind it, a slice that holds a row block's own tiles and foreign ones, row
blocks of the union pass that have fewer tiles than there are slices, and partial sums of the pairs pass that add many tiles.
Every size the suite ran before gives one slice per tile, so each of these ran for the first and only trip.  Production lies
here: at 100 000 samples a cluster workgroup walks 36 tiles.

The sizes are the smallest that reach each regime and ragged (a partial last tile, slices of unequal length); tests/test_scan_big.py
asserts on the CPU that they lie where they claim, and that the references of tests/scan_big_ref.py, which cost no N^2, equal the
dense restatements where those reach.  Cluster: label, degree and nclusters equal, entry for entry, on exact data with pairs on the
bound.  Manifold: the neighbours entry for entry on exact data with duplicates and ties at the k-th distance; beta and p by the
properties of test_beta_and_p_by_their_properties that need no search on the host (the row kernel does not depend on the tiling and
is pinned at small N); the gradient, Z and kl within the header's bounds against sums grouped by location; the descent bit for bit
against rounds of the gradient.

The SPAN term of scan_grid is reached at N = 196616 by the cluster stage and the gradient.  The affinities are left at the GRID
term: their 64 counting scans of 3.9e10 pairs each are the same kernel on the same kind of grid, and the kernels do not know
which term chose it."""
import functools

import numpy as np
import pytest

import scan_big_cases as C
import scan_big_ref as K
import tsne_ref
from neuralmelting_amd import _lib as B
from neuralmelting_amd import manifold
from test_cluster_gpu import SENT, raw
from test_tsne_gpu import affinities_raw, device_norm

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


# ---- the cluster stage
def check_cluster(x, eps, min_pts, ref):
    rc, msg, (label, degree, ncl) = raw(x, eps, min_pts)
    assert rc == B.NM_OK, msg
    rl, rd, rn = ref
    np.testing.assert_array_equal(degree, rd)
    np.testing.assert_array_equal(label, rl)
    assert ncl[0] == rn
    return label, degree, int(ncl[0])


@pytest.mark.parametrize('case', sorted(C.CLUSTER_CASES), ids=C.cluster_key)
def test_dbscan_where_a_workgroup_walks_several_tiles(case):
    x, eps, min_pts = C.cluster_points(*case)
    label, degree, ncl = check_cluster(x, eps, min_pts, C.cluster_reference(*case))
    assert not (label == SENT).any() and ncl >= 2


@pytest.mark.parametrize('shuffled', (True, False))
@pytest.mark.parametrize('min_pts', (2, 3))
@pytest.mark.parametrize('n', C.CHAIN_N)
def test_a_chain_across_every_tile_and_every_slice(n, min_pts, shuffled):
    x, eps, pos = C.chain(n, shuffled)
    label, degree, ncl = check_cluster(x, eps, min_pts, C.chain_reference(n, pos, min_pts))
    assert (degree == 2).sum() == 2


def test_two_calls_give_the_same_bytes_at_40007():
    x, eps, min_pts = C.cluster_points(40007, 2)
    one, two = raw(x, eps, min_pts), raw(x, eps, min_pts)
    assert one[0] == two[0] == B.NM_OK
    for a, b in zip(one[2], two[2]):
        assert a.tobytes() == b.tobytes()


def test_a_permutation_of_the_points_permutes_the_result_at_16392():
    x, eps, min_pts = C.cluster_points(16392, 3)
    label, degree, ncl = check_cluster(x, eps, min_pts, C.cluster_reference(16392, 3))
    p = np.random.default_rng(9).permutation(x.shape[0])
    xp = np.ascontiguousarray(x[p])
    pl, pd, pn = check_cluster(xp, eps, min_pts, K.dbscan_kd(xp, eps, min_pts))
    assert pn == ncl
    np.testing.assert_array_equal(pd, degree[p])
    core = degree >= min_pts
    np.testing.assert_array_equal(pl < 0, (label < 0)[p])
    # the cores' partition is the same (a border between two clusters may change sides with the numbering)
    pairs = set(zip(label[p][core[p]].tolist(), pl[core[p]].tolist()))
    assert len(pairs) == ncl == len({a for a, _ in pairs}) == len({b for _, b in pairs})


# ---- the manifold stage: affinities
PX = {9: 3.5, 65: 20.5}       # no whole numbers: a row with as many entries at dmin as the perplexity would hang on the last bit of a logarithm


@functools.lru_cache(maxsize=None)
def device_affinities(n, nd, k):
    rc, msg, out = affinities_raw(C.affinity_points(n, nd), PX[k], k)
    assert rc == B.NM_OK, msg
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize('k', C.AF_K)
@pytest.mark.parametrize('nd', C.AF_ND)
@pytest.mark.parametrize('n', C.AF_N)
def test_affinities_where_a_workgroup_walks_several_tiles(n, nd, k):
    x = C.affinity_points(n, nd)
    want, complete, tied = C.affinity_reference(n, nd, k)
    assert complete.all()                                       # the condition on the reference
    nbr, p, beta = device_affinities(n, nd, k)
    np.testing.assert_array_equal(nbr, want)
    # beta and p by their properties (the header's bounds), vectorised over the rows
    px, bnd = PX[k], int(np.ceil(k / 256)) + 32
    d = K.d2_pairs(x, np.arange(n)[:, None], nbr.astype(np.int64))
    t = d - d[:, :1]
    assert np.isfinite(beta).all() and (beta > 0).all() and np.isfinite(p).all() and (p >= 0).all()
    assert np.abs(p.sum(axis=1) - 1.0).max() <= bnd * U
    root = (t == 0.0).sum(axis=1) < px                          # fewer entries at dmin than the perplexity asks for
    assert root.sum() >= n // 2 and (beta[~root] == 2.0 ** 200).all()
    a = beta[root, None] * t[root]
    e = np.exp(-a)
    s = e.sum(axis=1, keepdims=True)
    want_p = e / s
    assert (np.abs(p[root] - want_p) <= 2 * (bnd + a) * U * want_p + 1e-300).all()
    h = np.log(s[:, 0]) + beta[root] * ((t[root] * e).sum(axis=1) / s[:, 0])
    hb = bnd * U * (1.0 + np.log(k) + np.where(want_p > 0.0, a * a * want_p, 0.0).sum(axis=1))
    worst = (np.abs(h - np.log(px)) / hb).max()
    print('N %d, ndim %d, k %d: %d rows tied at the k-th distance, %d without a root, largest |H - ln px| %.3g of its bound' % (
        n, nd, k, tied.sum(), (~root).sum(), worst))
    assert worst <= 1.0


# ---- the manifold stage: the gradient
def check_gradient(nbr, p, centres, member, ex):
    n, k = nbr.shape
    y = np.ascontiguousarray(centres[member])
    grad, kl, z = manifold.gradient(nbr, p, y, ex)
    rg, rkl, rz, mag, klmag = K.gradient_grouped(nbr, p, centres, member, ex)
    c = (3 * n + k + 64) * U
    err = np.abs(grad - rg)
    worst = (err / (c * mag + 1e-300)).max()
    print('Z off by %.3g of its bound, kl by %.3g, the gradient by %.3g' % (abs(z - rz) / (2 * (n + 64) * U * rz), abs(kl - rkl) / (c * klmag), worst))
    assert abs(z - rz) <= 2 * (n + 64) * U * rz, (z, rz)
    assert (err <= c * mag).all(), worst
    assert abs(kl - rkl) <= c * klmag, (kl, rkl, klmag)


@pytest.mark.parametrize('ex', (1.0, 12.0))
@pytest.mark.parametrize('nc', (1, 2, 3))
@pytest.mark.parametrize('n', C.AF_N)
def test_the_gradient_on_the_device_s_own_lists(n, nc, ex):
    nbr, p, beta = device_affinities(n, 2, 9)
    for name, scale in C.SCALES.items():
        centres, member = C.grouped_embedding(n, nc, scale, 40 + nc)
        check_gradient(nbr, p, centres, member, ex)


@pytest.mark.parametrize('ex', (1.0, 12.0))
@pytest.mark.parametrize('nc', (1, 2, 3))
@pytest.mark.parametrize('k', C.RING_K)
def test_the_gradient_on_ring_lists_at_196616(k, nc, ex):
    nbr, p = C.ring_lists(C.RING_N, k)
    for name, scale in C.SCALES.items():
        centres, member = C.grouped_embedding(C.RING_N, nc, scale, 50 + nc)
        check_gradient(nbr, p, centres, member, ex)


def test_two_gradient_calls_give_the_same_bytes_at_24583():
    n = 24583
    nbr, p, beta = device_affinities(n, 2, 9)
    centres, member = C.grouped_embedding(n, 2, C.SCALES['wide'], 60)
    y = np.ascontiguousarray(centres[member])
    one, two = manifold.gradient(nbr, p, y, 12.0), manifold.gradient(nbr, p, y, 12.0)
    assert one[0].tobytes() == two[0].tobytes() and one[1:] == two[1:]


def test_the_descent_is_rounds_of_the_gradient_and_the_update_at_12297():
    n, nc = 12297, 2
    x = C.affinity_points(n, 2)
    nbr, p, beta = device_affinities(n, 2, 9)
    rng = np.random.default_rng(60)
    y0 = manifold.start(x, nc)
    up0, ga0 = 1e-5 * rng.standard_normal((n, nc)), np.abs(rng.standard_normal((n, nc))) * 0.05 + 0.005
    y, up, ga = y0.copy(), up0.copy(), ga0.copy()
    trace = manifold.descend(nbr, p, y, up, ga, 4, 12.0, 0.5, 200.0)
    ry, rup, rga, rtrace = y0.copy(), up0.copy(), ga0.copy(), np.empty((4, 3))
    for s in range(4):
        g, kl, z = manifold.gradient(nbr, p, ry, 12.0)
        rtrace[s] = kl, z, device_norm(g)
        tsne_ref.update_step(ry, rup, rga, g, 0.5, 200.0)
    for a, b in ((y, ry), (up, rup), (ga, rga), (trace, rtrace)):
        assert a.tobytes() == b.tobytes()
    assert not (y == y0).all() and (rga == 0.01).any() and (rga > ga0).any()       # the floor and the growing branch were taken
