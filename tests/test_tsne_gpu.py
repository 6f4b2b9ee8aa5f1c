"""The manifold stage on the GPU (include/nm_tsne.h): nm_tsne_affinities, nm_tsne_gradient and nm_tsne_descend against
tests/tsne_ref.py: the neighbours entry for entry at ragged sizes around the tile and the row block, on exact data with ties at the
k-th distance and on a permutation; beta and p by properties that do not depend on the path of the search; the gradient, kl and Z
within the header's bounds on the device's own lists and on hand-made ones; the descent bit for bit against rounds of the gradient;
three blobs end to end; and pca's projections through manifold, cluster -em mfy and reweight."""
import functools
import os
import re

import numpy as np
import pytest

import tsne_ref as R
from cluster_ref import d2_matrix
from neuralmelting_amd import _lib as B
from neuralmelting_amd import cluster, manifold, reweight

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
T, ROWS = 128, 512          # csrc/nm_tsne.h: the columns of a tile, the rows of a workgroup (pinned below)
G = 2.0 ** -8               # the grid of the exact data


def test_the_tile_is_what_the_cases_assume():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'neuralmelting_amd', 'csrc', 'nm_tsne.h')).read()
    const = {k: v for k, v in re.findall(r'constexpr int (TS_\w+) = ([^;]+);', src)}
    assert int(const['TS_TILE']) == T and int(const['TS_BLOCK']) == 256 and int(const['TS_RPT']) == 2 and const['TS_ROWS'] == 'TS_RPT * TS_BLOCK'
    assert ROWS == 2 * 256 and int(const['TS_STEPS']) == R.STEPS and int(const['TS_MAXK']) == 4096
    assert '#pragma clang fp contract(off)' in src


def blobs(n, nd, seed, k=3):
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-3.0, 3.0, (k, nd))
    x = centre[rng.integers(0, k, n)] + 0.4 * rng.standard_normal((n, nd))
    return x[rng.permutation(n)]


def order_of(x):
    """of every row all other points by (d2, index), and the sorted distances: (N, N - 1) each"""
    d2 = d2_matrix(x)
    n = d2.shape[0]
    order = np.stack([(lambda o: o[o != i])(np.lexsort((np.arange(n), d2[i]))) for i in range(n)])
    return order, np.take_along_axis(d2, order, axis=1)


def affinities_raw(x, px, k):
    L = B.load()
    x = np.ascontiguousarray(x, dtype=np.float64)
    n, nd = x.shape
    nbr, p, beta = np.full((n, k), -77, np.int32), np.full((n, k), -77.0), np.full(n, -77.0)
    rc = L.nm_tsne_affinities(0, n, nd, x.ctypes.data_as(B.c_double_p), px, k, nbr.ctypes.data_as(B.c_int32_p), p.ctypes.data_as(B.c_double_p),
                              beta.ctypes.data_as(B.c_double_p))
    return rc, (L.nm_tsne_last_error().decode() if rc else ''), (nbr, p, beta)


# ---- the neighbours
KS = (1, 2, 63, 64, 65, -1)         # -1: N - 1


@pytest.mark.parametrize('nd', (1, 2, 16))
@pytest.mark.parametrize('n', (2, 3, T - 1, T, T + 1, 2 * T + 3, ROWS - 1, ROWS + 1, 2 * ROWS + T + 7))
def test_neighbours_at_ragged_sizes(n, nd):
    """Every k of the list that the size admits.  The header admits no perplexity at k = 1 (the interval (1, k) is empty), so k = 1,
    and with it N = 2, is the refusal."""
    x = blobs(n, nd, 100 * nd + n)
    order, _ = order_of(x)
    ks = sorted({n - 1 if k < 0 else k for k in KS} & set(range(1, n)))
    assert ks and ks[-1] == n - 1
    for k in ks:
        rc, msg, (nbr, p, beta) = affinities_raw(x, 1.5, k)
        if k == 1:
            assert rc == B.NM_ERR_ARG and 'perplexity' in msg and (nbr == -77).all()
            continue
        assert rc == B.NM_OK, msg
        np.testing.assert_array_equal(nbr, order[:, :k])
        assert np.isfinite(beta).all() and (beta > 0).all() and np.abs(p.sum(axis=1) - 1.0).max() <= (-(-k // 256) + 32) * U


def grid_points(n, nd, seed):
    """blobs rounded to a coarse grid, a third of them copies of others: every d2 is exact, duplicates and ties abound"""
    rng = np.random.default_rng(seed)
    x = np.round(blobs(n, nd, seed) / (16 * G)) * (16 * G)
    x[rng.permutation(n)[: n // 3]] = x[rng.integers(0, n, n // 3)]
    return x


@pytest.mark.parametrize('n,nd,k', ((2 * T + 3, 2, 7), (ROWS + 1, 1, 64), (2 * ROWS + T + 7, 3, 65), (T + 1, 16, 5)))
def test_neighbours_on_exact_data_with_ties_at_the_kth_distance(n, nd, k):
    x = grid_points(n, nd, 7 * n + nd)
    order, dist = order_of(x)
    assert len(np.unique(x, axis=0)) < n                                    # duplicated points
    tied = dist[:, k - 1] == dist[:, k]                                     # the k-th and the one behind it at one distance: the index decides
    assert tied.sum() >= (3 if nd == 16 else n // 8), tied.sum()
    rc, msg, (nbr, p, beta) = affinities_raw(x, 1.5, k)
    assert rc == B.NM_OK, msg
    np.testing.assert_array_equal(nbr, order[:, :k])


def test_neighbours_of_a_permutation():
    x = blobs(2 * T + 3, 3, 5)
    k = 20
    perm = np.random.default_rng(6).permutation(x.shape[0])
    rc, msg, (nbr, p, beta) = affinities_raw(x, 6.0, k)
    rc2, msg2, (nbr2, p2, beta2) = affinities_raw(x[perm], 6.0, k)
    assert rc == rc2 == B.NM_OK
    np.testing.assert_array_equal(nbr2, order_of(x[perm])[0][:, :k])
    np.testing.assert_array_equal(perm[nbr2], nbr[perm])                    # off ties the lists are the same points
    np.testing.assert_array_equal(beta2, beta[perm])                        # and the rows the same numbers in the same order
    np.testing.assert_array_equal(p2, p[perm])


# ---- beta and p
K0, STARS = 64, 2


@functools.lru_cache(maxsize=None)
def starred():
    """259 blob points in 8 dimensions and, far off, STARS groups of a centre and K0 copies of one point at distance 1 from it: the
    centre's K0 distances are all equal, and a copy sees K0 - 1 copies at distance 0"""
    x = blobs(2 * T + 3, 8, 11)
    extra = []
    for s in range(STARS):
        c = np.zeros(8)
        c[s] = 100.0
        q = c.copy()
        q[7] += 1.0
        extra += [c] + [q] * K0
    x = np.concatenate([x, np.array(extra)])
    x = x[np.random.default_rng(12).permutation(x.shape[0])]
    order, dist = order_of(x)
    for a in (x, order, dist):
        a.setflags(write=False)
    return x, order, dist


@pytest.mark.parametrize('px', (1.5, 5.0, 30.0, K0 - 0.5))
def test_beta_and_p_by_their_properties(px):
    x, order, dist = starred()
    n, k = x.shape[0], K0
    rc, msg, (nbr, p, beta) = affinities_raw(x, px, k)
    assert rc == B.NM_OK, msg
    np.testing.assert_array_equal(nbr, order[:, :k])
    d = dist[:, :k]
    t = d - d[:, :1]
    bnd = (int(np.ceil(k / 256)) + 32)                                       # the header's B
    assert np.isfinite(beta).all() and (beta > 0).all()
    assert np.abs(p.sum(axis=1) - 1.0).max() <= bnd * U
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        a = beta[:, None] * t
        e = np.exp(-a)
        s = e.sum(axis=1, keepdims=True)
        want = e / s
        assert (np.abs(p - want) <= 2 * (bnd + np.where(np.isfinite(a), a, 0.0)) * U * want + 1e-300).all()
        # a row has a root iff fewer of its entries lie at dmin than the perplexity asks for
        ties = (t == 0.0).sum(axis=1)
        noroot = ties >= px
        assert noroot.sum() == STARS + (STARS * K0 if px <= K0 - 1 else 0)  # the centres, and the copies while K0 - 1 zeros are too many
        for i in np.nonzero(noroot)[0]:
            assert beta[i] == 2.0 ** 200
            np.testing.assert_array_equal(p[i], np.where(t[i] == 0.0, 1.0 / ties[i], 0.0))
        worst = 0.0
        for i in np.nonzero(~noroot)[0]:
            h = R.entropy(t[i], beta[i])[0]
            m2 = float((a[i] ** 2 * want[i]).sum())
            hb = bnd * U * (1.0 + np.log(k) + m2)
            assert abs(h - np.log(px)) <= hb, (i, h - np.log(px), hb)
            bref = R.search(t[i], np.log(px))
            pr = R.entropy(t[i], bref)[1]
            slope = bref * float((pr * t[i] ** 2).sum() - (pr * t[i]).sum() ** 2)                # |H'| = beta Var_p(t)
            assert abs(beta[i] - bref) <= 2 * hb / slope, (i, beta[i], bref, hb, slope)
            worst = max(worst, abs(h - np.log(px)) / hb)
        print('px %g: largest |H - ln px| %.3g of its bound' % (px, worst))


def test_a_value_that_is_not_finite_is_refused():
    x = np.array(starred()[0])
    x[T + 5, 3] = np.nan
    x[-1, 0] = np.inf
    rc, msg, out = affinities_raw(x, 5.0, 20)
    assert rc == B.NM_ERR_ARG and msg.startswith('nm_tsne_affinities:') and msg.endswith('point %d' % (T + 5)), msg
    assert all((o == -77).all() for o in out)


# ---- the gradient
def embeddings(n, nc, seed):
    """the scale of the start, a spread of O(10), and that spread with a tenth of the points on top of others (w = 1)"""
    rng = np.random.default_rng(seed)
    wide = 10.0 * rng.standard_normal((n, nc))
    coincident = wide.copy()
    coincident[rng.permutation(n)[: n // 10]] = coincident[rng.integers(0, n, n // 10)]
    return {'start': 1e-4 * rng.standard_normal((n, nc)), 'wide': wide, 'coincident': coincident}


def check_gradient(nbr, p, y, ex):
    n, k = nbr.shape
    grad, kl, z = manifold.gradient(nbr, p, y, ex)
    rg, rkl, rz, mag, klmag = R.gradient(nbr, p, y, ex)
    c = (3 * n + k + 64) * U
    err = np.abs(grad - rg)
    assert (err <= c * mag).all(), (err / (c * mag + 1e-300)).max()
    assert abs(z - rz) <= 2 * (n + 64) * U * rz, (z, rz)
    assert abs(kl - rkl) <= c * klmag, (kl, rkl, klmag)
    return (err / (c * mag + 1e-300)).max()


def random_p(n, k, seed):
    p = np.random.default_rng(seed).random((n, k)) + 0.01
    return p / p.sum(axis=1, keepdims=True)


def hand_made(kind):
    n = T + 2
    i = np.arange(n)
    if kind == 'hub':                               # point 0 in every list: in-degree N - 1
        nbr = np.empty((n, 3), dtype=np.int64)
        nbr[0] = [1, 2, 3]
        for r in range(1, n):                       # a row's entries are distinct and not the row
            cand = [c for c in range(1, n) if c != r]
            nbr[r] = [0, cand[(r * 7) % len(cand)], cand[(r * 7 + 1) % len(cand)]]
    elif kind == 'orphan':                          # the last point in nobody's list
        nbr = np.stack([(i + 1) % (n - 1), (i + 3) % (n - 1)], axis=1)
        nbr[n - 1] = [0, 1]
    elif kind == 'mutual':                          # pairs that list each other and nobody else
        nbr = (i ^ 1)[:, None]
    else:                                           # k = 1, a ring
        nbr = ((i + 1) % n)[:, None]
    nbr = np.ascontiguousarray(nbr, dtype=np.int32)
    assert (nbr != i[:, None]).all() and all(len(set(r)) == len(r) for r in nbr.tolist())
    return nbr, random_p(n, nbr.shape[1], 3)


@pytest.mark.parametrize('ex', (1.0, 24.0))
@pytest.mark.parametrize('nc', (1, 2, 3))
@pytest.mark.parametrize('kind', ('hub', 'orphan', 'mutual', 'ring'))
def test_the_gradient_on_hand_made_lists(kind, nc, ex):
    nbr, p = hand_made(kind)
    n = nbr.shape[0]
    if kind == 'hub':
        assert (nbr == 0).sum() == n - 1
    if kind == 'orphan':
        assert not (nbr == n - 1).any()
    for name, y in embeddings(n, nc, 20 + nc).items():
        check_gradient(nbr, p, y, ex)


@functools.lru_cache(maxsize=None)
def own_lists():
    """the device's own affinities of 2 ROWS + T + 7 points: three row blocks, ten tiles, several column slices"""
    x = blobs(2 * ROWS + T + 7, 4, 31)
    nbr, p, beta = manifold.affinities(x, 20.0, 61)
    for a in (x, nbr, p):
        a.setflags(write=False)
    return x, nbr, p


@pytest.mark.parametrize('ex', (1.0, 24.0))
@pytest.mark.parametrize('nc', (1, 2, 3))
def test_the_gradient_on_the_device_s_own_affinities(nc, ex):
    x, nbr, p = own_lists()
    for name, y in embeddings(x.shape[0], nc, 40 + nc).items():
        worst = check_gradient(nbr, p, y, ex)
        print('%s, ncomp %d, exaggeration %g: largest error %.3g of the bound' % (name, nc, ex, worst))


def test_two_calls_give_the_same_bytes():
    x, nbr, p = own_lists()
    y = embeddings(x.shape[0], 2, 50)['wide']
    one, two = manifold.gradient(nbr, p, y, 12.0), manifold.gradient(nbr, p, y, 12.0)
    assert one[0].tobytes() == two[0].tobytes() and one[1:] == two[1:]
    ms = np.full(5, -1.0)
    assert B.load().nm_tsne_last_timing(ms.ctypes.data_as(B.c_double_p)) == B.NM_OK
    assert (ms >= 0.0).all() and ms[1] > 0.0 and ms[2] > 0.0 and ms[3] > 0.0
    a, b = affinities_raw(x, 20.0, 61), affinities_raw(x, 20.0, 61)
    for u, v in zip(a[2], b[2]):
        assert u.tobytes() == v.tobytes()
    np.testing.assert_array_equal(a[2][0], nbr)


# ---- the descent
def tree(v):
    """the sum of 256 values in the order of the kernels' workgroup tree"""
    v = np.array(v, dtype=np.float64)
    h = 128
    while h:
        v[:h] = v[:h] + v[h:2 * h]
        h //= 2
    return v[0]


def device_norm(g):
    """sqrt(sum g^2) in the kernels' order: blocks of 256 elements by the tree, the blocks' sums one thread each (256 apart, in sequence), the tree"""
    sq = np.zeros(-(-g.size // 256) * 256)
    sq[:g.size] = (g * g).ravel()
    blocks = [tree(b) for b in sq.reshape(-1, 256)]
    lanes = np.zeros(256)
    for b, v in enumerate(blocks):
        lanes[b % 256] = lanes[b % 256] + v
    return np.sqrt(tree(lanes))


@pytest.mark.parametrize('nc', (2, 3))
def test_the_descent_is_rounds_of_the_gradient_and_the_update(nc):
    x, nbr, p = own_lists()
    n = x.shape[0]
    rng = np.random.default_rng(60)
    y0 = manifold.start(x, nc)
    up0, ga0 = 1e-5 * rng.standard_normal((n, nc)), np.abs(rng.standard_normal((n, nc))) * 0.05 + 0.005
    y, up, ga = y0.copy(), up0.copy(), ga0.copy()
    trace = np.concatenate([manifold.descend(nbr, p, y, up, ga, 4, 12.0, 0.5, 200.0), manifold.descend(nbr, p, y, up, ga, 3, 1.0, 0.8, 200.0)])
    ry, rup, rga, rtrace = y0.copy(), up0.copy(), ga0.copy(), np.empty((7, 3))
    floored = grown = shrunk = False
    for s in range(7):
        ex, mom = (12.0, 0.5) if s < 4 else (1.0, 0.8)
        g, kl, z = manifold.gradient(nbr, p, ry, ex)
        rtrace[s] = kl, z, device_norm(g)
        before = rga.copy()
        R.update_step(ry, rup, rga, g, mom, 200.0)
        floored, grown, shrunk = floored or (rga == 0.01).any(), grown or (rga > before).any(), shrunk or (rga == before * 0.8).any()
    assert floored and grown and shrunk                                     # the floor and both branches were taken
    for a, b in ((y, ry), (up, rup), (ga, rga), (trace, rtrace)):
        assert a.tobytes() == b.tobytes()
    assert not (y == y0).any()


def test_one_step_against_the_restatement():
    """the gradient's bound through the update: |dy| <= rate gains |dg| and a few roundings of the update's own terms"""
    x, nbr, p = own_lists()
    n, k = nbr.shape
    rng = np.random.default_rng(61)
    y0 = rng.standard_normal((n, 2))
    up0, ga0 = 0.1 * rng.standard_normal((n, 2)), np.ones((n, 2))
    rg, rkl, rz, mag, klmag = R.gradient(nbr, p, y0, 4.0)
    dg = (3 * n + k + 64) * U * mag
    assert (np.abs(rg) > dg).all()                                          # no sign of update * g hangs on a rounding
    y, up, ga = y0.copy(), up0.copy(), ga0.copy()
    trace = manifold.descend(nbr, p, y, up, ga, 1, 4.0, 0.8, 200.0)
    ry, rup, rga = y0.copy(), up0.copy(), ga0.copy()
    R.update_step(ry, rup, rga, rg, 0.8, 200.0)
    np.testing.assert_array_equal(ga, rga)
    bound = 200.0 * rga * dg + 4 * U * (np.abs(0.8 * up0) + np.abs(200.0 * rg * rga) + np.abs(y0))
    assert (np.abs(up - rup) <= bound).all() and (np.abs(y - ry) <= bound).all()
    assert abs(trace[0, 0] - rkl) <= (3 * n + k + 64) * U * klmag and abs(trace[0, 1] - rz) <= 2 * (n + 64) * U * rz
    assert abs(trace[0, 2] - np.sqrt((rg * rg).sum())) <= 1e-12 * trace[0, 2]


# ---- end to end
def purity(y, blob):
    d2 = d2_matrix(y)
    np.fill_diagonal(d2, np.inf)
    return float((blob[d2.argmin(axis=1)] == blob).mean())


def test_three_blobs_end_to_end():
    rng = np.random.default_rng(70)
    blob = np.repeat(np.arange(3), 60)
    x = np.array([[6.0, 0, 0, 0], [-6.0, 0, 0, 0], [0, 6.0, 0, 0]])[blob] + 0.5 * rng.standard_normal((180, 4))
    k = manifold.neighbours(180, 15.0)
    rnbr, rp, rbeta, _ = R.affinities(x, 15.0, k)
    ry = manifold.start(x, 2)
    rup, rga = np.zeros_like(ry), np.ones_like(ry)
    R.descend(rnbr, rp, ry, rup, rga, 100, 12.0, 0.5, 200.0)
    rtrace = R.descend(rnbr, rp, ry, rup, rga, 200, 1.0, 0.8, 200.0)
    assert purity(ry, blob) == 1.0 and rtrace[-1, 0] < rtrace[0, 0], 'the restatement'
    nbr, p, beta = manifold.affinities(x, 15.0, k)
    np.testing.assert_array_equal(nbr, rnbr)
    y = manifold.start(x, 2)
    up, ga = np.zeros_like(y), np.ones_like(y)
    manifold.descend(nbr, p, y, up, ga, 100, 12.0, 0.5, 200.0)
    trace = manifold.descend(nbr, p, y, up, ga, 200, 1.0, 0.8, 200.0)
    print('kl %.6g -> %.6g (the restatement: %.6g -> %.6g)' % (trace[0, 0], trace[-1, 0], rtrace[0, 0], rtrace[-1, 0]))
    assert purity(y, blob) == 1.0
    assert trace[-1, 0] < trace[0, 0]


# ---- the stage
PN, TN, SN, LD, NATOMS = 2, 4, 100, 3, 32
HOT_SHARE = (0.0, 0.25, 0.75, 1.0)


def two_phase_grid(tmp_path):
    """test_cluster_gpu.py's grid: a cold blob at pc0 = -1 and a hot one at +1, the two columns in the middle mixed"""
    rng = np.random.default_rng(41)
    temp = np.linspace(1, 2, TN, dtype=np.float32)
    hot = np.stack([np.stack([rng.permutation(SN) < round(share * SN) for share in HOT_SHARE]) for _ in range(PN)])
    z = 0.15 * rng.standard_normal((PN, TN, SN, LD))
    z[..., 0] += np.where(hot, 1.0, -1.0)
    pe = -5.0 * NATOMS + 1.5 * NATOMS * temp[None, :, None] + 0.5 * NATOMS * hot + np.sqrt(1.5 * NATOMS) * temp[None, :, None] * rng.normal(size=hot.shape)
    vol = NATOMS * (1.0 + 0.1 * temp[None, :, None]) + rng.normal(size=hot.shape)
    prefix = str(tmp_path / 'mf.lj.fcc.lammps')
    np.save(prefix + '.virial.trgt.npy', np.linspace(1, 2, PN, dtype=np.float32))
    np.save(prefix + '.temp.trgt.npy', temp)
    np.save(prefix + '.pe.npy', pe.astype(np.float32))
    np.save(prefix + '.vol.npy', vol.astype(np.float32))
    np.save(prefix + '.natoms.npy', np.full(hot.shape, NATOMS, dtype=np.uint16))
    np.save(prefix + '.cdf.pcz.npy', z)
    return prefix, temp, hot


def test_the_stage_end_to_end(tmp_path, monkeypatch, capsys):
    prefix, temp, hot = two_phase_grid(tmp_path)
    monkeypatch.chdir(tmp_path)
    args = ['-n', 'mf', '-px', '30', '-ni', '300', '-xi', '100', '-ex', '12']
    assert manifold.main(['-v'] + args) == 0
    assert 'embedding 800 of 800 samples' in capsys.readouterr().out
    first = {key: open(prefix + '.cdf.%s.npy' % key, 'rb').read() for key in ('mfy', 'mfb', 'mft')}
    mfy, mfb, mft = (np.load(prefix + '.cdf.%s.npy' % key) for key in ('mfy', 'mfb', 'mft'))
    assert mfy.shape == hot.shape + (2,) and mfb.shape == hot.shape and mft.shape == (300, 3) and mfy.dtype == mfb.dtype == mft.dtype == np.float64
    assert np.isfinite(mfy).all() and (mfb > 0).all() and np.isfinite(mft).all() and mft[-1, 0] < mft[100, 0]
    assert manifold.main(args) == 0                                         # a second run writes the same bytes
    for key, data in first.items():
        assert open(prefix + '.cdf.%s.npy' % key, 'rb').read() == data, key
    # the embedding keeps the two phases apart: DBSCAN finds two clusters, cold first
    assert cluster.main(['-v', '-n', 'mf', '-em', 'mfy', '-nc', '0.1', '-ms', '5']) == 0
    assert '2 clusters' in capsys.readouterr().out
    cll, cls, cl0, cl1 = (np.load(prefix + '.cdf.%s.npy' % key) for key in ('cll', 'cls', 'cl0', 'cl1'))
    noise = cll < 0
    assert noise.mean() < 0.02 and cls.shape == (2, 5)
    # cl0 is the cold phase and cl1 the hot one.  t-SNE is no isometry: the exaggerated steps may strand a sample in the other
    # phase's island, so a sample in a hundred may sit on the wrong side (the noise's allowance above is two)
    assert ((cl0 + cl1) == ~noise).all() and (cl0 * cl1 == 0).all()
    assert (cl1 != (hot & ~noise)).mean() <= 0.01 and (cl0 != (~hot & ~noise)).mean() <= 0.01
    assert reweight.main(['-n', 'mf', '-e', 'LJ', '-tg', '33', '-ob', 'cdf.cl1', '-hq', 'cdf.cl1', '-hx', '0.5']) == 0
    rwe = np.load(prefix + '.rwe.npy')
    assert rwe.shape == (PN,) and ((temp[1] < rwe) & (rwe < temp[2])).all()
    frac = cl1.mean(axis=(0, 2))                                            # the liquid fraction rises with T
    assert (np.diff(frac) > 0).all() and frac[0] < 0.02 and frac[-1] > 0.9


def test_samples_left_out_of_the_embedding(tmp_path, monkeypatch):
    prefix, temp, hot = two_phase_grid(tmp_path)
    monkeypatch.chdir(tmp_path)
    assert manifold.main(['-n', 'mf', '-sk', '10', '-sd', '3', '-ni', '200', '-xi', '80', '-ex', '12']) == 0       # the perplexity: the 30 kept samples
    mfy, mfb = np.load(prefix + '.cdf.mfy.npy'), np.load(prefix + '.cdf.mfb.npy')
    out = np.ones(SN, dtype=bool)
    out[10::3] = False
    assert np.isnan(mfy[:, :, out]).all() and np.isnan(mfb[:, :, out]).all() and np.isfinite(mfy[:, :, ~out]).all() and np.isfinite(mfb[:, :, ~out]).all()
    assert cluster.main(['-n', 'mf', '-em', 'mfy', '-nc', '0.15', '-ms', '4', '-sk', '10', '-sd', '3']) == 0
    cll, cl0, cl1 = (np.load(prefix + '.cdf.%s.npy' % key) for key in ('cll', 'cl0', 'cl1'))
    assert (cll[:, :, out] == -1).all() and (cl0[:, :, out] == 0).all() and (cl1[:, :, out] == 0).all()
    assert (cll[:, :, ~out] >= 0).mean() > 0.95 and cl0[:, :, ~out].sum() > 0 and cl1[:, :, ~out].sum() > 0
    with pytest.raises(SystemExit, match='are not those'):
        cluster.main(['-n', 'mf', '-em', 'mfy', '-nc', '0.1', '-sk', '10', '-sd', '2'])


def test_cluster_em_pcz_writes_the_files_of_no_flag(tmp_path, monkeypatch):
    prefix, temp, hot = two_phase_grid(tmp_path)
    monkeypatch.chdir(tmp_path)
    keys = ('cll', 'cld', 'cls', 'cl0', 'cl1')
    assert cluster.main(['-n', 'mf', '-nc', '0.1']) == 0
    plain = {key: open(prefix + '.cdf.%s.npy' % key, 'rb').read() for key in keys}
    for key in keys:
        os.remove(prefix + '.cdf.%s.npy' % key)
    assert cluster.main(['-n', 'mf', '-nc', '0.1', '-em', 'pcz']) == 0
    for key in keys:
        assert open(prefix + '.cdf.%s.npy' % key, 'rb').read() == plain[key], key
