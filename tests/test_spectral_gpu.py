"""Spectral clustering on the GPU (include/nm_distr.h: nm_cluster_spectral): nm_cluster_spectral on sentinel-filled outputs against the dense
reference of tests/spectral_ref.py on ragged sizes around every edge of the pass's shape, in 1, 2, 3 and 16 dimensions and at every
padded width; the stops; a size at which a workgroup walks several tiles; tiny, duplicated, isolated and non-finite input; two calls;
and neuralmelting_amd.cluster -cl spectral end to end on a synthetic grid whose embedding is two rings."""
import os
import re

import numpy as np
import pytest

import spectral_cases as K
import spectral_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import cluster

pytestmark = pytest.mark.gpu

U = R.U
TOL = 1e-8
BIG = 24 * K.ROWS + K.TILE + 7                      # 12423 points: 25 row blocks, 98 tiles, 82 slices


def test_the_shape_is_what_the_cases_assume():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'neuralmelting_amd', 'csrc', 'nm_spectral.h')).read()
    const = {k: v for k, v in re.findall(r'constexpr int (SP_\w+) = ([^;]+);', src)}
    assert int(const['SP_BLOCK']) == 256 and int(const['SP_RPT']) == 2 and const['SP_ROWS'] == 'SP_RPT * SP_BLOCK' and K.ROWS == 2 * 256
    assert (int(const['SP_TILE']), int(const['SP_GRID']), int(const['SP_SPAN'])) == (K.TILE, K.GRID, K.SPAN)
    assert int(const['SP_CHUNK']) == 4096
    assert 'ScanShape<SP_BLOCK, SP_RPT, SP_TILE, SP_GRID, SP_SPAN>' in src
    # the grids of the sizes below: more than one slice; a workgroup that walks several tiles; the limit's partial sums below 2 GiB
    assert K.scan_grid(K.TILE + 1) == (1, 2) and K.scan_grid(K.SIZES[-1]) == (3, 10)
    blocks, slices = K.scan_grid(BIG)
    assert (blocks, slices) == (25, 82) and (BIG + K.TILE - 1) // K.TILE == 98 > slices
    assert K.scan_grid(2 ** 20)[1] * 2 ** 20 * 16 * 8 < 2 ** 31


def dense_checks(x, nd, ncomp, nblock, ref, out, converged=True):
    """what every successful call must satisfy against the dense reference; the figures are printed before they are asserted.  The
    c-th Ritz value is near the c-th eigenvalue only where the call converged: a call stopped early has its true residuals all the same"""
    n = x.shape[0]
    embed, eigval, resid, deg = out['embed'], out['eigval'], out['resid'], out['deg']
    assert np.isfinite(embed).all() and np.isfinite(eigval).all() and np.isfinite(resid).all() and (resid >= 0.0).all()
    assert (np.diff(eigval) <= 0.0).all()
    off = np.abs(deg - ref.deg).astype(np.float64) / R.deg_bound(ref, n, nd)
    eps_r = R.eps_r(ref, n, nd, nblock)
    true, v, block = R.residuals(ref, embed, deg, eigval)
    ortho = np.abs(v.T @ v - np.eye(ncomp)).max()
    print('n %d nd %d %d/%d: deg off by %.3g of its bound; eps_R %.3g; resid %s, recomputed off by %.3g; eigval off by %s; orthonormal to %.3g' % (
        n, nd, ncomp, nblock, off.max(), eps_r, resid[:ncomp], np.abs(true - resid[:ncomp]).max(), np.abs(eigval[:ncomp] - ref.lam[:ncomp]), ortho))
    assert off.max() <= 1.0
    assert eps_r < 1e-10
    assert (np.abs(true - resid[:ncomp]) <= eps_r).all()
    assert not converged or (np.abs(eigval[:ncomp] - ref.lam[:ncomp]) <= resid[:ncomp] + 2 * eps_r).all()
    assert ortho <= 1e-12
    for c in range(ncomp):                                                  # the sign rule
        assert embed[np.argmax(np.abs(embed[:, c])), c] > 0.0
    return block, v


CASES = ([(n, 2, nc, nb) for n in K.SIZES for nc, nb in K.WIDTHS if nb <= n]
         + [(n, nd, nc, nb) for nd in (1, 3, 16) for n in (K.TILE + 1, K.SIZES[-1]) for nc, nb in K.WIDTHS])


@pytest.mark.parametrize('n,nd,ncomp,nblock', CASES)
def test_ragged_sizes_dimensions_and_widths(n, nd, ncomp, nblock):
    x, gamma, truth, ref = K.case(n, nd, ncomp)
    rc, msg, out = K.raw(x, gamma, ncomp, K.start(n, nblock), tol=TOL)
    assert rc == B.NM_OK, msg
    passes, status = out['info']
    block, v = dense_checks(x, nd, ncomp, nblock, ref, out)
    assert status == 0 and passes >= 1 and out['resid'][:ncomp].max() <= TOL
    if ncomp < n:
        # The sine of the largest angle of a returned vector to the reference's eigenspace is at most max resid / gap: the part y of
        # v_c outside that space obeys (M - theta_c) y = the residual's part outside it, and theta_c is at least gap above the rest of
        # the spectrum (Davis and Kahan for one vector).  The residual is the returned one within the header's eps_R, and the
        # reference's eigenvectors are eigh's, exact for a matrix within 4 N u of M.  For the two spaces the theorem wants the 2-norm
        # of the block of residuals, which lies between the largest residual and sqrt(ncomp) times it.
        gap = ref.lam[ncomp - 1] - ref.lam[ncomp]
        slack = R.eps_r(ref, n, nd, nblock) + 4 * n * U
        sines, bound = R.sines(v, ref.vec[:, :ncomp]), (out['resid'][:ncomp].max() + slack) / gap
        spaces, wide = R.sine(v, ref.vec[:, :ncomp]), (block + slack) / gap
        print('gap %.4g, sines %s, bound %.3g; between the spaces %.3g, bound %.3g; %d passes' % (gap, sines, bound, spaces, wide, passes))
        assert gap > 0.0 and sines.max() <= bound and spaces <= wide
    if ncomp == 3 and nd > 1 and n >= K.TILE - 1:                          # the blobs: k-means of the embedding is the truth
        assert gap >= K.BLOBS_GAP and R.labels_agree(R.lloyd(out['embed'], 3, 1), truth)
    if ncomp == 2 and nd > 1:
        assert gap >= K.RINGS_GAP and R.labels_agree(R.lloyd(out['embed'], 2, 1), truth)


def test_where_a_workgroup_walks_several_tiles():
    """12423 points: slices 0 to 15 walk two tiles.  The reference is float64 in blocks of rows, its own error of the size of the
    header's bounds, so the comparisons allow twice those."""
    n, nd, ncomp, nblock = BIG, 2, 3, 8
    x, which = K.blobs(n, 99)
    rc, msg, out = K.raw(x, K.BLOBS_GAMMA, ncomp, K.start(n, nblock), tol=TOL)
    assert rc == B.NM_OK, msg
    assert tuple(out['info'])[1] == 0
    deg, slack, gmax = np.empty(n), np.empty(n), 0.0
    v = out['embed'] * np.sqrt(out['deg'])[:, None]
    rs, mv = 1.0 / np.sqrt(out['deg']), np.empty((n, ncomp))
    for r0 in range(0, n, 1024):
        t = K.BLOBS_GAMMA * ((x[r0:r0 + 1024, None, :] - x[None, :, :]) ** 2).sum(axis=2)
        a = np.exp(-t)
        a[np.arange(a.shape[0]), r0 + np.arange(a.shape[0])] = 0.0
        deg[r0:r0 + 1024], slack[r0:r0 + 1024], gmax = a.sum(axis=1), (t * a).sum(axis=1), max(gmax, float(t.max()))
        mv[r0:r0 + 1024] = rs[r0:r0 + 1024, None] * (a @ (rs[:, None] * v))
    bound = U * ((nd + 3) * slack + (2 * n + 2) * deg)
    eps_r = np.sqrt(nblock) * (2 * (nd + 3) * gmax + 4 * n + 16) * U + 160 * U
    true = np.linalg.norm(mv - v * out['eigval'][None, :ncomp], axis=0)
    print('deg off by %.3g of its bound, eps_R %.3g, resid %s recomputed off by %.3g' % (
        (np.abs(out['deg'] - deg) / bound).max(), eps_r, out['resid'][:ncomp], np.abs(true - out['resid'][:ncomp]).max()))
    assert (np.abs(out['deg'] - deg) <= 2 * bound).all()
    assert eps_r < 1e-10 and (np.abs(true - out['resid'][:ncomp]) <= 2 * eps_r).all()
    assert np.abs(v.T @ v - np.eye(ncomp)).max() <= 1e-12
    assert R.labels_agree(R.lloyd(out['embed'][::16], 3, 1), which[::16])


# ---- the stops
def test_stops():
    n, nd, ncomp, nblock = K.SIZES[-1], 2, 2, 5
    x, gamma, truth, ref = K.case(n, nd, ncomp)
    init = K.start(n, nblock)
    rc, msg, one = K.raw(x, gamma, ncomp, init, max_pass=1, tol=TOL)
    assert rc == B.NM_OK and tuple(one['info']) == (1, 2), msg
    dense_checks(x, nd, ncomp, nblock, ref, one, converged=False)                            # still the true residuals of the returned pairs
    assert one['resid'][:ncomp].max() > 1e-3
    rc, msg, seven = K.raw(x, gamma, ncomp, init, max_pass=8, tol=TOL)      # one pass short of the second round's Rayleigh-Ritz pass
    assert rc == B.NM_OK and tuple(seven['info']) == (1, 2) and seven['embed'].tobytes() == one['embed'].tobytes()
    rc, msg, zero = K.raw(x, gamma, ncomp, init, max_pass=40, tol=0.0)
    assert rc == B.NM_OK and tuple(zero['info']) == (33, 2), (msg, zero['info'])        # 1 + 4 * 8, and 41 would pass max_pass
    dense_checks(x, nd, ncomp, nblock, ref, zero, converged=False)
    assert zero['resid'][:ncomp].max() < one['resid'][:ncomp].max()
    rc, msg, plain = K.raw(x, gamma, ncomp, init, degree=1, max_pass=5, tol=0.0)        # degree 1: every pass a Rayleigh-Ritz pass
    assert rc == B.NM_OK and tuple(plain['info']) == (5, 2)
    dense_checks(x, nd, ncomp, nblock, ref, plain, converged=False)


def test_the_pass_count_on_the_rings():
    x, inner = K.rings(1287, 1)
    ref = R.dense(x, K.RINGS_GAMMA)
    init = K.start(1287, 16)
    rc, msg, out = K.raw(x, K.RINGS_GAMMA, 2, init, degree=8, tol=TOL)
    assert rc == B.NM_OK, msg
    want = R.filtered(ref.m, init, 2, 8, 2000, TOL)[0]
    print('rings of 1287 points, block 16, degree 8: %d passes to %g, the restatement %d' % (out['info'][0], TOL, want))
    assert out['info'][1] == 0 and out['info'][0] < 200
    dense_checks(x, 2, 2, 16, ref, out)
    assert R.labels_agree(R.lloyd(out['embed'], 2, 1), inner)


# ---- tiny, duplicated, isolated and non-finite input
def test_two_points_have_the_eigenvalues_1_and_minus_1():
    x = np.array([[0.0, 0.0], [0.5, 0.0]])
    rc, msg, out = K.raw(x, 2.0, 2, np.array([[1.0, 0.3], [0.2, 1.0]]), tol=TOL)
    assert rc == B.NM_OK, msg
    dense_checks(x, 2, 2, 2, R.dense(x, 2.0), out)                          # the block is the whole space: the first Rayleigh-Ritz pass is exact
    assert np.abs(out['eigval'] - [1.0, -1.0]).max() <= 1e-13 and tuple(out['info']) == (1, 0)
    want = np.exp(-0.5)
    assert np.abs(out['deg'] - want).max() <= 4 * U
    assert np.abs(np.abs(out['embed']) - np.sqrt(0.5 / want)).max() <= 1e-15 and (out['embed'][0] > 0.0).all()
    assert out['embed'][1, 0] > 0.0 > out['embed'][1, 1]


def test_duplicate_points_give_a_finite_result():
    x, gamma, truth, ref = K.case(K.ROWS + 1, 2, 3)
    x = np.array(x)
    x[1::2] = x[:-1:2]                                                      # every point twice, but the last
    rc, msg, out = K.raw(x, gamma, 3, K.start(x.shape[0], 8), tol=TOL)
    assert rc == B.NM_OK and out['info'][1] == 0, msg
    dense_checks(x, 2, 3, 8, R.dense(x, gamma), out)
    assert out['deg'][1::2].tobytes() == out['deg'][:-1:2].tobytes()       # a twin's sum has the same terms in the same places, but for a +0


def test_an_isolated_point_is_refused_with_its_index():
    x = np.array(K.case(K.ROWS + 1, 2, 3)[0])
    x[K.TILE + 5] = [1e3, 0.0]
    rc, msg, out = K.raw(x, 1.0, 3, K.start(x.shape[0], 8), tol=TOL)
    assert rc == B.NM_ERR_ARG and msg.startswith('nm_cluster_spectral:') and 'point %d ' % (K.TILE + 5) in msg and 'gamma is too large' in msg, msg
    assert K.untouched(out)
    x[7] = [-1e3, 0.0]                                                      # the first of two is named
    rc, msg, out = K.raw(x, 1.0, 3, K.start(x.shape[0], 8), tol=TOL)
    assert rc == B.NM_ERR_ARG and 'point 7 ' in msg and K.untouched(out), msg


@pytest.mark.parametrize('bad', (np.nan, np.inf, -np.inf))
def test_a_value_that_is_not_finite_is_refused(bad):
    x = np.array(K.case(K.ROWS + 1, 2, 3)[0])
    x[-1, 1] = bad
    rc, msg, out = K.raw(x, K.BLOBS_GAMMA, 3, K.start(x.shape[0], 8))
    assert rc == B.NM_ERR_ARG and msg.startswith('nm_cluster_spectral:') and msg.endswith('point %d' % (x.shape[0] - 1)), msg
    assert K.untouched(out)
    x[K.TILE + 5, 0] = bad
    rc, msg, out = K.raw(x, K.BLOBS_GAMMA, 3, K.start(x.shape[0], 8))
    assert rc == B.NM_ERR_ARG and msg.endswith('point %d' % (K.TILE + 5)) and K.untouched(out), msg


def test_a_dependent_start_block_is_refused():
    x, gamma, truth, ref = K.case(K.ROWS + 1, 2, 3)
    init = K.start(x.shape[0], 8)
    init[:, 5] = init[:, 1]
    rc, msg, out = K.raw(x, gamma, 3, init)
    assert rc == B.NM_ERR_ARG and msg.startswith('nm_cluster_spectral:') and 'dependent' in msg and K.untouched(out), msg


# ---- determinism
def test_two_calls_give_the_same_bytes():
    n = K.SIZES[-1]
    x, gamma, truth, ref = K.case(n, 16, 8)
    init = K.start(n, 16)
    L = B.load()
    kmeans = np.full(3, -1.0)
    assert L.nm_cluster_kmeans_last_timing(kmeans) == B.NM_OK
    one, two, other = K.raw(x, gamma, 8, init, tol=TOL), K.raw(x, gamma, 8, init, tol=TOL), K.raw(x, gamma, 8, init, tol=TOL, fill=-33)
    assert one[0] == two[0] == other[0] == B.NM_OK
    for name in K.OUTPUTS:
        assert one[2][name].tobytes() == two[2][name].tobytes() == other[2][name].tobytes(), name
    ms, after = np.full(5, -1.0), np.full(3, -1.0)
    assert L.nm_cluster_spectral_last_timing(ms) == B.NM_OK and L.nm_cluster_kmeans_last_timing(after) == B.NM_OK
    assert (ms >= 0.0).all() and ms.sum() > 0.0 and ms[2] > 0.0
    assert after.tobytes() == kmeans.tobytes()                              # the k-means slots are left alone
    embed, eigval, resid, deg, passes, status = cluster.spectral(x, gamma, 8, init, tol=TOL)
    assert embed.tobytes() == one[2]['embed'].tobytes() and (passes, status) == tuple(one[2]['info'])


# ---- end to end
PN, TN, SN, LD, NATOMS = 2, 4, 100, 3, 32


def ring_grid():
    """pcz (PN, TN, SN, LD) whose two leading components are the two rings, the inner ring on the two colder temperatures"""
    x, inner = K.rings(PN * TN * SN, 5)
    z = np.zeros((PN, TN, SN, LD))
    cold = np.zeros((PN, TN, SN), dtype=bool)
    cold[:, :TN // 2] = True
    z[cold, :2], z[~cold, :2] = x[inner], x[~inner]
    z[..., 2] = 20.0 * np.random.default_rng(6).standard_normal((PN, TN, SN))       # a component that -nd 2 leaves out
    return z, cold


def test_the_stage_end_to_end(tmp_path, monkeypatch, capsys):
    z, cold = ring_grid()
    temp = np.linspace(1, 2, TN, dtype=np.float32)
    prefix = str(tmp_path / 'sp.lj.fcc.lammps')
    rng = np.random.default_rng(8)
    np.save(prefix + '.virial.trgt.npy', np.linspace(1, 2, PN, dtype=np.float32))
    np.save(prefix + '.temp.trgt.npy', temp)
    np.save(prefix + '.pe.npy', rng.standard_normal(cold.shape).astype(np.float32))
    np.save(prefix + '.vol.npy', (NATOMS + rng.standard_normal(cold.shape)).astype(np.float32))
    np.save(prefix + '.natoms.npy', np.full(cold.shape, NATOMS, dtype=np.uint16))
    np.save(prefix + '.cdf.pcz.npy', z)
    monkeypatch.chdir(tmp_path)
    # the rings have the radii 1 and 3: in the stage's unit (pc0's range 6, the variances' sum 5 / 36) the tests' gamma 5 is -gm 25
    args = ['-n', 'sp', '-nc', '2', '-sk', '10', '-sd', '2']
    assert cluster.main(['-v', '-cl', 'spectral', '-gm', '25'] + args) == 0
    said = capsys.readouterr().out
    assert 'eigenvalues' in said and 'the gap behind the 2-th' in said and 'passes' in said and 'warning' not in said
    assert not os.path.exists(prefix + '.cdf.cld.npy')
    keys = ('cll', 'cls', 'clr', 'cl0', 'cl1', 'cle', 'clv', 'clg')
    out = {key: np.load(prefix + '.cdf.%s.npy' % key) for key in keys}
    used = np.zeros(SN, dtype=bool)
    used[10::2] = True
    assert out['cll'].shape == cold.shape and out['cll'].dtype == np.int32 and (out['cll'][:, :, ~used] == -1).all()
    assert out['cle'].shape == (16, 2) and out['clv'].shape == cold.shape + (2,) and out['clg'].shape == cold.shape
    assert out['cle'].dtype == out['clv'].dtype == out['clg'].dtype == np.float64
    np.testing.assert_array_equal(np.isnan(out['clg']), np.broadcast_to(~used, cold.shape))
    np.testing.assert_array_equal(np.isnan(out['clv']), np.broadcast_to(~used[:, None], cold.shape + (2,)))
    assert (np.diff(out['cle'][:, 0]) <= 0.0).all() and out['cle'][:2, 1].max() <= 1e-6 and out['cle'][0, 0] == pytest.approx(1.0, abs=1e-9)
    assert out['clg'][:, :, used].min() > 1.0
    # the labels are the rings, cl0 the inner one, which lies on the colder half
    label = out['cll'][:, :, used]
    assert R.labels_agree(label.ravel(), cold[:, :, used].ravel())
    np.testing.assert_array_equal(out['cl0'], (cold & used).astype(np.float64))
    np.testing.assert_array_equal(out['cl1'], (~cold & used).astype(np.float64))
    assert out['cls'].shape == (2, 5) and out['cls'][:, 0].sum() == PN * TN * used.sum() and out['clr'].shape == (10, 3)
    assert np.abs(out['cls'][:, 3:]).max() < 0.2                            # the centroid is in the projections: both rings' is the origin
    first = {key: open(prefix + '.cdf.%s.npy' % key, 'rb').read() for key in keys}
    assert cluster.main(['-cl', 'spectral', '-gm', '25'] + args) == 0
    assert all(open(prefix + '.cdf.%s.npy' % key, 'rb').read() == first[key] for key in keys)
    # centroids cannot cut the rings
    assert cluster.main(['-cl', 'kmeans'] + args) == 0
    straight = np.load(prefix + '.cdf.cll.npy')[:, :, used]
    assert not R.labels_agree(straight.ravel(), cold[:, :, used].ravel())
    wrong = ((straight == straight[0, 0, 0]) != (cold[:, :, used] == cold[0, 0, 0])).mean()
    assert 0.25 < wrong < 0.75
