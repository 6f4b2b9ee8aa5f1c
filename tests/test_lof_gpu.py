"""The outlier stage on the GPU (include/nm_distr.h: nm_distr_lof) on sentinel-filled outputs against tests/lof_ref.py: ragged
sizes around the tile and the rows of a workgroup (the reduced ones above k = 16 and k = 32 among them), sets that would see each
other through any leak, duplicates and ties, a relabelling, two calls, values that are not finite; and neuralmelting_amd.outlier end to
end on a synthetic grid with planted outliers, through manifold -il, cluster -il and reweight's loader."""
import functools
import os
import re

import numpy as np
import pytest

import lof_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import cluster, manifold, outlier, reweight

pytestmark = pytest.mark.gpu

SENT = -77.0
T, ROWS, KFULL = 128, 256, 16           # csrc/nm_lof.h: the columns of a tile, the rows of a workgroup up to k = KFULL (pinned below)


def rows(k):
    """the rows of a workgroup of the neighbour pass: halved above KFULL and again above twice KFULL"""
    return ROWS >> (k > KFULL) >> (k > 2 * KFULL)


def test_the_tile_is_what_the_cases_assume():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'neuralmelting_amd', 'csrc', 'nm_lof.h')).read()
    const = {k: v for k, v in re.findall(r'constexpr int (LOF_\w+) = ([^;]+);', src)}
    assert int(const['LOF_TILE']) == T and int(const['LOF_ROWS']) == ROWS and int(const['LOF_KFULL']) == KFULL and int(const['LOF_MAXK']) == 64
    assert 'return k <= LOF_KFULL ? LOF_ROWS : k <= 2 * LOF_KFULL ? LOF_ROWS / 2 : LOF_ROWS / 4;' in src
    assert [rows(k) for k in (1, 16, 17, 32, 33, 64)] == [256, 256, 128, 128, 64, 64]


def raw(x, k, neighbours=True):
    """the raw ABI on sentinel-filled outputs: rc, message, (lof, lrd, kdist, nbr)"""
    L = B.load()
    x = np.ascontiguousarray(x, dtype=np.float64)
    nsets, npts, nd = x.shape
    out = [np.full((nsets, npts), SENT) for _ in range(3)] + [np.full((nsets, npts, k), int(SENT), np.int32)]
    rc = L.nm_distr_lof(0, nsets, npts, nd, x, k, out[0], out[1], out[2], out[3] if neighbours else None)
    return rc, (L.nm_distr_last_error().decode() if rc else ''), out


def check(x, k, ref=None):
    """the device's results, after they have been found to be the restatement's: the lists identical, kdist, lrd and lof within
    twice the header's bounds (the restatement carries them as the device does)"""
    rc, msg, (lof, lrd, kdist, nbr) = raw(x, k)
    assert rc == B.NM_OK, msg
    rl, rr, rk, rn = ref or R.batch(x, k)
    np.testing.assert_array_equal(nbr, rn)
    for name, got, want, bound in zip(('lof', 'lrd', 'kdist'), (lof, lrd, kdist), (rl, rr, rk), R.bounds(x.shape[2], k)):
        err = np.abs(got - want)
        assert (err <= 2.0 * bound * np.abs(want)).all(), (name, float((err / np.maximum(np.abs(want), 1e-300)).max()) / R.U, bound / R.U)
    return lof, lrd, kdist, nbr


def blobs(nsets, npts, nd, seed):
    """two blobs and a scattered tenth per set, every set its own draw"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nsets, npts, nd)) * 0.5 + 3.0 * rng.integers(0, 2, (nsets, npts, 1))
    x[:, : npts // 10] = rng.uniform(-6.0, 6.0, (nsets, npts // 10, nd))
    return x


# ---- ragged sizes: every size for every k, the other two parameters taking turns; 4096 points with two sets only
def cases():
    out = []
    for a, k in enumerate((1, 5, 20, 64)):
        r = rows(k)
        for b, npts in enumerate((2, 3, k + 1, k + 2, T - 1, T, T + 1, r - 1, r + 1, 2 * r + T + 7, 4096)):
            if npts == 4096 and k not in (20, 64):
                continue
            nd = (1, 2, 3, 8, 16)[(a + b) % 5] if npts < 4096 else (3 if k == 20 else 2)
            case = (2 if npts == 4096 else (1, 2, 37)[(a + 2 * b) % 3], npts, nd, min(k, npts - 1))
            if case not in out:
                out.append(case)
    return out


def test_the_cases_hold_every_value():
    cs = cases()
    assert {c[0] for c in cs} == {1, 2, 37} and {c[2] for c in cs} == {1, 2, 3, 8, 16} and {1, 5, 20, 64} <= {c[3] for c in cs}
    for k in (1, 5, 20, 64):
        r = rows(k)
        assert {2, 3, k + 1, k + 2, T - 1, T, T + 1, r - 1, r + 1, 2 * r + T + 7} <= {c[1] for c in cs if c[3] == min(k, c[1] - 1)}
    assert {c[0] for c in cs if c[1] == 4096} == {2} and {c[3] for c in cs if c[1] == 4096} == {20, 64}


@pytest.mark.parametrize('nsets,npts,nd,k', cases())
def test_ragged_sizes(nsets, npts, nd, k):
    x = blobs(nsets, npts, nd, 1000 * k + npts + nd)
    lof, lrd, kdist, nbr = check(x, k)
    assert np.isfinite(lof).all() and (lrd > 0.0).all() and (kdist > 0.0).all()
    if npts >= 100:
        assert (lof > 1.5).any() and (lof < 1.5).sum() > npts // 2              # the case holds outliers and inliers


# ---- sets do not see each other
def test_a_batch_is_its_sets_one_by_one():
    """set s + 1 is set s moved by a thousandth of the spacing of its points: a column read across a set's end, in either direction,
    is far nearer to a row than anything of the row's own set and would enter its list"""
    nsets, npts, nd, k = 37, rows(20) + T // 2 + 3, 3, 20
    base = np.random.default_rng(12).uniform(-1.0, 1.0, (npts, nd))
    x = base[None] + 1e-4 * np.arange(nsets)[:, None, None]
    dd = R.d2(base) + 4.0 * np.eye(npts)
    assert dd.min() > 1e3 * (1e-4 * np.sqrt(nd)) ** 2                             # the next set's copy is the nearer one by far
    rc, msg, whole = raw(x, k)
    assert rc == B.NM_OK, msg
    for s in range(nsets):
        rc, msg, one = raw(x[s:s + 1], k)
        assert rc == B.NM_OK, msg
        for a, b in zip(whole, one):
            assert a[s].tobytes() == b[0].tobytes(), s
    check(x[-2:], k)


# ---- duplicates and ties
def test_a_coincident_set_among_others():
    x = blobs(3, 70, 2, 5)
    x[1] = 0.375
    lof, lrd, kdist, nbr = check(x, 20)
    assert (kdist[1] == 0.0).all() and (lrd[1] == 1e10).all() and (lof[1] == 1.0).all()
    np.testing.assert_array_equal(nbr[1, 0], np.arange(1, 21))
    np.testing.assert_array_equal(nbr[1, 69], np.arange(0, 20))
    np.testing.assert_array_equal(nbr[1, 7], np.delete(np.arange(21), 7))


@pytest.mark.parametrize('k', (5, 20, 64))
def test_copies_are_listed_in_index_order(k):
    rng = np.random.default_rng(k)
    npts = rows(k) + k + 9
    x = rng.standard_normal((2, npts, 3))
    same = np.sort(rng.permutation(npts)[: k + 5])
    x[1, same] = x[1, same[0]]
    lof, lrd, kdist, nbr = check(x, k)
    for i in same:
        np.testing.assert_array_equal(nbr[1, i], same[same != i][:k])
    assert (kdist[1, same] == 0.0).all() and (lrd[1, same] == 1e10).all() and (lof[1, same] == 1.0).all()


def test_an_integer_lattice():
    """5^3 lattice points at shuffled indices, twice over (every point has a copy), and a 19 x 19 square: d2 takes few values, every
    list is decided by the index again and again"""
    rng = np.random.default_rng(6)
    cube = np.stack(np.meshgrid(*[np.arange(5.0)] * 3, indexing='ij'), axis=-1).reshape(-1, 3)
    x = np.stack([np.concatenate([cube, cube])[rng.permutation(250)] for _ in range(3)])
    for k in (1, 20, 64):
        lof, lrd, kdist, nbr = check(x, k)
        dd = R.d2(x[2])
        for i in range(250):                                                      # the lexicographic order, stated once more
            keys = list(zip(dd[i, nbr[2, i]].tolist(), nbr[2, i].tolist()))
            rest = np.setdiff1d(np.arange(250), np.append(nbr[2, i], i))
            assert keys == sorted(keys) and keys[-1] < min(zip(dd[i, rest].tolist(), rest.tolist()))
    square = np.stack(np.meshgrid(np.arange(19.0), np.arange(19.0), indexing='ij'), axis=-1).reshape(1, -1, 2)[:, rng.permutation(361)]
    check(square, 20)


# ---- relabelling and determinism
@functools.lru_cache(maxsize=None)
def generic():
    x = blobs(2, 2 * rows(20) + T + 7, 8, 77)
    x.setflags(write=False)
    return x, R.batch(x, 20)


def test_a_permutation_of_the_points_permutes_the_result():
    x, ref = generic()
    lof, lrd, kdist, nbr = check(x, 20, ref)
    p = np.random.default_rng(9).permutation(x.shape[1])
    pl, pr, pk, pn = check(x[:, p], 20)
    np.testing.assert_array_equal(pk, kdist[:, p])                                # off ties: the same lists, the same sums in the same order
    np.testing.assert_array_equal(pr, lrd[:, p])
    np.testing.assert_array_equal(pl, lof[:, p])
    np.testing.assert_array_equal(p[pn], nbr[:, p])


def test_two_calls_give_the_same_bytes_with_and_without_the_lists():
    x, ref = generic()
    one, two, bare = raw(x, 20), raw(x, 20), raw(x, 20, neighbours=False)
    assert one[0] == two[0] == bare[0] == B.NM_OK
    for a, b in zip(one[2], two[2]):
        assert a.tobytes() == b.tobytes()
    for a, b in zip(one[2][:3], bare[2][:3]):
        assert a.tobytes() == b.tobytes()
    assert (bare[2][3] == int(SENT)).all()                                        # the array that was not handed over
    ms = np.full(5, -1.0)
    assert B.load().nm_distr_last_timing(ms) == B.NM_OK
    assert (ms[:4] >= 0.0).all() and ms[1] > 0.0 and ms[4] == -1.0                # four slots
    got = outlier.lof(x, 20, neighbours=True)
    for a, b in zip(one[2], got):
        assert a.tobytes() == b.tobytes()
    assert len(outlier.lof(x, 20)) == 3


# ---- a value that is not finite
@pytest.mark.parametrize('bad', (np.nan, np.inf, -np.inf))
def test_a_value_that_is_not_finite_is_refused(bad):
    x = np.array(generic()[0])
    npts = x.shape[1]
    x[1, npts - 1, 7] = bad
    rc, msg, out = raw(x, 20)
    assert rc == B.NM_ERR_ARG and msg.startswith('nm_distr_lof:') and msg.endswith('set 1, point %d' % (npts - 1)), msg
    assert all((o == SENT).all() for o in out)
    x[0, T + 5, 0] = bad                                                          # the first of two is named
    rc, msg, out = raw(x, 20)
    assert rc == B.NM_ERR_ARG and msg.endswith('set 0, point %d' % (T + 5)) and all((o == SENT).all() for o in out), msg


# ---- end to end
PN, TN, SN, LD, SK, SD = 2, 3, 96, 4, 8, 2


def planted_grid():
    """pcz: every grid point a blob, uniform in a cube of side 2 about a centre of its own, with three of its kept samples moved 25
    along an axis each; planted (PN, TN, SN) says which"""
    rng = np.random.default_rng(41)
    z = rng.uniform(-1.0, 1.0, (PN, TN, SN, LD)) + rng.uniform(-3.0, 3.0, (PN, TN, 1, LD))
    planted = np.zeros((PN, TN, SN), dtype=bool)
    for p in range(PN):
        for t in range(TN):
            idx = SK + SD * rng.permutation(len(range(SK, SN, SD)))[:3]
            planted[p, t, idx] = True
            z[p, t, idx] += 25.0 * np.eye(LD)[rng.permutation(LD)[:3]] * rng.choice([-1.0, 1.0], (3, 1))
    return z, planted


def test_the_stage_end_to_end(tmp_path, monkeypatch, capsys):
    z, planted = planted_grid()
    prefix = str(tmp_path / 'lo.lj.fcc.lammps')
    np.save(prefix + '.virial.trgt.npy', np.linspace(1, 2, PN, dtype=np.float32))
    np.save(prefix + '.temp.trgt.npy', np.linspace(1, 2, TN, dtype=np.float32))
    np.save(prefix + '.pe.npy', np.random.default_rng(2).random((PN, TN, SN)).astype(np.float32))
    np.save(prefix + '.cdf.pcz.npy', z)
    monkeypatch.chdir(tmp_path)
    flags = ['-n', 'lo', '-sk', str(SK), '-sd', str(SD)]
    assert outlier.main(['-v'] + flags) == 0
    said = capsys.readouterr().out
    assert '6 sets of 44 of 96 samples of cdf in 4 components, 20 neighbours' in said and '18 of 264 samples' in said and 'the most, 3 of 44' in said
    out = {key: np.load(prefix + '.cdf.%s.npy' % key) for key in ('lof', 'lod', 'loi', 'lon')}
    assert all(out[key].shape == (PN, TN, SN) and out[key].dtype == np.float64 for key in ('lof', 'lod', 'loi'))
    assert out['lon'].shape == (PN, TN) and out['lon'].dtype == np.int32 and (out['lon'] == 3).all()
    left_out = np.ones(SN, dtype=bool)
    left_out[SK::SD] = False
    for key in ('lof', 'lod'):
        np.testing.assert_array_equal(np.isnan(out[key]), np.broadcast_to(left_out, (PN, TN, SN)))
    assert (out['loi'][:, :, left_out] == 0.0).all()
    # the planted samples are the outliers, and the decision is the restatement's
    np.testing.assert_array_equal(out['loi'][:, :, SK::SD], (~planted[:, :, SK::SD]).astype(np.float64))
    rl, rr, rk, rn = R.batch(z[:, :, SK::SD].reshape(PN * TN, -1, LD), 20)
    assert np.abs(rl - 1.5).min() > 0.1
    np.testing.assert_array_equal(out['loi'][:, :, SK::SD].reshape(PN * TN, -1), (rl <= 1.5).astype(np.float64))
    bound_lof, bound_lrd, _ = R.bounds(LD, 20)
    assert (np.abs(out['lof'][:, :, SK::SD].reshape(PN * TN, -1) - rl) <= 2.0 * bound_lof * rl).all()
    assert (np.abs(out['lod'][:, :, SK::SD].reshape(PN * TN, -1) - rr) <= 2.0 * bound_lrd * rr).all()
    np.testing.assert_array_equal(reweight.load_observables(prefix, ['cdf.loi'], (PN, TN, SN))[0], out['loi'])
    # manifold -il embeds the inliers only
    gone = np.broadcast_to(left_out, (PN, TN, SN)) | planted
    assert manifold.main(flags + ['-il', '-ni', '20', '-xi', '10']) == 0
    mfy, mfb = np.load(prefix + '.cdf.mfy.npy'), np.load(prefix + '.cdf.mfb.npy')
    assert mfy.shape == (PN, TN, SN, 2) and mfb.shape == (PN, TN, SN)
    np.testing.assert_array_equal(np.isnan(mfy), np.broadcast_to(gone[..., None], mfy.shape))
    np.testing.assert_array_equal(np.isnan(mfb), gone)
    # cluster -il takes that file, and refuses it without -il; it works on pcz as well
    assert cluster.main(flags + ['-il', '-em', 'mfy', '-nc', '0.2', '-ms', '3']) == 0
    cll, cld = np.load(prefix + '.cdf.cll.npy'), np.load(prefix + '.cdf.cld.npy')
    assert (cll[gone] == -1).all() and (cld[gone] == 0).all() and (cld[~gone] >= 1).all() and (cll[~gone] >= 0).any()
    with pytest.raises(SystemExit, match=r'cluster: -sk 8 -sd 2 are not those that .*cdf\.mfy\.npy was written with'):
        cluster.main(flags + ['-em', 'mfy', '-nc', '0.2'])
    assert cluster.main(flags + ['-il', '-nc', '0.15', '-ms', '3', '-nd', '4']) == 0
    cll, cld = np.load(prefix + '.cdf.cll.npy'), np.load(prefix + '.cdf.cld.npy')
    assert (cll[gone] == -1).all() and (cld[gone] == 0).all() and (cld[~gone] >= 1).all() and (cll[~gone] >= 0).any()
    assert cluster.main(flags + ['-nc', '0.15', '-ms', '3', '-nd', '4']) == 0      # without -il the planted samples are clustered too
    assert (np.load(prefix + '.cdf.cld.npy')[planted] >= 1).all()
    # a mask of another -sk is refused by both
    for main, more in ((manifold.main, ['-ni', '2', '-xi', '1']), (cluster.main, ['-nc', '0.05'])):
        with pytest.raises(SystemExit, match=r'-sk 10 -sd 2 are not those that .*cdf\.lof\.npy was written with'):
            main(['-n', 'lo', '-sk', '10', '-sd', '2', '-il'] + more)
