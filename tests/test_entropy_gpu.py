"""nm_distr_entropy (include/nm_distr.h) on the GPU: the pair entropy per atom s, its neighbour average sbar, the entry counts, the
means and the count below a cut through the C-ABI against the long-double restatement tests/entropy_ref.py.  Every call runs on
sentinel-filled outputs and is checked for: nnb and nlow equal exactly, every output written completely, s, sbar and the means within
the derived bound of the public header (entropy_ref.bounds, taken once, not doubled), and that bound below 1e-9 (1 + |s|).  The cut
of nlow is the midpoint of the largest gap of the restatement's sorted sbar, a gap above 1e-6, so that no atom is near it.

Covered: random liquids of 1 to 500 atoms (on both sides of the block of 32 centres, of the wave and of 256) at a first-shell r_m and
at half the box; every instantiation of the grid (nbins 1, 63, 64, 65, 128, 256, 512, 1024) and the blocks of grid points a small
sigma skips; the closed form without entries; perfect fcc; a sigma that leaves grid points with h_k == 0; crystal below random frame;
every neighbour in two images; r_m and r_avg exactly on a float32 distance; coincident atoms; mixed boxes; an unwrapped frame; two
launch chunks; 4095 atoms; a permutation; determinism; every combination of NULL outputs; nm_distr_bondorder untouched; the refusals;
the command line."""
import itertools
import os

import numpy as np
import pytest

import entropy_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import distr, reweight

pytestmark = pytest.mark.gpu

SENT = -7.25e300
ISENT = -77777777
NAMES = ('s', 'sbar', 'nnb', 'smean', 'sbarmean', 'nlow')
INTS = ('nnb', 'nlow')
NAN, INF = float('nan'), float('inf')


def call(pos, box, r_m, sigma, nbins, r_avg, s_cut=-INF, want=NAMES, device=0, ns=None, natoms=None, null=()):
    """the raw ABI on sentinel-filled outputs, NULL for the outputs not in `want`; returns (rc, message, dict of the six arrays)"""
    L = B.load()
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    box = np.ascontiguousarray(box, dtype=np.float32).reshape(-1)
    m, n = pos.shape[0], pos.shape[1]
    out = dict(s=np.full((m, n), SENT), sbar=np.full((m, n), SENT), nnb=np.full((m, n), ISENT, dtype=np.int32), smean=np.full(m, SENT),
               sbarmean=np.full(m, SENT), nlow=np.full(m, ISENT, dtype=np.int32))
    ptr = {k: (out[k].ctypes.data_as(B.c_int32_p if k in INTS else B.c_double_p) if k in want and k not in null else None) for k in NAMES}
    rc = L.nm_distr_entropy(device, m if ns is None else ns, n if natoms is None else natoms,
                            None if 'pos' in null else pos.ctypes.data_as(B.c_float_p), None if 'box' in null else box.ctypes.data_as(B.c_float_p),
                            float(r_m), float(sigma), int(nbins), float(r_avg), float(s_cut), *[ptr[k] for k in NAMES])
    return rc, (L.nm_distr_last_error().decode() if rc else ''), out


def untouched(out):
    return all((out[k] == (ISENT if k in INTS else SENT)).all() for k in NAMES)


def run(pos, box, r_m, sigma, nbins, r_avg, s_cut=-INF):
    rc, msg, out = call(pos, box, r_m, sigma, nbins, r_avg, s_cut)
    assert rc == 0, msg
    for k in NAMES:
        assert (out[k] != (ISENT if k in INTS else SENT)).all(), k + ' is not written completely'
    return out


def gap_cut(sbar):
    """the midpoint of the largest gap of the sorted values and the gap; where all values are one (a single atom, equal samples: no gap
    above 1e-6) the cut lies 1 above them and the gap is infinite"""
    v = np.sort(np.asarray(sbar, dtype=np.float64).reshape(-1))
    g = np.diff(v)
    if len(g) == 0 or g.max() <= 1e-6:
        return float(v[-1]) + 1.0, INF
    k = int(np.argmax(g))
    return 0.5 * (v[k] + v[k + 1]), float(g[k])


def compare(out, ref, label):
    """the six outputs against the restatement within the derived bounds"""
    np.testing.assert_array_equal(out['nnb'], ref['nnb'])
    sabs = np.abs(ref['s']).astype(np.float64)
    assert (ref['e_s'] < 1e-9 * (1 + sabs)).all(), 'the derived bound is too large: the derivation is wrong'
    for k, tol in (('s', ref['e_s']), ('sbar', ref['e_sbar'][:, None]), ('smean', ref['e_smean']), ('sbarmean', ref['e_sbarmean'])):
        err = np.abs(out[k].astype(R.LD) - ref[k]).astype(np.float64)
        tol = np.broadcast_to(tol, err.shape)
        print('%s %s: max |error| %.3g, bound there %.3g, largest error / bound %.3g (%d entries at most, %d within r_avg)'
              % (label, k, err.max(), tol.reshape(-1)[int(np.argmax(err))], (err / tol).max(), ref['nnb'].max(), ref['navg'].max()))
        assert (err <= tol).all(), k
    np.testing.assert_array_equal(out['nlow'], ref['nlow'])


def check(pos, box, r_m, sigma, nbins, r_avg, label=''):
    """the six outputs against the restatement, the cut of nlow in the largest gap of sbar; returns (outputs, restatement)"""
    pos = np.asarray(pos, dtype=np.float32)
    box = np.asarray(box, dtype=np.float32).reshape(-1)
    ref = R.entropy(pos, box, r_m, sigma, nbins, r_avg)
    cut, gap = gap_cut(ref['sbar'])
    assert gap > 1e-6
    ref['nlow'] = (ref['sbar'] < R.LD(cut)).sum(axis=1).astype(np.int32)
    out = run(pos, box, r_m, sigma, nbins, r_avg, cut)
    compare(out, ref, label or 'n %d nbins %d' % (pos.shape[1], nbins))
    assert 0 < out['nlow'].sum() < pos.shape[0] * pos.shape[1] or gap == INF
    return out, ref


def liquid(rng, ns, n, rho=0.9, spread=0.0):
    box = ((n / rho) ** (1 / 3) * (1.0 + spread * rng.random(ns))).astype(np.float32)
    pos = (rng.random((ns, n, 3)) * box[:, None, None]).astype(np.float32)
    return pos, box


def fcc_integer(cells):
    """fcc with a0 = 2 on integer coordinates: exact in float32; box 2 * cells"""
    base = np.array([[0, 0, 0], [0, 1, 1], [1, 0, 1], [1, 1, 0]])
    g = np.arange(cells) * 2
    pos = (np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 1, 3) + base).reshape(-1, 3)
    return pos.astype(np.float32), np.float32(2 * cells)


# ---- random liquids
@pytest.mark.parametrize('shell', ('first', 'half'))
@pytest.mark.parametrize('n', (1, 2, 13, 63, 64, 65, 257, 500))
def test_liquid(n, shell):
    rng = np.random.default_rng(9000 + n)
    pos, box = liquid(rng, 2 if n <= 257 else 1, n)
    l = float(box.min())
    r_m = min(1.5, 0.5 * l) if shell == 'first' else 0.5 * l
    out, ref = check(pos, box, r_m, 0.12, 64, min(1.5, 0.5 * l))
    if n == 1:
        assert not out['nnb'].any() and out['sbar'].tobytes() == out['s'].tobytes() == out['smean'].tobytes() == out['sbarmean'].tobytes()
    if n >= 257 and shell == 'half':
        assert ref['nnb'].min() > 64


@pytest.mark.parametrize('nbins', (1, 63, 64, 65, 128, 256, 512, 1024))
def test_grid_sizes(nbins):
    """65 atoms at half the box: one to seventeen grid points per lane, the last block of them partly beyond nbins"""
    rng = np.random.default_rng(9100)
    pos, box = liquid(rng, 2, 65)
    l = float(box.min())
    check(pos, box, 0.5 * l, 0.1, nbins, 0.3 * l)


@pytest.mark.parametrize('nbins', (128, 1024))
def test_narrow_gaussians_skip_blocks_of_grid_points(nbins):
    """sigma = r_m / 200: an entry reaches 10 sigma = r_m / 20 to either side, less than a block of 64 grid points at 1024 intervals,
    so most blocks are skipped for most entries"""
    rng = np.random.default_rng(9150)
    pos, box = liquid(rng, 1, 100)
    l = float(box.min())
    check(pos, box, 0.5 * l, 0.5 * l / 200, nbins, 0.25 * l)


def test_largest_atom_count():
    """4095 atoms, a first-shell r_m: nnb against nm_distr_bondorder's, s of centres on both sides of the blocks of 32 against the
    restatement of single centres"""
    rng = np.random.default_rng(9200)
    n = 4095
    pos, box = liquid(rng, 1, n)
    r_m, sigma, nbins = 1.5, 0.12, 32
    out = run(pos, box, r_m, sigma, nbins, 1.2)
    L = B.load()
    ls = np.array([6], dtype=np.int32)
    nnb = np.zeros((1, n), dtype=np.int32)
    rc = L.nm_distr_bondorder(0, 1, n, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), 0.0, r_m, 1,
                              ls.ctypes.data_as(B.c_int_p), None, None, None, nnb.ctypes.data_as(B.c_int32_p))
    assert rc == 0
    np.testing.assert_array_equal(out['nnb'], nnb)
    M = int(nnb.max())
    for c in (0, 31, 32, 2047, 4064, 4094):
        s, A, h, rho, m = R.local(pos[0], box[0], c, r_m, sigma, nbins)
        b = R.bounds(np.array([[A]]), h[None, None], np.array([rho]), R.grid(r_m, nbins)[1], R.grid(r_m, nbins)[0], sigma, nbins, M, 0,
                     np.array([[s]]))
        err = float(abs(R.LD(out['s'][0, c]) - s))
        print('4095 atoms, centre %d: |error| %.3g, bound %.3g' % (c, err, b['e_s'][0, 0]))
        assert m == nnb[0, c] and err <= b['e_s'][0, 0] < 1e-9 * (1 + abs(float(s)))


# ---- known answers
def test_no_entries_closed_form():
    """one atom; and a dilute frame on a coarse integer grid whose nearest distance is 2 > r_m"""
    for nbins in (1, 7, 64):
        out, ref = check(np.full((1, 1, 3), 0.25), [3.0], 1.5, 0.1, nbins, 1.5, 'one atom, nbins %d' % nbins)
        want = R.no_entries(1, 3.0, 1.5, nbins)
        assert abs(R.LD(out['s'][0, 0]) - want) <= ref['e_s'][0, 0] + 4 * R.U * abs(float(want))
    rng = np.random.default_rng(9300)
    g = rng.permutation(125)[:40]
    pos = (2.0 * np.stack([g // 25, (g // 5) % 5, g % 5], axis=-1)).astype(np.float32)[None]
    rc, msg, out = call(pos, [10.0], 1.9, 0.05, 50, 4.0)
    assert rc == 0, msg
    ref = R.entropy(pos, [10.0], 1.9, 0.05, 50, 4.0)
    compare(out, ref, 'dilute frame')
    assert not out['nnb'].any() and ref['navg'].min() > 0
    want = R.no_entries(40, 10.0, 1.9, 50)
    assert (np.abs(out['s'].astype(R.LD) - want) <= ref['e_s'] + 4 * R.U * abs(float(want))).all()
    assert len(set(out['s'].reshape(-1).tolist())) == 1


def test_perfect_fcc_has_one_value():
    p, box = fcc_integer(4)
    pos = p[None]
    ref = R.entropy(pos, [box], 4.0, 0.15, 128, 1.7)
    out = run(pos, [box], 4.0, 0.15, 128, 1.7, -1e30)
    compare(out, ref, 'perfect fcc')
    assert (out['nnb'] == out['nnb'][0, 0]).all() and out['nnb'][0, 0] > 128 and (ref['navg'] == 12).all()
    spread = out['s'].max() - out['s'].min()
    print('perfect fcc: s %.15g, spread over the 256 atoms %.3g, bound %.3g' % (out['s'][0, 0], spread, ref['e_s'].max()))
    assert spread <= 2 * ref['e_s'].max() and np.abs(out['sbar'] - out['s']).max() <= 2 * ref['e_sbar'][0]
    assert (out['nlow'] == 0).all()


def test_sigma_so_small_that_grid_points_hold_nothing():
    """a0 = 2 fcc, sigma = 0.01, D = 0.01: the shells sit at sqrt 2, 2, sqrt 6, sqrt 8, and every grid point further than 0.1 from all of
    them gets no term at all (h_k == 0, I_k = r_k^2), where the restatement holds 24 terms below exp(-50) times the prefactor"""
    p, box = fcc_integer(3)
    pos = p[None]
    ref = R.entropy(pos, [box], 3.0, 0.01, 300, 1.7)
    _, rk = R.grid(3.0, 300)
    shells = np.sqrt(np.array([2.0, 4.0, 6.0, 8.0]))
    empty = (np.abs(rk[:, None] - shells[None, :]) > 0.1 + 1e-9).all(axis=1)
    assert 200 < empty.sum() < 300
    h, rho = R.local(pos[0], box, 0, 3.0, 0.01, 300)[2:4]
    assert (h[empty] < 24 * np.exp(R.LD(-50.0)) / (4 * R.PI * rho * R.LD(0.01) * np.sqrt(2 * R.PI))).all() and (h[~empty] > 0).all()
    out = run(pos, [box], 3.0, 0.01, 300, 1.7, -1e30)
    compare(out, ref, 'narrow sigma')
    assert out['s'].max() < -5.0


def test_crystal_below_random_frame():
    """256 atoms at the density of the a0 = 2 lattice, the command line's automatic parameters: the mean sbar of the 4^3 fcc crystal with
    Gaussian noise of 3 % of the neighbour distance lies below that of uniform random atoms, in the restatement and in the kernel"""
    rng = np.random.default_rng(9400)
    p, box = fcc_integer(4)
    solid = ((p + 0.03 * np.sqrt(2.0) * rng.normal(size=p.shape)) % box).astype(np.float32)
    gas = (rng.random(p.shape) * box).astype(np.float32)
    rm, sigma, nbins, ravg = distr.entropy_params(distr.parse_args(['-le']), 256)
    l = float(box)
    out, ref = check(np.stack([solid, gas]), [box, box], rm * l, sigma * l, nbins, ravg * l, 'crystal and gas')
    for name, d in (('restatement', ref), ('kernel', out)):
        print('%s: mean sbar %.4f (crystal) against %.4f (random)' % (name, d['sbarmean'][0], d['sbarmean'][1]))
        assert d['sbarmean'][0] < d['sbarmean'][1] and d['smean'][0] < d['smean'][1]


# ---- edges
def test_every_neighbour_in_two_images():
    """two atoms half a box apart along x, r_m = box / 2: the other atom is an entry in two images"""
    pos = np.array([[[0.5, 1.0, 1.0], [2.5, 1.0, 1.0]]], dtype=np.float32)
    out, ref = check(pos, [4.0], 2.0, 0.2, 40, 2.0, 'two images')
    assert (out['nnb'] == 2).all() and (ref['navg'] == 2).all()


def test_radii_exactly_on_a_float32_distance():
    """a0 = 2 fcc with ten vacancies (s varies): the second neighbours sit at d = 2 exactly, inside r_m = 2 and r_avg = 2, outside the
    next smaller doubles"""
    rng = np.random.default_rng(9500)
    p, box = fcc_integer(3)
    pos = p[np.sort(rng.permutation(108)[:98])][None]
    below = np.nextafter(2.0, 0.0)
    on, ron = check(pos, [box], 2.0, 0.2, 40, 2.0, 'radii on a distance')
    off, roff = check(pos, [box], below, 0.2, 40, below, 'radii below it')
    assert (on['nnb'] > off['nnb']).all() and (ron['navg'] > roff['navg']).all()
    mixed, rmix = check(pos, [box], 2.0, 0.2, 40, below, 'r_avg below it')
    assert mixed['s'].tobytes() == on['s'].tobytes() and np.abs(mixed['sbar'] - on['sbar']).max() > 1e-6


def test_coincident_atoms():
    """every atom has a twin at d = 0, which is no entry; the twins share their entries and their values"""
    rng = np.random.default_rng(9600)
    pos, box = liquid(rng, 2, 120)
    pos[:, 1::2] = pos[:, 0::2]
    l = float(box.min())
    out, ref = check(pos, box, 0.5 * l, 0.12, 64, 0.3 * l, 'coincident atoms')
    assert np.array_equal(out['nnb'][:, 0::2], out['nnb'][:, 1::2]) and (out['nnb'] % 2 == 0).all()
    assert np.abs(out['s'][:, 0::2] - out['s'][:, 1::2]).max() <= 2 * ref['e_s'].max()


def test_boxes_that_differ_inside_one_batch():
    rng = np.random.default_rng(9700)
    pos, box = liquid(rng, 4, 120, spread=0.5)
    l = float(box.min())
    out, ref = check(pos, box, 0.5 * l, 0.12, 64, 0.3 * l, 'mixed boxes')
    assert len({a.tobytes() for a in out['smean']}) == 4
    one = run(pos[3:], box[3:], 0.5 * l, 0.12, 64, 0.3 * l)                   # rho is the sample's own
    assert one['s'].tobytes() == out['s'][3:].tobytes() and one['sbarmean'].tobytes() == out['sbarmean'][3:].tobytes()


def test_unwrapped_frame():
    rng = np.random.default_rng(9800)
    pos, box = liquid(rng, 3, 130)
    l = float(box.min())
    wrapped = run(pos, box, 0.3 * l, 0.12, 64, 0.3 * l)
    pos[0] -= box[0]
    pos[1] += (rng.integers(-1, 2, pos[1].shape) * box[1]).astype(np.float32)
    pos[2] += (rng.integers(-3, 4, pos[2].shape) * box[2]).astype(np.float32)   # beyond the 27 images: fewer entries
    out, ref = check(pos, box, 0.3 * l, 0.12, 64, 0.3 * l, 'unwrapped')
    assert out['nnb'][2].sum() < wrapped['nnb'][2].sum()


def test_more_samples_than_one_launch_chunk():
    """4096 + 1 samples of 5 atoms: two launches, the second with one sample.  The samples on both sides of the seam equal, bit for
    bit, a call of their own, which passes the restatement"""
    rng = np.random.default_rng(9900)
    pos, box = liquid(rng, 4097, 5, rho=0.8, spread=0.3)
    l = float(box.min())
    pos[4096, 1] = pos[4096, 0] + np.float32(0.25)                            # the last sample has a pair within r_m, whatever its box
    pick = [0, 4094, 4095, 4096]
    out, ref = check(pos[pick], box[pick], 0.5 * l, 0.1, 32, 0.5 * l, 'seam')
    cut, _ = gap_cut(ref['sbar'])
    big = run(pos, box, 0.5 * l, 0.1, 32, 0.5 * l, cut)
    for k in NAMES:
        assert big[k][pick].tobytes() == out[k].tobytes(), k
    assert big['nnb'][4096].sum() > 0


def test_permutation_of_the_atoms():
    rng = np.random.default_rng(10000)
    pos, box = liquid(rng, 2, 200)
    l = float(box.min())
    one, ref = check(pos, box, 0.4 * l, 0.12, 64, 0.25 * l, 'permutation')
    p = rng.permutation(200)
    cut, _ = gap_cut(ref['sbar'])
    two = run(pos[:, p], box, 0.4 * l, 0.12, 64, 0.25 * l, cut)
    np.testing.assert_array_equal(two['nnb'], one['nnb'][:, p])
    np.testing.assert_array_equal(two['nlow'], one['nlow'])
    assert (np.abs(two['s'] - one['s'][:, p]) <= 2 * ref['e_s'][:, p]).all()
    assert (np.abs(two['sbar'] - one['sbar'][:, p]) <= 2 * ref['e_sbar'][:, None]).all()
    assert (np.abs(two['smean'] - one['smean']) <= 2 * ref['e_smean']).all()
    assert (np.abs(two['sbarmean'] - one['sbarmean']) <= 2 * ref['e_sbarmean']).all()


# ---- determinism and isolation
def test_two_calls_are_equal_bit_for_bit():
    rng = np.random.default_rng(10100)
    pos, box = liquid(rng, 6, 300)
    l = float(box.min())
    a = run(pos, box, 0.5 * l, 0.12, 200, 0.3 * l, -2.0)
    b = run(pos, box, 0.5 * l, 0.12, 200, 0.3 * l, -2.0)
    for k in NAMES:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert 0 < a['nlow'].sum() < 1800


def test_null_outputs():
    """each of the 62 proper subsets of the outputs: what is asked for equals the all-outputs call bit for bit, the rest is untouched"""
    rng = np.random.default_rng(10200)
    pos, box = liquid(rng, 3, 60)
    l = float(box.min())
    full, ref = check(pos, box, 0.5 * l, 0.12, 64, 0.3 * l, 'all outputs')
    cut, _ = gap_cut(ref['sbar'])
    for r in range(1, 6):
        for want in itertools.combinations(NAMES, r):
            rc, msg, out = call(pos, box, 0.5 * l, 0.12, 64, 0.3 * l, cut, want=want)
            assert rc == 0, msg
            for x in NAMES:
                if x in want:
                    assert out[x].tobytes() == full[x].tobytes(), (want, x)
                else:
                    assert (out[x] == (ISENT if x in INTS else SENT)).all(), (want, x)


def test_bondorder_is_the_same_before_and_after():
    rng = np.random.default_rng(10300)
    pos, box = liquid(rng, 3, 150)
    l = float(box.min())
    L = B.load()
    ls = np.array([4, 6], dtype=np.int32)

    def bondorder():
        q2, b2, g2 = np.full((3, 150, 2), SENT), np.full((3, 150, 2), SENT), np.full((3, 2), SENT)
        nb = np.full((3, 150), ISENT, dtype=np.int32)
        rc = L.nm_distr_bondorder(0, 3, 150, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), 0.0, 0.4 * l, 2,
                                  ls.ctypes.data_as(B.c_int_p), q2.ctypes.data_as(B.c_double_p), b2.ctypes.data_as(B.c_double_p),
                                  g2.ctypes.data_as(B.c_double_p), nb.ctypes.data_as(B.c_int32_p))
        assert rc == 0
        return q2, b2, g2, nb
    before = bondorder()
    out = run(pos, box, 0.4 * l, 0.12, 64, 0.3 * l)
    after = bondorder()
    for a, b in zip(before, after):
        assert a.tobytes() == b.tobytes()
    np.testing.assert_array_equal(out['nnb'], before[3])                      # the entries are nm_distr_bondorder's with r_lo = 0


# ---- refusals
REFUSED = {
    'ns-1': dict(ns=-1), 'natoms0': dict(natoms=0), 'natoms4096': dict(natoms=4096), 'nbins0': dict(nbins=0), 'nbins1025': dict(nbins=1025),
    'sigma0': dict(sigma=0.0), 'sigma-negative': dict(sigma=-0.1), 'sigma-nan': dict(sigma=NAN), 'sigma-inf': dict(sigma=INF),
    'r_m0': dict(r_m=0.0), 'r_m-negative': dict(r_m=-1.0), 'r_m-nan': dict(r_m=NAN), 'r_m-inf': dict(r_m=INF),
    'r_m-beyond-half-the-smaller-box': dict(box=[3.0, 2.7], r_m=1.4), 'r_avg-beyond-half-the-smaller-box': dict(box=[3.0, 2.7], r_avg=1.4),
    'r_avg0': dict(r_avg=0.0), 'r_avg-negative': dict(r_avg=-0.5), 'r_avg-nan': dict(r_avg=NAN), 'r_avg-inf': dict(r_avg=INF),
    's_cut-nan': dict(s_cut=NAN), 'box-zero': dict(box=[3.0, 0.0]), 'box-negative': dict(box=[-3.0, 3.0]), 'box-nan': dict(box=[3.0, NAN]),
    'box-inf': dict(box=[INF, 3.0]), 'null-pos': dict(null=('pos',)), 'null-box': dict(null=('box',)), 'all-outputs-null': dict(null=NAMES),
    'device-1': dict(device=-1), 'device-out-of-range': dict(device=4096),
}


@pytest.mark.parametrize('case', sorted(REFUSED))
def test_refusals_leave_the_outputs_untouched(case):
    kw = dict(r_m=1.0, sigma=0.1, nbins=16, r_avg=1.0, s_cut=0.0)
    kw.update(REFUSED[case])
    rng = np.random.default_rng(5)
    box = np.array(kw.pop('box', [3.0, 3.0]), dtype=np.float32)
    pos = (rng.random((2, 8, 3)) * 2.9).astype(np.float32)
    rc, msg, out = call(pos, box, **kw)
    assert rc == B.NM_ERR_ARG
    assert msg.startswith('nm_distr_entropy:')
    assert untouched(out)


def test_empty_batch_and_infinite_cuts():
    rng = np.random.default_rng(10400)
    pos, box = liquid(rng, 2, 20)
    l = float(box.min())
    rc, msg, out = call(pos[:0], box[:0], 0.5, 0.1, 16, 0.5)
    assert rc == B.NM_OK, msg
    rc, msg, out = call(pos, box, 0.5, 0.1, 16, 0.5, ns=0)
    assert rc == B.NM_OK and untouched(out)
    assert (run(pos, box, 0.5 * l, 0.1, 16, 0.5 * l, -INF)['nlow'] == 0).all()
    assert (run(pos, box, 0.5 * l, 0.1, 16, 0.5 * l, INF)['nlow'] == 20).all()


# ---- the command line
def test_cli_writes_the_entropy_files(tmp_path, monkeypatch):
    """distr.main with -le -lt -la -ef on a 2 x 2 grid of parsed frames (2 samples each, 108 atoms): every file with the documented
    shape and dtype and the values of local_entropy() / entropy_functional(), the six other files byte-identical to a run without the
    flags, which writes none of the new ones; reweight's loader takes the means as they are"""
    rng = np.random.default_rng(10500)
    pn, tn, sn, n = 2, 2, 2, 108
    old = ('cdf', 'dn', 'dni', 'r', 'rdf', 'rv')
    new = ('ef', 'leb', 'leba', 'lef', 'len', 'les', 'lesa', 's2')
    ns = pn * tn * sn
    p, _ = fcc_integer(3)
    box = (4.8 + 0.03 * np.arange(ns)).astype(np.float32)
    noise = np.where(np.arange(ns) % 2 == 0, 0.01, 0.08)[:, None, None]
    pos = np.array([((p / 6.0 + nz * rng.normal(size=p.shape)) % 1.0) * b for b, nz in zip(box, noise)]).astype(np.float32)
    natoms = np.full((pn, tn, sn), n, dtype=np.uint16)
    files = {}
    for sub, extra in (('plain', []), ('le', ['-le']), ('all', ['-le', '-lt', '-4.0', '-la', '-ef'])):
        d = tmp_path / sub
        d.mkdir()
        pref = str(d / 'd7.lj.fcc.lammps')
        np.save(pref + '.virial.trgt.npy', np.linspace(1, 8, pn, dtype=np.float32))
        np.save(pref + '.temp.trgt.npy', np.linspace(0.25, 2.5, tn, dtype=np.float32))
        np.save(pref + '.natoms.npy', natoms)
        np.save(pref + '.box.npy', box.reshape(pn, tn, sn))
        np.save(pref + '.pos.npy', pos.reshape(pn, tn, sn, n, 3))
        monkeypatch.chdir(d)
        before = set(os.listdir(d))
        distr.main(['-n', 'd7', '-e', 'LJ', '-sb', '32', '-cb', '6'] + extra)
        files[sub] = {f: open(os.path.join(d, f), 'rb').read() for f in sorted(set(os.listdir(d)) - before)}
    base = 'd7.lj.fcc.lammps.'
    assert sorted(files['plain']) == [base + x + '.npy' for x in old]
    assert sorted(set(files['le']) - set(files['plain'])) == [base + x + '.npy' for x in ('leb', 'len', 'les')]
    assert sorted(set(files['all']) - set(files['plain'])) == [base + x + '.npy' for x in new]
    for sub in ('le', 'all'):
        for nm in old:
            assert files[sub][base + nm + '.npy'] == files['plain'][base + nm + '.npy'], nm
    l = float(box.min())
    rm, sigma, nbins, ravg = distr.entropy_params(distr.parse_args(['-le']), n)
    s, sbar, nnb, smean, sbarmean, nlow = distr.local_entropy(natoms.reshape(-1), box, pos, rm * l, sigma * l, nbins, ravg * l, -4.0)
    load = lambda x: np.load(str(tmp_path / 'all' / (base + x + '.npy')))
    for x, want in (('les', smean), ('leb', sbarmean), ('len', nnb.mean(axis=1)), ('lef', nlow / np.float64(n))):
        a = load(x)
        assert a.dtype == np.float64 and a.shape == (pn, tn, sn), x
        np.testing.assert_array_equal(a.reshape(ns), want)
        if x != 'lef':
            assert files['le'][base + x + '.npy'] == files['all'][base + x + '.npy']
    for x, want in (('lesa', s), ('leba', sbar)):
        a = load(x)
        assert a.dtype == np.float64 and a.shape == (pn, tn, sn, n), x
        np.testing.assert_array_equal(a.reshape(ns, n), want)
    leb = load('leb').reshape(ns)
    print('cli: mean sbar %s, below -4: %s' % (leb.round(3), load('lef').reshape(ns).round(3)))
    assert leb[0::2].max() < leb[1::2].min()                                  # the colder frames lie lower
    ef, s2, rdf, r = load('ef'), load('s2'), load('rdf'), load('r')
    assert ef.dtype == np.float32 and ef.shape == rdf.shape == (pn, tn, sn, 32) and s2.dtype == np.float64 and s2.shape == (pn, tn, sn)
    wef, ws2 = distr.entropy_functional(rdf.reshape(ns, 32), r, np.float32(n) / box ** 3)
    np.testing.assert_array_equal(ef.reshape(ns, 32), wef.astype(np.float32))
    np.testing.assert_array_equal(s2.reshape(ns), ws2)
    assert (s2 < 0).all() and s2.reshape(ns)[0::2].max() < s2.reshape(ns)[1::2].min()
    obs = reweight.load_observables(str(tmp_path / 'all' / base[:-1]), ['les', 'leb', 'lef', 's2'], (pn, tn, sn))   # reweight -ob les leb -hq leb
    assert len(obs) == 4 and np.array_equal(obs[1], load('leb'))
