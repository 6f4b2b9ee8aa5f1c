"""nm_distr_bondorder (include/nm_distr.h) on the GPU: the squares q2, qbar2, Q2 and the neighbour counts through the C-ABI against
the long-double restatement tests/bondorder_ref.py.  Every call runs on sentinel-filled outputs and is checked for three things:
nnb equal exactly, every output written completely, and the squares within twice the derived bound bondorder_ref.tol (absolute),
which stays below 1e-12 for every l <= 12.

Covered: random liquids on both sides of the block of centres (32), of the wave (64) and of 256 atoms at a first-shell cutoff and
at half the box (more than 64 neighbours from about 130 atoms up: several batches of the wave's list); a cluster with 529
neighbours per centre; 2048 atoms; a sparse frame with empty and single-neighbour shells; the l sets (4, 6), (1,), (12,) and (2,
.., 12); lattices on integer coordinates (fcc, simple cubic with bonds on the poles, a cutoff exactly on the second-neighbour
distance, every neighbour in two images); boxes that differ inside a batch, an unwrapped frame, a metal-unit box, coincident atoms,
two launch chunks, a batch that the scratch cap splits; the entries against nm_distr_angles' neighbours; NULL outputs; a
permutation, an exact translation, determinism; crystal against ideal gas; the command line."""
import os

import numpy as np
import pytest

import bondorder_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import distr

pytestmark = pytest.mark.gpu

SENT = -7.25e300
ISENT = -77777777
NAMES = ('q2', 'qbar2', 'Q2', 'nnb')


def call(pos, box, ls, r_lo, r_hi, want=NAMES, device=0):
    """the raw ABI on sentinel-filled outputs, NULL for the outputs not in `want`; returns (rc, message, dict of the four arrays)"""
    L = B.load()
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    box = np.ascontiguousarray(box, dtype=np.float32).reshape(-1)
    ls = np.ascontiguousarray(ls, dtype=np.int32)
    ns, n, nl = pos.shape[0], pos.shape[1], len(ls)
    out = dict(q2=np.full((ns, n, nl), SENT), qbar2=np.full((ns, n, nl), SENT), Q2=np.full((ns, nl), SENT),
               nnb=np.full((ns, n), ISENT, dtype=np.int32))
    ptr = {k: (out[k].ctypes.data_as(B.c_int32_p if k == 'nnb' else B.c_double_p) if k in want else None) for k in NAMES}
    rc = L.nm_distr_bondorder(device, ns, n, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), float(r_lo), float(r_hi),
                              nl, ls.ctypes.data_as(B.c_int_p), ptr['q2'], ptr['qbar2'], ptr['Q2'], ptr['nnb'])
    return rc, (L.nm_distr_last_error().decode() if rc else ''), out


def run(pos, box, ls, r_lo, r_hi):
    rc, msg, out = call(pos, box, ls, r_lo, r_hi)
    assert rc == 0, msg
    for k in ('q2', 'qbar2', 'Q2'):
        assert (out[k] != SENT).all(), k + ' is not written completely'
    assert (out['nnb'] != ISENT).all(), 'nnb is not written completely'
    return out


def check(pos, box, ls, r_lo, r_hi):
    """the four outputs against the restatement; returns (outputs, restatement)"""
    pos = np.asarray(pos, dtype=np.float32)
    box = np.asarray(box, dtype=np.float32).reshape(-1)
    out = run(pos, box, ls, r_lo, r_hi)
    ref = dict(zip(NAMES, R.bond_order2(pos, box, ls, r_lo, r_hi)))
    np.testing.assert_array_equal(out['nnb'], ref['nnb'])
    m, n = int(ref['nnb'].max()), pos.shape[1]
    for k, which in (('q2', 'q'), ('qbar2', 'qbar'), ('Q2', 'Q')):
        for i, l in enumerate(ls):
            want = ref[k][..., i]
            tol = 2 * R.tol(l, want.astype(np.float64), m, n, which)
            assert tol.max() <= 1e-12
            err = np.abs(out[k][..., i].astype(R.LD) - want).astype(np.float64)
            print('%s l = %d: max |error| %.3g, smallest allowed %.3g, largest error / allowed %.3g (%d neighbours at most)'
                  % (k, l, err.max(), tol.min(), (err / tol).max(), m))
            assert (err <= tol).all(), (k, l)
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


def cubic_integer(cells):
    g = np.arange(cells)
    return np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3).astype(np.float32), np.float32(cells)


# ---- random liquids
@pytest.mark.parametrize('shell', ('first', 'half'))
@pytest.mark.parametrize('n', (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 500))
def test_liquid(n, shell):
    rng = np.random.default_rng(7000 + n)
    pos, box = liquid(rng, 2 if n <= 257 else 1, n)
    l = float(box.min())
    if shell == 'first':
        out, ref = check(pos, box, (4, 6), 1e-16 * l, min(1.5, 0.5 * l))
    else:
        out, ref = check(pos, box, (1, 6, 12), 1e-16 * l, 0.5 * l)
        if n == 65:
            assert 22 <= ref['nnb'].min() and ref['nnb'].max() <= 44
        if n >= 255:
            assert ref['nnb'].min() > 64
    if n == 1:
        assert not out['nnb'].any() and not out['q2'].any() and not out['qbar2'].any() and not out['Q2'].any()


def test_more_than_256_neighbours():
    """530 atoms inside a ball of diameter < l/2: 529 neighbours per centre, nine batches of the wave's list"""
    rng = np.random.default_rng(7100)
    n, L = 530, 10.0
    u = rng.normal(size=(n, 3))
    u *= (2.4 * rng.random(n) ** (1 / 3) / np.linalg.norm(u, axis=1))[:, None]
    out, ref = check((u + 5.0).astype(np.float32)[None], [np.float32(L)], (4, 6), 1e-16 * L, 0.5 * L)
    assert (ref['nnb'] == 529).all()


def test_largest_size():
    rng = np.random.default_rng(7200)
    pos, box = liquid(rng, 1, 2048)
    out, ref = check(pos, box, (4, 6), 1e-16, 1.5)
    assert 8 < ref['nnb'].mean() < 18


def test_sparse_frame_with_empty_and_single_neighbour_shells():
    rng = np.random.default_rng(7300)
    pos, box = liquid(rng, 2, 100, rho=0.05)
    out, ref = check(pos, box, (4, 6), 1e-16, 0.9)
    assert (ref['nnb'] == 0).any() and (ref['nnb'] == 1).any()
    lone = ref['nnb'] == 0
    assert not out['q2'][lone].any() and not out['qbar2'][lone].any()
    assert np.abs(out['q2'][ref['nnb'] == 1] - 1.0).max() < 1e-13


@pytest.mark.parametrize('ls', ((4, 6), (1,), (12,), (2, 4, 6, 8, 10, 12)))
def test_l_sets(ls):
    rng = np.random.default_rng(7400 + len(ls) + ls[0])
    pos, box = liquid(rng, 2, 150)
    l = float(box.min())
    out, ref = check(pos, box, ls, 1e-16 * l, 0.5 * l)
    assert ref['nnb'].max() > 64


# ---- lattices on integer coordinates
def test_fcc_lattice_known_answers():
    pos, box = fcc_integer(3)
    out, ref = check(pos[None], [box], (2, 4, 6), 0.0, 1.7)
    assert (out['nnb'] == 12).all()
    for i, want in enumerate((0.0, 0.190941, 0.574524)):
        for k in ('q2', 'qbar2', 'Q2'):
            assert np.abs(np.sqrt(out[k][..., i]) - want).max() < (1e-6 if want else 1e-12), (k, i)


def test_simple_cubic_lattice_has_bonds_on_the_poles():
    pos, box = cubic_integer(4)
    out, ref = check(pos[None], [box], (4, 6), 0.0, 1.2)
    assert (out['nnb'] == 6).all()
    for i, want in enumerate((0.763763, 0.353553)):
        for k in ('q2', 'qbar2', 'Q2'):
            assert np.abs(np.sqrt(out[k][..., i]) - want).max() < 1e-6


def test_fcc_cutoff_exactly_on_the_second_neighbour_distance():
    """a0 = 2: the six second neighbours sit at d = 2 = r_hi, the closed end of the shell"""
    pos, box = fcc_integer(3)
    out, ref = check(pos[None], [box], (4, 6), 0.0, 2.0)
    assert (out['nnb'] == 18).all()
    inside = run(pos[None], [box], (4, 6), 0.0, np.nextafter(2.0, 0.0))
    assert (inside['nnb'] == 12).all()


def test_every_neighbour_in_two_images():
    """a 2^3 grid of spacing 1 in a box of 2 with r_hi = box / 2: each of the six directions is reached in two images, two entries"""
    pos, box = cubic_integer(2)
    out, ref = check(pos[None], [box], (4, 6), 0.0, 1.0)
    assert (out['nnb'] == 6).all()
    assert np.abs(np.sqrt(out['q2'][..., 0]) - 0.763763).max() < 1e-6


# ---- batches and boxes
def test_boxes_that_differ_inside_one_batch():
    rng = np.random.default_rng(7500)
    pos, box = liquid(rng, 4, 120, spread=0.5)
    out, ref = check(pos, box, (4, 6), 1e-16, 0.5 * float(box.min()))
    assert len({a.tobytes() for a in out['Q2']}) == 4


def test_unwrapped_frame():
    rng = np.random.default_rng(7600)
    pos, box = liquid(rng, 3, 130)
    l = float(box.min())
    wrapped = run(pos, box, (4, 6), 1e-16 * l, 0.3 * l)
    pos[0] -= box[0]
    pos[1] += (rng.integers(-1, 2, pos[1].shape) * box[1]).astype(np.float32)
    pos[2] += (rng.integers(-3, 4, pos[2].shape) * box[2]).astype(np.float32)   # beyond the 27 images: fewer neighbours
    out, ref = check(pos, box, (4, 6), 1e-16 * l, 0.3 * l)
    assert out['nnb'][2].sum() < wrapped['nnb'][2].sum()


def test_metal_unit_box():
    """element Al in Angstrom: a displaced 4^3 fcc lattice, a0 = 4.05, box 16.2, first shell"""
    rng = np.random.default_rng(7700)
    p, _ = fcc_integer(4)
    b = np.float32(4 * 4.05)
    pos = (p * (4.05 / 2) + 0.3 * (rng.random(p.shape) - 0.5)).astype(np.float32)[None]
    out, ref = check(pos, [b], (4, 6), 1e-16 * float(b), 0.853553 * 4.05)
    assert 11.5 < out['nnb'].mean() < 12.5 and np.sqrt(out['q2'][..., 1]).mean() > 0.4


def test_coincident_atoms():
    """every atom has a twin at d = 0, outside the shell for r_lo = 0; the twins share their neighbours and their values"""
    rng = np.random.default_rng(7800)
    pos, box = liquid(rng, 2, 120)
    pos[:, 1::2] = pos[:, 0::2]
    out, ref = check(pos, box, (4, 6), 0.0, 0.5 * float(box.min()))
    assert np.array_equal(out['nnb'][:, 0::2], out['nnb'][:, 1::2]) and out['q2'][:, 0::2].tobytes() == out['q2'][:, 1::2].tobytes()


def test_more_samples_than_one_launch_chunk():
    """4096 + 1 samples of 5 atoms: two launches, the second with one sample"""
    rng = np.random.default_rng(7900)
    pos, box = liquid(rng, 4097, 5, rho=0.8, spread=0.3)
    out, ref = check(pos, box, (4, 6), 1e-16, 0.5 * float(box.min()))
    for s in (0, 4095, 4096):
        assert out['nnb'][s].sum() > 0


def test_scratch_cap_splits_the_batch():
    """4096 samples of 66 atoms with l = 7 .. 12: nc2 = 2 * (8 + 9 + 10 + 11 + 12 + 13) = 126 doubles per atom, so a sample's moments
    take 66 * 126 * 8 = 66,528 B of the scratch, and 2^28 // 66,528 = 4034 of them fit under the cap of 256 MiB (4034 * 66,528 =
    268,373,952 <= 268,435,456 < 4035 * 66,528): launch chunks of 4034 and 62 samples where the sample cap alone would give one.
    The samples on both sides of the seam and the last one equal, bit for bit, a call of their own (the entry point is
    reproducible bit for bit), and four of them pass the restatement.  This checks the results across the seam, not that the
    batch is split: one launch of 4096 samples would give the same bits, and the split cannot be seen through the entry point"""
    ls = (7, 8, 9, 10, 11, 12)
    rng = np.random.default_rng(7950)
    pos, box = liquid(rng, 4096, 66)
    assert float(box.min()) > 3.0
    big = run(pos, box, ls, 1e-16, 1.5)
    for sl in (slice(4030, 4040), slice(4095, 4096)):
        part = run(pos[sl], box[sl], ls, 1e-16, 1.5)
        for k in NAMES:
            assert big[k][sl].tobytes() == part[k].tobytes(), (k, sl)
    pick = [0, 4033, 4034, 4095]
    out, ref = check(pos[pick], box[pick], ls, 1e-16, 1.5)
    for k in NAMES:
        assert big[k][pick].tobytes() == out[k].tobytes(), k
    assert out['nnb'].sum() > 0


# ---- the entries are the neighbours of nm_distr_angles
def test_entries_are_the_neighbours_of_the_angular_distribution():
    """nm_distr_angles with the edges cos = (1, 0, -1) counts every unordered pair of a centre's neighbours in one of its two bins
    (the clipped cosine lies in [-1, 1]); with Nb(c) entries per centre that is sum_c Nb(c) (Nb(c) - 1) / 2, in integers.  Liquids of
    65 and 257 atoms at half the box and the ball of test_more_than_256_neighbours (529 neighbours: three tiles of the angular
    kernel, nine batches of the list)"""
    L = B.load()
    frames = []
    for n in (65, 257):
        pos, box = liquid(np.random.default_rng(7000 + n), 2, n)
        frames.append((pos, box, 1e-16 * float(box.min()), 0.5 * float(box.min())))
    rng = np.random.default_rng(7100)
    u = rng.normal(size=(530, 3))
    u *= (2.4 * rng.random(530) ** (1 / 3) / np.linalg.norm(u, axis=1))[:, None]
    frames.append(((u + 5.0).astype(np.float32)[None], np.full(1, 10.0, dtype=np.float32), 1e-15, 5.0))
    ce = np.array([1.0, 0.0, -1.0])
    for pos, box, r_lo, r_hi in frames:
        pos = np.ascontiguousarray(pos, dtype=np.float32)
        rc, msg, out = call(pos, box, (4,), r_lo, r_hi, want=('nnb',))
        assert rc == 0, msg
        adf = np.full((pos.shape[0], 3), 2 ** 64 - 1, dtype=np.uint64)
        rc = L.nm_distr_angles(0, pos.shape[0], pos.shape[1], pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p),
                               float(r_lo), float(r_hi), 3, ce.ctypes.data_as(B.c_double_p), adf.ctypes.data_as(B.c_uint64_p))
        assert rc == 0, L.nm_distr_last_error().decode()
        for s in range(pos.shape[0]):
            nb = [int(x) for x in out['nnb'][s]]
            assert min(nb) >= 0 and max(nb) > 1
            assert int(adf[s, 0]) == 0
            assert int(adf[s, 1]) + int(adf[s, 2]) == sum(m * (m - 1) // 2 for m in nb), (pos.shape[1], s)
        if pos.shape[1] == 530:
            assert (out['nnb'] == 529).all()


# ---- NULL outputs, invariance, determinism
def test_null_outputs():
    rng = np.random.default_rng(8000)
    pos, box = liquid(rng, 3, 100)
    l = float(box.min())
    full, ref = check(pos, box, (4, 6), 1e-16 * l, 0.4 * l)
    sent = dict(q2=SENT, qbar2=SENT, Q2=SENT, nnb=ISENT)
    for k in NAMES:
        for want in ((k,), tuple(x for x in NAMES if x != k)):
            rc, msg, out = call(pos, box, (4, 6), 1e-16 * l, 0.4 * l, want=want)
            assert rc == 0, msg
            for x in NAMES:
                if x in want:
                    assert out[x].tobytes() == full[x].tobytes(), (want, x)
                else:
                    assert (out[x] == sent[x]).all(), (want, x)


def test_permutation_of_the_atoms():
    rng = np.random.default_rng(8100)
    pos, box = liquid(rng, 2, 200)
    l = float(box.min())
    one, ref = check(pos, box, (4, 6), 1e-16 * l, 0.4 * l)
    p = rng.permutation(200)
    two = run(pos[:, p], box, (4, 6), 1e-16 * l, 0.4 * l)
    np.testing.assert_array_equal(two['nnb'], one['nnb'][:, p])
    m = int(one['nnb'].max())
    for i, lv in enumerate((4, 6)):
        for k, which in (('q2', 'q'), ('qbar2', 'qbar')):
            assert (np.abs(two[k][:, :, i] - one[k][:, p, i]) <= 4 * R.tol(lv, one[k][:, p, i], m, 200, which)).all()
        assert (np.abs(two['Q2'][:, i] - one['Q2'][:, i]) <= 4 * R.tol(lv, one['Q2'][:, i], m, 200, 'Q')).all()


def test_translation_by_a_grid_vector_changes_no_bit():
    """distinct points of the integer grid of an 8-box: every displacement is an integer, before and after the shift"""
    rng = np.random.default_rng(8200)
    g = np.array([rng.permutation(512)[:90] for _ in range(2)])
    pos = np.stack([g // 64, (g // 8) % 8, g % 8], axis=-1).astype(np.float32)
    box = np.full(2, 8.0, dtype=np.float32)
    one, ref = check(pos, box, (4, 6), 0.0, 3.0)
    two = run(pos + np.array([3.0, -5.0, 16.0], dtype=np.float32), box, (4, 6), 0.0, 3.0)
    for k in NAMES:
        assert one[k].tobytes() == two[k].tobytes(), k
    assert one['nnb'].sum() > 0


def test_two_calls_are_equal_bit_for_bit():
    rng = np.random.default_rng(8300)
    pos, box = liquid(rng, 6, 300)
    l = float(box.min())
    a, ref = check(pos, box, (4, 6), 1e-16 * l, 0.5 * l)
    b = run(pos, box, (4, 6), 1e-16 * l, 0.5 * l)
    for k in NAMES:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a['Q2'].sum() > 0


def test_device_ordinal_out_of_range_and_empty_batch():
    rng = np.random.default_rng(8400)
    pos, box = liquid(rng, 2, 20)
    rc, msg, out = call(pos, box, (4, 6), 1e-16, 0.5 * float(box.min()), device=4096)
    assert rc == B.NM_ERR_ARG and msg.startswith('nm_distr_bondorder:')
    assert (out['q2'] == SENT).all() and (out['qbar2'] == SENT).all() and (out['Q2'] == SENT).all() and (out['nnb'] == ISENT).all()
    rc, msg, out = call(pos[:0], box[:0], (4, 6), 1e-16, 1.0)
    assert rc == B.NM_OK, msg


# ---- sanity
def test_crystal_against_ideal_gas():
    """108 atoms, a0 = 2: fcc with Gaussian displacements of 0.08 neighbour distances against uniform random atoms in the same box,
    cutoff 1.7: the mean qbar6 separates the two, and by a larger ratio than the mean q6 (restatement and kernel alike)"""
    rng = np.random.default_rng(8500)
    p, box = fcc_integer(3)
    solid = ((p + 0.08 * np.sqrt(2.0) * rng.normal(size=p.shape)) % box).astype(np.float32)
    gas = (rng.random(p.shape) * box).astype(np.float32)
    out, ref = check(np.stack([solid, gas]), [box, box], (6,), 1e-16, 1.7)
    for name, d in (('restatement', ref), ('kernel', out)):
        q = np.sqrt(np.maximum(d['q2'][..., 0].astype(np.float64), 0)).mean(axis=1)
        qb = np.sqrt(np.maximum(d['qbar2'][..., 0].astype(np.float64), 0)).mean(axis=1)
        print('%s: q6 %.3f against %.3f, qbar6 %.3f against %.3f' % (name, q[0], q[1], qb[0], qb[1]))
        assert qb[0] > qb[1] and qb[0] / qb[1] > q[0] / q[1]


# ---- the command line
def test_cli_writes_the_bond_order_files(tmp_path, monkeypatch):
    """distr.main with -bo on a 2 x 2 grid of parsed frames (2 samples each, 108 atoms): the five files, with -ba the three per-atom
    files, with the documented shapes and dtypes and the values of bond_order(); the six other files are byte-identical to a run
    without -bo, which writes none of them"""
    rng = np.random.default_rng(8600)
    pn, tn, sn, n = 2, 2, 2, 108
    names = ('dni', 'r', 'rdf', 'dn', 'rv', 'cdf')
    new = ('bob', 'bog', 'bol', 'bon', 'boq')
    per_atom = ('boba', 'bona', 'boqa')
    ns = pn * tn * sn
    p, _ = fcc_integer(3)
    box = (4.8 + 0.03 * np.arange(ns)).astype(np.float32)
    pos = np.array([((p / 6.0 + 0.02 * rng.normal(size=p.shape)) % 1.0) * b for b in box]).astype(np.float32)
    natoms = np.full((pn, tn, sn), n, dtype=np.uint16)
    files = {}
    for sub, extra in (('plain', []), ('bo', ['-bo']), ('atoms', ['-bo', '-bl', '6', '2', '-bc', '0.3', '-ba'])):
        d = tmp_path / sub
        d.mkdir()
        pref = str(d / 'd5.lj.fcc.lammps')
        np.save(pref + '.virial.trgt.npy', np.linspace(1, 8, pn, dtype=np.float32))
        np.save(pref + '.temp.trgt.npy', np.linspace(0.25, 2.5, tn, dtype=np.float32))
        np.save(pref + '.natoms.npy', natoms)
        np.save(pref + '.box.npy', box.reshape(pn, tn, sn))
        np.save(pref + '.pos.npy', pos.reshape(pn, tn, sn, n, 3))
        monkeypatch.chdir(d)
        distr.main(['-n', 'd5', '-e', 'LJ', '-sb', '32', '-cb', '6'] + extra)
        files[sub] = {f: open(os.path.join(d, f), 'rb').read() for f in sorted(os.listdir(d))}
    base = 'd5.lj.fcc.lammps.'
    assert not any(f.endswith(tuple('.%s.npy' % x for x in new + per_atom)) for f in files['plain'])
    assert sorted(set(files['bo']) - set(files['plain'])) == [base + x + '.npy' for x in new]
    assert sorted(set(files['atoms']) - set(files['plain'])) == [base + x + '.npy' for x in sorted(new + per_atom)]
    for sub in ('bo', 'atoms'):
        for nm in names:
            assert files[sub][base + nm + '.npy'] == files['plain'][base + nm + '.npy'], nm
    l = float(box.min())
    for sub, ls, cut in (('bo', [4, 6], 0.853553 / 3), ('atoms', [2, 6], 0.3)):
        load = lambda x: np.load(str(tmp_path / sub / (base + x + '.npy')))
        q, qb, qg, nb = distr.bond_order(natoms.reshape(-1), box, pos, ls, 1e-16 * l, cut * l)
        assert q.shape == (ns, n, 2) and qb.shape == (ns, n, 2) and qg.shape == (ns, 2) and nb.shape == (ns, n) and nb.dtype == np.int32
        bol, boq, bob, bog, bon = load('bol'), load('boq'), load('bob'), load('bog'), load('bon')
        assert bol.dtype == np.int64 and bol.tolist() == ls
        for a in (boq, bob, bog):
            assert a.dtype == np.float32 and a.shape == (pn, tn, sn, 2)
        assert bon.dtype == np.float32 and bon.shape == (pn, tn, sn)
        np.testing.assert_array_equal(boq.reshape(ns, 2), q.mean(axis=1).astype(np.float32))
        np.testing.assert_array_equal(bob.reshape(ns, 2), qb.mean(axis=1).astype(np.float32))
        np.testing.assert_array_equal(bog.reshape(ns, 2), qg.astype(np.float32))
        np.testing.assert_array_equal(bon.reshape(ns), nb.mean(axis=1).astype(np.float32))
        if sub == 'atoms':
            boqa, boba, bona = load('boqa'), load('boba'), load('bona')
            assert boqa.dtype == np.float32 and boqa.shape == (pn, tn, sn, n, 2) and boba.dtype == np.float32 and boba.shape == boqa.shape
            assert bona.dtype == np.int32 and bona.shape == (pn, tn, sn, n)
            np.testing.assert_array_equal(boqa.reshape(ns, n, 2), q.astype(np.float32))
            np.testing.assert_array_equal(boba.reshape(ns, n, 2), qb.astype(np.float32))
            np.testing.assert_array_equal(bona.reshape(ns, n), nb)
        else:
            assert 11 < bon.mean() < 13 and boq[..., 1].mean() > 0.4
