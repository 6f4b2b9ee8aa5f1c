"""nm_distr_solid (include/nm_distr.h) on the GPU: the five integer outputs through the C-ABI against the long-double restatement
tests/solid_ref.py.  Every call runs on sentinel-filled outputs and is checked for complete writes and for EXACT equality of
nconn, label, nsolid, nclus and largest.

Condition, not tolerance: the kernel's bond values differ from the restatement's by rounding errors, so the comparison s > s_min can
only be demanded where the restatement's value lies further from s_min than its margin (solid_ref.decided).  Every frame here is
chosen (its seed, on the CPU) so that ALL its entries are decided; check() asserts that before it compares.  An undecided entry
means another seed, never a looser comparison.

Covered: random liquids on both sides of the block of centres (32), of the wave (64) and of 256 atoms at a first-shell cutoff and at
half the box (several batches of the wave's list) at the default (s_min, n_min) and at (0, 1); displaced and noised fcc crystals at
256 and 2048 atoms; two crystallites with interleaved indices; a crystallite that holds together only through the periodic boundary;
a closed chain of 2048 atoms with permuted indices (the deepest trees of the union); l = 4, 6, 12; n_min on and one above an atom's
count; integer lattices (every neighbour in two images, a cutoff on a neighbour distance); boxes that differ inside a batch, an
unwrapped frame, coincident atoms, two launch chunks, a batch that the scratch cap splits; NULL outputs; determinism; a permutation;
nm_distr_bondorder untouched by a call; the command line."""
import os

import numpy as np
import pytest

import solid_ref as S
from neuralmelting_amd import _lib as B
from neuralmelting_amd import distr

pytestmark = pytest.mark.gpu

ISENT = -77777777
NAMES = ('nconn', 'label', 'nsolid', 'nclus', 'largest')
DEFAULTS = (0.5, 8)
LOOSE = (0.0, 1)


def call(pos, box, l, r_lo, r_hi, s_min, n_min, want=NAMES, device=0):
    """the raw ABI on sentinel-filled outputs, NULL for the outputs not in `want`; returns (rc, message, dict of the five arrays)"""
    L = B.load()
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    box = np.ascontiguousarray(box, dtype=np.float32).reshape(-1)
    ns, n = pos.shape[0], pos.shape[1]
    out = {k: np.full((ns, n) if k in ('nconn', 'label') else (ns,), ISENT, dtype=np.int32) for k in NAMES}
    ptr = [out[k].ctypes.data_as(B.c_int32_p) if k in want else None for k in NAMES]
    rc = L.nm_distr_solid(device, ns, n, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), float(r_lo), float(r_hi),
                          int(l), float(s_min), int(n_min), *ptr)
    return rc, (L.nm_distr_last_error().decode() if rc else ''), out


def run(pos, box, l, r_lo, r_hi, s_min, n_min):
    rc, msg, out = call(pos, box, l, r_lo, r_hi, s_min, n_min)
    assert rc == 0, msg
    for k in NAMES:
        assert (out[k] != ISENT).all(), k + ' is not written completely'
    return out


def compare(out, ref, s_min):
    """the condition (every entry decided), then exact equality of the five outputs"""
    dist = np.abs(ref['s'] - S.LD(s_min)).astype(np.float64)
    print('%d entries; closest bond value to s_min %.3g; largest margin %.3g; undecided %d'
          % (len(dist), dist.min() if len(dist) else np.inf, ref['margin'].max() if len(dist) else 0.0, S.undecided(ref, s_min)))
    assert S.undecided(ref, s_min) == 0, 'the frame has undecided entries: choose another seed'
    for k in NAMES:
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)


def check(pos, box, l, r_lo, r_hi, params=(DEFAULTS,)):
    """the five outputs against the restatement for every (s_min, n_min) of params; returns [(outputs, restatement)]"""
    pos = np.asarray(pos, dtype=np.float32)
    box = np.asarray(box, dtype=np.float32).reshape(-1)
    b = S.bonds(pos, box, l, r_lo, r_hi)
    res = []
    for s_min, n_min in params:
        ref = S.classify(b, s_min, n_min)
        out = run(pos, box, l, r_lo, r_hi, s_min, n_min)
        compare(out, ref, s_min)
        res.append((out, ref))
    return res


def partition(label):
    return {frozenset(np.flatnonzero(label == k).tolist()) for k in np.unique(label[label >= 0])}


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


def noised_fcc(rng, cells, sigma):
    """fcc with a0 = 2 (neighbour distance sqrt 2) and Gaussian displacements of sigma per component, wrapped"""
    p, box = fcc_integer(cells)
    return ((p + sigma * rng.normal(size=p.shape)) % box).astype(np.float32), box


FIRST = 1.7       # between the first (1.414) and second (2) neighbour distance of fcc_integer


# ---- random liquids
@pytest.mark.parametrize('shell', ('first', 'half'))
@pytest.mark.parametrize('n', (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 500))
def test_liquid(n, shell):
    rng = np.random.default_rng(9000 + n)
    pos, box = liquid(rng, 2 if n <= 257 else 1, n)
    l = float(box.min())
    r_hi = min(1.5, 0.5 * l) if shell == 'first' else 0.5 * l
    (o1, r1), (o2, r2) = check(pos, box, 6, 1e-16 * l, r_hi, (DEFAULTS, LOOSE))
    if shell == 'half' and n >= 255:
        assert r1['nnb'].min() > 64                                           # several batches of the wave's list
    if n >= 31:
        assert r2['nsolid'].min() > n // 2 and (r2['nconn'] != r1['nconn']).any()
    if n == 1:
        assert not o1['nconn'].any() and (o1['label'] == -1).all() and not o1['nsolid'].any() and not o1['largest'].any()


# ---- crystals
def test_displaced_crystal_is_one_cluster():
    """fcc displaced uniformly by up to 3 % of a0 per component: every atom keeps its 12 connections"""
    rng = np.random.default_rng(9100)
    p, box = fcc_integer(4)
    pos = ((p + 0.06 * (rng.random(p.shape) - 0.5)) % box).astype(np.float32)
    (out, ref), = check(pos[None], [box], 6, 1e-16, FIRST)
    assert (out['nconn'] == 12).all() and (out['label'] == 0).all()
    assert out['nsolid'][0] == 256 and out['nclus'][0] == 1 and out['largest'][0] == 256


@pytest.mark.parametrize('cells', (4, 8))
def test_noised_crystal_is_partly_solid(cells):
    rng = np.random.default_rng(9200 + cells)
    pos, box = noised_fcc(rng, cells, 0.17)
    (out, ref), = check(pos[None], [box], 6, 1e-16, FIRST)
    n = 4 * cells ** 3
    assert 0.1 * n < out['nsolid'][0] < 0.98 * n and out['largest'][0] > 0.05 * n
    assert (out['label'] == -1).sum() == n - out['nsolid'][0]


def crystallites(rng, order):
    """two 4^3-cell fcc blocks (a0 = 2, 256 atoms each, slightly displaced) 20 apart in a box of 40; the atoms in `order`"""
    p, _ = fcc_integer(4)
    a = p + np.array([4.0, 4.0, 4.0]) + 0.04 * (rng.random(p.shape) - 0.5)
    b = p + np.array([24.0, 24.0, 24.0]) + 0.04 * (rng.random(p.shape) - 0.5)
    both = np.empty((512, 3))
    both[0::2], both[1::2] = a, b                                            # even indices in one block, odd ones in the other
    return both[order].astype(np.float32), np.float32(40.0)


def test_two_crystallites_with_interleaved_indices():
    """the blocks' surface atoms lack neighbours and are not solid-like; the interiors are two clusters.  The atoms 0 and 1 are
    moved to interior sites of the two blocks, so the labels are the two smallest indices"""
    rng = np.random.default_rng(9300)
    inner = 2 * (4 * (1 * 16 + 1 * 4 + 1) + 0)                              # cell (1, 1, 1), basis atom 0, of the even block
    order = np.arange(512)
    order[[0, inner]] = order[[inner, 0]]
    order[[1, inner + 1]] = order[[inner + 1, 1]]
    pos, box = crystallites(rng, order)
    (out, ref), = check(pos[None], [box], 6, 1e-16, FIRST)
    assert out['nclus'][0] == 2 and sorted(set(out['label'][0].tolist())) == [-1, 0, 1]
    assert out['label'][0, 0] == 0 and out['label'][0, 1] == 1
    assert (out['label'][0] == 0).sum() == (out['label'][0] == 1).sum() == out['largest'][0] > 20


def test_crystallite_connected_only_through_the_boundary():
    """a block that straddles the box's faces in x: wrapped into the box it is two slabs at opposite faces, one cluster through the
    periodic images, and two clusters in a box twice as large that has no such images"""
    rng = np.random.default_rng(9400)
    p, _ = fcc_integer(4)
    blk = p + 0.04 * (rng.random(p.shape) - 0.5) + np.array([-4.0, 8.0, 8.0])
    box = np.float32(24.0)
    pos = (blk % box).astype(np.float32)
    assert ((pos[:, 0] < 5) | (pos[:, 0] > 19)).all() and (pos[:, 0] < 5).any() and (pos[:, 0] > 19).any()
    (out, ref), = check(pos[None], [box], 6, 1e-16, FIRST)
    assert out['nclus'][0] == 1 and out['largest'][0] == out['nsolid'][0] > 20
    (far, _), = check(pos[None], [np.float32(48.0)], 6, 1e-16, FIRST, (LOOSE,))
    (near, _), = check(pos[None], [box], 6, 1e-16, FIRST, (LOOSE,))
    assert far['nclus'][0] == 2 and near['nclus'][0] == 1 and near['nsolid'][0] == far['nsolid'][0] == 256


def test_closed_chain_with_permuted_indices():
    """2048 atoms on a line with spacing 1 in a box of 2048, closed through the boundary, the indices permuted: every atom has two
    opposite bonds (s = 1 for even l), n_min 1: one cluster of 2048 with label 0, out of the deepest trees the union can meet"""
    rng = np.random.default_rng(9500)
    n = 2048
    pos = np.zeros((n, 3), dtype=np.float32)
    pos[:, 0] = rng.permutation(n)
    pos[:, 1:] = 1024.0
    (out, ref), = check(pos[None], [np.float32(n)], 6, 0.0, 1.2, ((0.5, 1),))
    assert (out['nconn'] == 2).all() and (out['label'] == 0).all()
    assert out['nsolid'][0] == n and out['nclus'][0] == 1 and out['largest'][0] == n


@pytest.mark.parametrize('l', (4, 6, 12))
def test_l_values(l):
    rng = np.random.default_rng(9600 + l)
    pos, box = noised_fcc(rng, 3, 0.12)
    lq, lbox = liquid(rng, 1, 108)
    lq = lq * (box / lbox[0])
    res = check(np.stack([pos, lq[0].astype(np.float32)]), [box, box], l, 1e-16, FIRST, (DEFAULTS, LOOSE))
    assert res[0][0]['nsolid'][0] > res[0][0]['nsolid'][1]


def test_n_min_on_and_above_an_atoms_count():
    rng = np.random.default_rng(9700)
    pos, box = noised_fcc(rng, 3, 0.15)
    b = S.bonds(pos[None], [box], 6, 1e-16, FIRST)
    nconn = S.classify(b, 0.5, 1)['nconn'][0]
    k = int(np.sort(nconn)[len(nconn) // 2])
    c = int(np.flatnonzero(nconn == k)[0])
    assert k >= 1
    (on, _), (above, _) = check(pos[None], [box], 6, 1e-16, FIRST, ((0.5, k), (0.5, k + 1)))
    assert on['nconn'][0, c] == k and on['label'][0, c] >= 0 and above['label'][0, c] == -1
    assert above['nsolid'][0] < on['nsolid'][0]


# ---- lattices on integer coordinates
def test_every_neighbour_in_two_images():
    """a 2^3 grid of spacing 1 in a box of 2 with r_hi = box / 2: each of the six directions is reached in two images, 6 entries for 3 atoms"""
    pos, box = cubic_integer(2)
    (out, ref), = check(pos[None], [box], 6, 0.0, 1.0, ((0.5, 6),))
    assert (ref['nnb'] == 6).all() and (out['nconn'] == 6).all() and (out['label'] == 0).all() and out['largest'][0] == 8


def test_cutoff_exactly_on_a_neighbour_distance():
    """a0 = 2: the six second neighbours sit at d = 2 = r_hi, the closed end of the shell: 18 entries, and 12 just inside"""
    pos, box = fcc_integer(3)
    (out, ref), = check(pos[None], [box], 6, 0.0, 2.0, ((0.5, 18),))
    assert (out['nconn'] == 18).all() and out['nclus'][0] == 1 and out['largest'][0] == 108
    (inside, _), = check(pos[None], [box], 6, 0.0, np.nextafter(2.0, 0.0), ((0.5, 13),))
    assert (inside['nconn'] == 12).all() and inside['nsolid'][0] == 0 and inside['nclus'][0] == 0 and inside['largest'][0] == 0


# ---- batches and boxes
def test_boxes_that_differ_inside_one_batch():
    rng = np.random.default_rng(9800)
    pos, box = liquid(rng, 4, 120, spread=0.5)
    res = check(pos, box, 6, 1e-16, 0.5 * float(box.min()), (DEFAULTS, LOOSE))
    assert len({a.tobytes() for a in res[1][0]['nconn']}) == 4


def test_unwrapped_frame():
    rng = np.random.default_rng(9900)
    pos, box = liquid(rng, 3, 130)
    l = float(box.min())
    pos[0] -= box[0]
    pos[1] += (rng.integers(-1, 2, pos[1].shape) * box[1]).astype(np.float32)
    pos[2] += (rng.integers(-3, 4, pos[2].shape) * box[2]).astype(np.float32)   # beyond the 27 images: fewer entries
    check(pos, box, 6, 1e-16 * l, 0.3 * l, (LOOSE,))


def test_coincident_atoms():
    """every atom has a twin at d = 0, outside the shell for r_lo = 0; the twins share their entries, counts and cluster"""
    rng = np.random.default_rng(10000)
    pos, box = liquid(rng, 2, 120)
    pos[:, 1::2] = pos[:, 0::2]
    (out, ref), = check(pos, box, 6, 0.0, 0.5 * float(box.min()), (LOOSE,))
    assert np.array_equal(out['nconn'][:, 0::2], out['nconn'][:, 1::2]) and np.array_equal(out['label'][:, 0::2], out['label'][:, 1::2])


def test_more_samples_than_one_launch_chunk():
    """4100 samples of 8 atoms: two launches, the second with four samples"""
    rng = np.random.default_rng(10100)
    pos, box = liquid(rng, 4100, 8, rho=0.8, spread=0.3)
    (out, ref), = check(pos, box, 6, 1e-16, 0.5 * float(box.min()), (LOOSE,))
    for s in (0, 4095, 4096, 4099):
        assert out['nconn'][s].sum() > 0
    assert out['nsolid'][4096:].sum() > 0


def test_scratch_cap_splits_the_batch():
    """4040 samples of 320 atoms at l = 12: a sample's moments take 320 * 26 * 8 = 66,560 B of the scratch, and 2^28 // 66,560 = 4033
    of them fit under the cap of 256 MiB: launch chunks of 4033 and 7 samples where the sample cap alone would give one.  The samples
    on both sides of the seam and the last one equal a call of their own, and four of them pass the restatement.  This checks the
    results across the seam, not that the batch is split, which cannot be seen through the entry point"""
    rng = np.random.default_rng(10200)
    pos, box = liquid(rng, 4040, 320)
    big = run(pos, box, 12, 1e-16, 1.5, *LOOSE)
    for sl in (slice(4028, 4038), slice(4039, 4040)):
        part = run(pos[sl], box[sl], 12, 1e-16, 1.5, *LOOSE)
        for k in NAMES:
            assert big[k][sl].tobytes() == part[k].tobytes(), (k, sl)
    pick = [0, 4032, 4033, 4039]
    (out, ref), = check(pos[pick], box[pick], 12, 1e-16, 1.5, (LOOSE,))
    for k in NAMES:
        assert big[k][pick].tobytes() == out[k].tobytes(), k
    assert out['nsolid'].min() > 0


# ---- NULL outputs, determinism, invariance
def test_null_outputs():
    rng = np.random.default_rng(10300)
    pos, box = liquid(rng, 3, 100)
    l = float(box.min())
    (full, ref), = check(pos, box, 6, 1e-16 * l, 0.4 * l, (LOOSE,))
    for k in NAMES:
        for want in ((k,), tuple(x for x in NAMES if x != k)):
            rc, msg, out = call(pos, box, 6, 1e-16 * l, 0.4 * l, *LOOSE, want=want)
            assert rc == 0, msg
            for x in NAMES:
                if x in want:
                    assert out[x].tobytes() == full[x].tobytes(), (want, x)
                else:
                    assert (out[x] == ISENT).all(), (want, x)


def test_two_calls_are_equal_bit_for_bit():
    rng = np.random.default_rng(10400)
    pos, box = liquid(rng, 6, 300)
    l = float(box.min())
    (a, ref), = check(pos, box, 6, 1e-16 * l, 0.5 * l, ((0.1, 60),))
    b = run(pos, box, 6, 1e-16 * l, 0.5 * l, 0.1, 60)
    for k in NAMES:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a['nsolid'].min() > 0 and (a['label'] == -1).any()


def test_permutation_of_the_atoms():
    """the permuted frame gives the permuted counts and the same partition into clusters"""
    rng = np.random.default_rng(10500)
    pos, box = noised_fcc(rng, 4, 0.2)
    (one, _), = check(pos[None], [box], 6, 1e-16, FIRST)
    p = rng.permutation(256)
    (two, _), = check(pos[p][None], [box], 6, 1e-16, FIRST)
    np.testing.assert_array_equal(two['nconn'][0], one['nconn'][0][p])
    assert one['nclus'][0] > 1
    assert {frozenset(p[list(c)].tolist()) for c in partition(two['label'][0])} == partition(one['label'][0])
    for k in ('nsolid', 'nclus', 'largest'):
        assert one[k][0] == two[k][0]


def test_bondorder_is_untouched_by_a_solid_call():
    L = B.load()
    rng = np.random.default_rng(10600)
    pos, box = liquid(rng, 5, 200)
    l = float(box.min())
    ls = np.array([4, 6], dtype=np.int32)

    def bondorder():
        q2, b2 = np.full((5, 200, 2), -1.0), np.full((5, 200, 2), -1.0)
        g2, nnb = np.full((5, 2), -1.0), np.full((5, 200), ISENT, dtype=np.int32)
        rc = L.nm_distr_bondorder(0, 5, 200, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), 1e-16 * l, 0.4 * l, 2,
                                  ls.ctypes.data_as(B.c_int_p), q2.ctypes.data_as(B.c_double_p), b2.ctypes.data_as(B.c_double_p),
                                  g2.ctypes.data_as(B.c_double_p), nnb.ctypes.data_as(B.c_int32_p))
        assert rc == 0, L.nm_distr_last_error().decode()
        return [x.tobytes() for x in (q2, b2, g2, nnb)]

    before = bondorder()
    out = run(pos, box, 6, 1e-16 * l, 0.4 * l, *LOOSE)
    assert bondorder() == before
    nnb = np.frombuffer(before[3], dtype=np.int32).reshape(5, 200)
    assert (out['nconn'] <= nnb).all() and out['nconn'].sum() > 0


def test_device_ordinal_out_of_range_and_empty_batch():
    rng = np.random.default_rng(10700)
    pos, box = liquid(rng, 2, 20)
    rc, msg, out = call(pos, box, 6, 1e-16, 0.5 * float(box.min()), *DEFAULTS, device=4096)
    assert rc == B.NM_ERR_ARG and msg.startswith('nm_distr_solid:')
    for k in NAMES:
        assert (out[k] == ISENT).all()
    rc, msg, out = call(pos[:0], box[:0], 6, 1e-16, 1.0, *DEFAULTS)
    assert rc == B.NM_OK, msg


# ---- the command line
def test_cli_writes_the_solid_files(tmp_path, monkeypatch):
    """distr.main with -so on a 2 x 2 grid of parsed frames (2 samples each, 256 atoms; displaced crystals and ideal gases in turn): the
    four files, with -sa the two per-atom files, with the documented shapes and dtypes and the values of solid(); the six other files
    are byte-identical to a run without -so, which writes none of them; the solid fraction is 1 for the crystals and 0 for the gases
    at the defaults, in the files and in the restatement"""
    rng = np.random.default_rng(10800)
    pn, tn, sn, n = 2, 2, 2, 256
    names = ('dni', 'r', 'rdf', 'dn', 'rv', 'cdf')
    new = ('soc', 'sof', 'sol', 'son')
    per_atom = ('sola', 'sona')
    ns = pn * tn * sn
    p, _ = fcc_integer(4)
    box = (6.4 + 0.02 * np.arange(ns)).astype(np.float32)
    pos = np.array([(((p / 8.0 + 0.004 * (rng.random(p.shape) - 0.5)) % 1.0) if s % 2 == 0 else rng.random(p.shape)) * b
                    for s, b in enumerate(box)]).astype(np.float32)
    natoms = np.full((pn, tn, sn), n, dtype=np.uint16)
    files = {}
    for sub, extra in (('plain', []), ('so', ['-so']), ('atoms', ['-so', '-sl', '4', '-st', '0.3', '-sx', '6', '-bc', '0.22', '-sa'])):
        d = tmp_path / sub
        d.mkdir()
        pref = str(d / 'd6.lj.fcc.lammps')
        np.save(pref + '.virial.trgt.npy', np.linspace(1, 8, pn, dtype=np.float32))
        np.save(pref + '.temp.trgt.npy', np.linspace(0.25, 2.5, tn, dtype=np.float32))
        np.save(pref + '.natoms.npy', natoms)
        np.save(pref + '.box.npy', box.reshape(pn, tn, sn))
        np.save(pref + '.pos.npy', pos.reshape(pn, tn, sn, n, 3))
        monkeypatch.chdir(d)
        distr.main(['-n', 'd6', '-e', 'LJ', '-sb', '32', '-cb', '6'] + extra)
        files[sub] = {f: open(os.path.join(d, f), 'rb').read() for f in sorted(os.listdir(d))}
    base = 'd6.lj.fcc.lammps.'
    assert not any(f.endswith(tuple('.%s.npy' % x for x in new + per_atom)) for f in files['plain'])
    assert sorted(set(files['so']) - set(files['plain'])) == [base + x + '.npy' for x in new]
    assert sorted(set(files['atoms']) - set(files['plain'])) == [base + x + '.npy' for x in sorted(new + per_atom)]
    for sub in ('so', 'atoms'):
        for nm in names:
            assert files[sub][base + nm + '.npy'] == files['plain'][base + nm + '.npy'], nm
    l = float(box.min())
    for sub, lv, cut, s_min, n_min in (('so', 6, 0.853553 / 4, 0.5, 8), ('atoms', 4, 0.22, 0.3, 6)):
        load = lambda x: np.load(str(tmp_path / sub / (base + x + '.npy')))
        nconn, label, nsolid, nclus, largest = distr.solid(natoms.reshape(-1), box, pos, lv, 1e-16 * l, cut * l, s_min, n_min)
        for a in (nconn, label):
            assert a.shape == (ns, n) and a.dtype == np.int32
        for a in (nsolid, nclus, largest):
            assert a.shape == (ns,) and a.dtype == np.int32
        sof, sol, soc, son = load('sof'), load('sol'), load('soc'), load('son')
        for a in (sof, sol, son):
            assert a.dtype == np.float32 and a.shape == (pn, tn, sn)
        assert soc.dtype == np.int32 and soc.shape == (pn, tn, sn)
        np.testing.assert_array_equal(sof.reshape(ns), (nsolid / np.float64(n)).astype(np.float32))
        np.testing.assert_array_equal(sol.reshape(ns), (largest / np.float64(n)).astype(np.float32))
        np.testing.assert_array_equal(soc.reshape(ns), nclus)
        np.testing.assert_array_equal(son.reshape(ns), nconn.mean(axis=1).astype(np.float32))
        if sub == 'atoms':
            sona, sola = load('sona'), load('sola')
            assert sona.dtype == np.int32 and sona.shape == (pn, tn, sn, n) and sola.dtype == np.int32 and sola.shape == (pn, tn, sn, n)
            np.testing.assert_array_equal(sona.reshape(ns, n), nconn)
            np.testing.assert_array_equal(sola.reshape(ns, n), label)
        else:
            ref = S.solid(pos, box, 6, 1e-16 * l, cut * l, 0.5, 8)
            assert S.undecided(ref, 0.5) == 0
            for k, got in zip(NAMES, (nconn, label, nsolid, nclus, largest)):
                np.testing.assert_array_equal(got, ref[k], err_msg=k)
            for d in (ref['nsolid'], sof.reshape(ns) * n):
                assert (d[0::2] == n).all() and (d[1::2] == 0).all()
            assert (sol.reshape(ns)[0::2] == 1.0).all() and (sof.reshape(ns)[1::2] == 0.0).all()
