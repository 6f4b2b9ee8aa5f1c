"""nm_distr_cna (include/nm_distr.h) on the GPU: the four integer outputs through the C-ABI against the numpy restatement
tests/cna_ref.py.  Every call runs on sentinel-filled outputs and is checked for complete writes and for EXACT equality of type, sig,
ntype and nsig; there is no tolerance anywhere, the definition is in integers and in stated float32 / float64 comparisons.

Covered, in both modes wherever both make sense: random liquids on both sides of 12 and 14 entries, of the block of centres (32), of
the wave (64) and of 256 atoms, at a first-shell radius and at half the box (more than 64 and more than 128 entries per centre: the
adaptive selection crosses scan batches); the known-answer lattices and clusters and a noised crystal with a mixture of types; the
fixed mode's list limit (32 entries against 33 or more); exact ties in d around the 12th and 14th entry (fcc, and simple cubic where
the tie-break decides the result); every neighbour in two images; a cutoff exactly on a neighbour and a neighbour-neighbour distance;
coincident atoms, an unwrapped frame, boxes that differ inside a batch; two launch chunks; NULL outputs; determinism; a permutation;
nm_distr_solid untouched by a call; a bad device ordinal and an empty batch; the command line."""
import os

import numpy as np
import pytest

import cna_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import distr

pytestmark = pytest.mark.gpu

ISENT = -77777777
NAMES = ('type', 'sig', 'ntype', 'nsig')
SHAPE = {'type': lambda m, n: (m, n), 'sig': lambda m, n: (m, n, 8), 'ntype': lambda m, n: (m, 5), 'nsig': lambda m, n: (m, 8)}
BOTH = (R.FIXED, R.ADAPTIVE)


def call(pos, box, r_lo, r_hi, mode, want=NAMES, device=0):
    """the raw ABI on sentinel-filled outputs, NULL for the outputs not in `want`; returns (rc, message, dict of the four arrays)"""
    L = B.load()
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    box = np.ascontiguousarray(box, dtype=np.float32).reshape(-1)
    ns, n = pos.shape[0], pos.shape[1]
    out = {k: np.full(SHAPE[k](ns, n), ISENT, dtype=np.int32) for k in NAMES}
    ptr = [out[k].ctypes.data_as(B.c_int32_p) if k in want else None for k in NAMES]
    rc = L.nm_distr_cna(device, ns, n, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), float(r_lo), float(r_hi),
                        int(mode), *ptr)
    return rc, (L.nm_distr_last_error().decode() if rc else ''), out


def run(pos, box, r_lo, r_hi, mode):
    rc, msg, out = call(pos, box, r_lo, r_hi, mode)
    assert rc == 0, msg
    for k in NAMES:
        assert (out[k] != ISENT).all(), k + ' is not written completely'
    return out


def check(pos, box, r_lo, r_hi, modes=BOTH):
    """the four outputs against the restatement for every mode, and every atom typed once; returns {mode: outputs}"""
    pos = np.asarray(pos, dtype=np.float32)
    box = np.asarray(box, dtype=np.float32).reshape(-1)
    res = {}
    for mode in modes:
        ref = dict(zip(NAMES, R.cna(pos, box, r_lo, r_hi, mode)))
        out = run(pos, box, r_lo, r_hi, mode)
        print('mode %d: types %s, columns %s' % (mode, ref['ntype'].sum(axis=0).tolist(), ref['nsig'].sum(axis=0).tolist()))
        for k in NAMES:
            np.testing.assert_array_equal(out[k], ref[k], err_msg='%s, mode %d' % (k, mode))
        assert (out['ntype'].sum(axis=1) == pos.shape[1]).all()
        res[mode] = out
    return res


def counts(pos, box, r_lo, r_hi):
    """entries per centre of one frame, by the restatement"""
    return np.array([len(R.entries(pos, box, c, r_lo, r_hi)[0]) for c in range(len(pos))])


def liquid(rng, ns, n, rho=0.9, spread=0.0):
    box = ((n / rho) ** (1 / 3) * (1.0 + spread * rng.random(ns))).astype(np.float32)
    pos = (rng.random((ns, n, 3)) * box[:, None, None]).astype(np.float32)
    return pos, box


def lattice_integer(base, cells):
    g = np.arange(cells) * 2
    pos = (np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 1, 3) + np.array(base)).reshape(-1, 3)
    return pos.astype(np.float32), np.float32(2 * cells)


def fcc_integer(cells):
    """fcc with a0 = 2 on integer coordinates: exact in float32; box 2 * cells"""
    return lattice_integer([[0, 0, 0], [0, 1, 1], [1, 0, 1], [1, 1, 0]], cells)


def bcc_integer(cells):
    return lattice_integer([[0, 0, 0], [1, 1, 1]], cells)


def cubic_integer(cells):
    g = np.arange(cells)
    return np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3).astype(np.float32), np.float32(cells)


def hcp_block(cells=3):
    """ideal-c/a hcp with neighbour distance 1, cells^3 four-atom orthorhombic cells in the middle of a box of 40"""
    e = [1.0, np.sqrt(3.0), np.sqrt(8.0 / 3.0)]
    base = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 5.0 / 6.0, 0.5], [0, 1.0 / 3.0, 0.5]]) * e
    g = np.stack(np.meshgrid(np.arange(cells), np.arange(cells), np.arange(cells), indexing='ij'), -1).reshape(-1, 1, 3) * e
    pos = (g + base).reshape(-1, 3)
    return (pos - pos.mean(axis=0) + 20.0).astype(np.float32), np.float32(40.0)


def icosahedron():
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = np.array([[0, s1, s2 * g] for s1 in (-1, 1) for s2 in (-1, 1)], dtype=np.float64)
    v = np.concatenate([v, np.roll(v, 1, axis=1), np.roll(v, 2, axis=1)]) / np.sqrt(1.0 + g * g)
    return (np.concatenate([np.zeros((1, 3)), v]) + 10.0).astype(np.float32), np.float32(20.0)


# ---- random liquids
@pytest.mark.parametrize('shell', ('first', 'half'))
@pytest.mark.parametrize('n', (1, 2, 11, 12, 13, 14, 15, 31, 32, 33, 63, 64, 65, 108, 256, 257, 500))
def test_liquid(n, shell):
    rng = np.random.default_rng(12000 + n)
    pos, box = liquid(rng, 2 if n >= 108 else 3, n)
    l = float(box.min())
    r_hi = min(1.5, 0.5 * l) if shell == 'first' else 0.5 * l
    res = check(pos, box, 1e-16 * l, r_hi)
    if shell == 'half' and n >= 256:
        nb = counts(pos[0], box[0], 1e-16 * l, r_hi)
        assert nb.min() > (128 if n == 500 else 64)                           # the selection crosses scan batches
        assert (res[R.FIXED]['sig'][0, :, R.COTHER] == nb).all()              # beyond the list limit: all entries are `other`
    if n == 1:
        assert not res[R.FIXED]['sig'].any() and not res[R.ADAPTIVE]['type'].any()


# ---- known answers
def test_perfect_fcc_and_bcc():
    pos, box = fcc_integer(3)
    a = check(pos[None], [box], 0.0, 0.5 * float(box), (R.ADAPTIVE,))[R.ADAPTIVE]
    f = check(pos[None], [box], 0.0, 0.853553 * 2.0, (R.FIXED,))[R.FIXED]
    for out in (a, f):
        assert (out['type'] == R.FCC).all() and (out['sig'][..., R.C421] == 12).all() and out['nsig'][0].sum() == 12 * 108
    pos, box = bcc_integer(3)
    a = check(pos[None], [box], 0.0, 0.5 * float(box), (R.ADAPTIVE,))[R.ADAPTIVE]
    f = check(pos[None], [box], 0.0, 1.207 * 2.0, (R.FIXED,))[R.FIXED]
    for out in (a, f):
        assert (out['type'] == R.BCC).all() and (out['sig'][..., R.C444] == 6).all() and (out['sig'][..., R.C666] == 8).all()


def test_hcp_block_and_icosahedron():
    pos, box = hcp_block()
    out = check(pos[None], [box], 0.0, 0.5 * float(box), (R.ADAPTIVE,))[R.ADAPTIVE]
    inner = int(np.argmin(((pos - pos.mean(axis=0)) ** 2).sum(axis=1)))
    assert out['type'][0, inner] == R.HCP and out['sig'][0, inner, R.C421] == 6 and out['sig'][0, inner, R.C422] == 6
    check(pos[None], [box], 0.0, 1.2, (R.FIXED,))
    pos, box = icosahedron()
    out = check(pos[None], [box], 0.0, 0.5 * float(box))[R.ADAPTIVE]
    assert out['type'][0].tolist() == [R.ICO] + 12 * [R.OTHER] and out['sig'][0, 0, R.C555] == 12


def test_noised_crystal_is_a_mixture():
    """fcc at 4^3 cells (a0 = 2) with Gaussian displacements of 0.11 per component: the restatement finds fcc atoms and others side by side"""
    rng = np.random.default_rng(12100)
    p, box = fcc_integer(4)
    pos = ((p + 0.11 * rng.normal(size=p.shape)) % box).astype(np.float32)
    ref = R.cna(pos[None], [box], 1e-16, 0.4 * float(box), R.ADAPTIVE)
    assert (ref[2][0] > 0).sum() >= 2 and 20 < ref[2][0, R.FCC] < 236
    check(pos[None], [box], 1e-16, 0.4 * float(box), (R.ADAPTIVE,))
    check(pos[None], [box], 1e-16, 1.7, (R.FIXED,))


# ---- limits of the lists
def test_fixed_mode_list_limit():
    """r_hi between the 32nd and the 33rd distance of centre 0: centres with exactly 32 entries get their graph, centres with 33 or
    more an all-`other` row that adds up to Nb"""
    rng = np.random.default_rng(12200)
    pos, box = liquid(rng, 1, 256)
    l = float(box[0])
    d = np.sort(R.entries(pos[0], box[0], 0, 1e-16, 0.5 * l)[0].astype(np.float64))
    r_hi = 0.5 * (d[31] + d[32])
    nb = counts(pos[0], box[0], 1e-16, r_hi)
    assert nb[0] == 32 and (nb == 32).sum() >= 2 and (nb >= 33).sum() >= 20 and (nb < 32).sum() >= 20
    out = check(pos, box, 1e-16, r_hi, (R.FIXED,))[R.FIXED]
    big = nb >= 33
    assert (out['sig'][0, big, :R.COTHER] == 0).all() and (out['sig'][0, big, R.COTHER] == nb[big]).all()
    assert (out['sig'][0].sum(axis=1) == nb).all() and out['sig'][0, nb == 32, :R.COTHER].any()


@pytest.mark.parametrize('lattice', ('fcc', 'cubic'))
def test_exact_ties_around_the_twelfth_and_fourteenth_entry(lattice):
    """perfect fcc: 12 equal distances, then 6 equal ones across the positions 12 to 17.  Simple cubic: 6, then 12 equal ones across
    the positions 6 to 17, so the 12 and the 14 vertices are cut out of a tie by the scan order alone, and the columns depend on it"""
    if lattice == 'fcc':
        pos, box = fcc_integer(3)
        r_hi = 0.5 * float(box)
    else:
        pos, box = cubic_integer(5)
        r_hi = 2.0
    d = np.sort(R.entries(pos, box, 0, 0.0, r_hi)[0])
    assert d[11] == d[12] if lattice == 'cubic' else d[12] == d[13]
    assert d[13] == d[14]
    out = check(pos[None], [box], 0.0, r_hi, (R.ADAPTIVE,))[R.ADAPTIVE]
    if lattice == 'cubic':
        assert (out['type'] == R.OTHER).all() and out['nsig'][0].sum() == 12 * len(pos)
    rng = np.random.default_rng(12300)
    p = rng.permutation(len(pos))                                             # another scan order, another cut through the tie
    check(pos[p][None], [box], 0.0, r_hi, (R.ADAPTIVE,))


# ---- lattices on integer coordinates
def test_every_neighbour_in_two_images():
    """a 2^3 grid of spacing 1 in a box of 2 with r_hi = box / 2: each of the six directions is reached in two images, 6 entries for
    3 atoms, and two entries of one atom are two vertices; 3^3 in a box of 3 has no such pairs"""
    pos, box = cubic_integer(2)
    out = check(pos[None], [box], 0.0, 1.0)[R.FIXED]
    assert (out['sig'][0].sum(axis=1) == 6).all()
    pos, box = cubic_integer(3)
    check(pos[None], [box], 0.0, 1.5)


def test_cutoff_exactly_on_a_distance():
    """fcc with a0 = 2 and r_hi = 2: the second neighbours sit on the closed end of the shell (18 entries), and so do the pairs of
    first neighbours 2 apart (bonded); just inside, 12 entries and the fcc graph"""
    pos, box = fcc_integer(3)
    on = check(pos[None], [box], 0.0, 2.0, (R.FIXED,))[R.FIXED]
    assert (on['sig'][0].sum(axis=1) == 18).all() and (on['type'] == R.OTHER).all()
    inside = check(pos[None], [box], 0.0, np.nextafter(2.0, 0.0), (R.FIXED,))[R.FIXED]
    assert (inside['type'] == R.FCC).all()
    # a first-neighbour pair sqrt 2 apart with the cutoff on the float32 value of sqrt 2 and just below it
    edge = float(np.sqrt(np.float32(2.0)))
    assert (check(pos[None], [box], 0.0, edge, (R.FIXED,))[R.FIXED]['type'] == R.FCC).all()
    assert not check(pos[None], [box], 0.0, np.nextafter(edge, 0.0), (R.FIXED,))[R.FIXED]['sig'].any()


# ---- batches and boxes
def test_boxes_that_differ_inside_one_batch():
    rng = np.random.default_rng(12400)
    pos, box = liquid(rng, 4, 120, spread=0.5)
    res = check(pos, box, 1e-16, 0.5 * float(box.min()))
    assert len({a.tobytes() for a in res[R.ADAPTIVE]['sig']}) == 4


def test_unwrapped_frame():
    rng = np.random.default_rng(12500)
    pos, box = liquid(rng, 3, 130)
    l = float(box.min())
    pos[0] -= box[0]
    pos[1] += (rng.integers(-1, 2, pos[1].shape) * box[1]).astype(np.float32)
    pos[2] += (rng.integers(-3, 4, pos[2].shape) * box[2]).astype(np.float32)   # beyond the 27 images: fewer entries
    check(pos, box, 1e-16 * l, 0.3 * l)
    check(pos, box, 1e-16 * l, 0.5 * l, (R.ADAPTIVE,))


def test_coincident_atoms():
    """every atom has a twin at d = 0, outside the shell for r_lo = 0; the twins' entries are coincident vertices, never bonded to
    each other, and the twins share their results"""
    rng = np.random.default_rng(12600)
    pos, box = liquid(rng, 2, 60)
    pos[:, 1::2] = pos[:, 0::2]
    l = float(box.min())
    for r_hi in (0.32 * l, 0.5 * l):
        res = check(pos, box, 0.0, r_hi)
        for out in res.values():
            assert np.array_equal(out['sig'][:, 0::2], out['sig'][:, 1::2]) and np.array_equal(out['type'][:, 0::2], out['type'][:, 1::2])


def test_more_samples_than_one_launch_chunk():
    """4097 samples of 2 atoms: two launches, the second with one sample"""
    rng = np.random.default_rng(12700)
    pos, box = liquid(rng, 4097, 2, rho=0.8, spread=0.3)
    res = check(pos, box, 1e-16, 0.5 * float(box.min()))
    assert res[R.FIXED]['nsig'][:4096].sum() > 0 and res[R.FIXED]['nsig'].shape == (4097, 8)


# ---- NULL outputs, determinism, invariance
@pytest.mark.parametrize('mode', BOTH)
def test_null_outputs(mode):
    rng = np.random.default_rng(12800)
    pos, box = liquid(rng, 3, 100)
    l = float(box.min())
    r_hi = (0.3 if mode == R.FIXED else 0.5) * l
    full = check(pos, box, 1e-16 * l, r_hi, (mode,))[mode]
    for k in NAMES:
        for want in ((k,), tuple(x for x in NAMES if x != k)):
            rc, msg, out = call(pos, box, 1e-16 * l, r_hi, mode, want=want)
            assert rc == 0, msg
            for x in NAMES:
                if x in want:
                    assert out[x].tobytes() == full[x].tobytes(), (want, x)
                else:
                    assert (out[x] == ISENT).all(), (want, x)


def test_two_calls_are_equal_bit_for_bit():
    rng = np.random.default_rng(12900)
    pos, box = liquid(rng, 6, 300)
    l = float(box.min())
    for mode, r_hi in ((R.FIXED, 0.27 * l), (R.ADAPTIVE, 0.5 * l)):
        a = run(pos, box, 1e-16 * l, r_hi, mode)
        b = run(pos, box, 1e-16 * l, r_hi, mode)
        for k in NAMES:
            assert a[k].tobytes() == b[k].tobytes(), k
        assert a['nsig'].min(axis=0).sum() > 0


def test_permutation_of_the_atoms():
    """the permuted frame gives the permuted per-atom results and the same sums"""
    rng = np.random.default_rng(13000)
    p0, box = fcc_integer(4)
    pos = ((p0 + 0.11 * rng.normal(size=p0.shape)) % box).astype(np.float32)
    p = rng.permutation(256)
    for mode, r_hi in ((R.FIXED, 1.7), (R.ADAPTIVE, 0.4 * float(box))):
        one = check(pos[None], [box], 1e-16, r_hi, (mode,))[mode]
        two = check(pos[p][None], [box], 1e-16, r_hi, (mode,))[mode]
        np.testing.assert_array_equal(two['type'][0], one['type'][0][p])
        np.testing.assert_array_equal(two['sig'][0], one['sig'][0][p])
        np.testing.assert_array_equal(two['ntype'], one['ntype'])
        np.testing.assert_array_equal(two['nsig'], one['nsig'])
        assert (one['ntype'][0] > 0).sum() >= 2


def test_solid_is_untouched_by_a_cna_call():
    rng = np.random.default_rng(13100)
    pos, box = liquid(rng, 5, 200)
    l = float(box.min())
    before = [x.tobytes() for x in distr.solid(np.full(5, 200), box, pos, 6, 1e-16 * l, 0.3 * l, 0.0, 1)]
    for mode in BOTH:
        run(pos, box, 1e-16 * l, 0.3 * l, mode)
    assert [x.tobytes() for x in distr.solid(np.full(5, 200), box, pos, 6, 1e-16 * l, 0.3 * l, 0.0, 1)] == before


def test_device_ordinal_out_of_range_and_empty_batch():
    rng = np.random.default_rng(13200)
    pos, box = liquid(rng, 2, 20)
    for mode in BOTH:
        rc, msg, out = call(pos, box, 1e-16, 0.5 * float(box.min()), mode, device=4096)
        assert rc == B.NM_ERR_ARG and msg.startswith('nm_distr_cna:')
        for k in NAMES:
            assert (out[k] == ISENT).all()
        rc, msg, out = call(pos[:0], box[:0], 1e-16, 1.0, mode)
        assert rc == B.NM_OK, msg


# ---- the command line
def test_cli_writes_the_cna_files(tmp_path, monkeypatch):
    """distr.main with -cn on a 2 x 2 grid of parsed frames (2 samples each, 108 atoms; displaced crystals and ideal gases in turn):
    the five files, with -ca the sixth, against the restatement; the six other files are byte-identical to a run without -cn, which
    writes none of the new ones"""
    rng = np.random.default_rng(13300)
    pn, tn, sn, n = 2, 2, 2, 108
    names = ('dni', 'r', 'rdf', 'dn', 'rv', 'cdf')
    new = ('cnb', 'cnf', 'cnh', 'cni', 'cns')
    ns = pn * tn * sn
    p, _ = fcc_integer(3)
    box = (4.8 + 0.02 * np.arange(ns)).astype(np.float32)
    pos = np.array([(((p / 6.0 + 0.004 * (rng.random(p.shape) - 0.5)) % 1.0) if s % 2 == 0 else rng.random(p.shape)) * b
                    for s, b in enumerate(box)]).astype(np.float32)
    files = {}
    for sub, extra in (('plain', []), ('cn', ['-cn']), ('fixed', ['-cn', '-cm', 'fixed', '-ca']), ('radius', ['-cn', '-cr', '0.3', '-ca'])):
        d = tmp_path / sub
        d.mkdir()
        pref = str(d / 'd7.lj.fcc.lammps')
        np.save(pref + '.virial.trgt.npy', np.linspace(1, 8, pn, dtype=np.float32))
        np.save(pref + '.temp.trgt.npy', np.linspace(0.25, 2.5, tn, dtype=np.float32))
        np.save(pref + '.natoms.npy', np.full((pn, tn, sn), n, dtype=np.uint16))
        np.save(pref + '.box.npy', box.reshape(pn, tn, sn))
        np.save(pref + '.pos.npy', pos.reshape(pn, tn, sn, n, 3))
        monkeypatch.chdir(d)
        distr.main(['-n', 'd7', '-e', 'LJ', '-sb', '32', '-cb', '6'] + extra)
        files[sub] = {f: open(os.path.join(d, f), 'rb').read() for f in sorted(os.listdir(d))}
    base = 'd7.lj.fcc.lammps.'
    assert not any('.cn' in f for f in files['plain'])
    assert sorted(set(files['cn']) - set(files['plain'])) == [base + x + '.npy' for x in new]
    for sub in ('fixed', 'radius'):
        assert sorted(set(files[sub]) - set(files['plain'])) == [base + x + '.npy' for x in new + ('cnta',)]
    for sub in ('cn', 'fixed', 'radius'):
        for nm in names:
            assert files[sub][base + nm + '.npy'] == files['plain'][base + nm + '.npy'], nm
    l = float(box.min())
    for sub, mode, cut in (('cn', R.ADAPTIVE, 1.3 / 3), ('fixed', R.FIXED, 0.853553 / 3), ('radius', R.ADAPTIVE, 0.3)):
        load = lambda x: np.load(str(tmp_path / sub / (base + x + '.npy')))
        typ, sig, ntype, nsig = R.cna(pos, box, 1e-16 * l, cut * l, mode)
        for x, t in (('cnf', R.FCC), ('cnh', R.HCP), ('cnb', R.BCC), ('cni', R.ICO)):
            a = load(x)
            assert a.dtype == np.float32 and a.shape == (pn, tn, sn)
            np.testing.assert_array_equal(a.reshape(ns), (ntype[:, t] / np.float64(n)).astype(np.float32))
        cnf = load('cnf').reshape(ns)
        assert (cnf[0::2] == 1.0).all() and (cnf[1::2] < 0.1).all()
        cns = load('cns')
        assert cns.dtype == np.float32 and cns.shape == (pn, tn, sn, 8)
        tot = nsig.sum(axis=1, dtype=np.int64)
        assert (tot > 0).all()
        np.testing.assert_array_equal(cns.reshape(ns, 8), (nsig / tot[:, None].astype(np.float64)).astype(np.float32))
        if sub != 'cn':
            ta = load('cnta')
            assert ta.dtype == np.int8 and ta.shape == (pn, tn, sn, n)
            np.testing.assert_array_equal(ta.reshape(ns, n), typ)
