"""nm_distr_bondorder_w (include/nm_distr.h) on the GPU: the cubic forms w3, wbar3, W3 through the C-ABI against the long-double
restatement tests/bondorder_w_ref.py.  Every call runs on sentinel-filled outputs and is checked for three things: every output
written completely; q2, qbar2, Q2 and nnb equal, bit for bit, to what nm_distr_bondorder returns for the same arguments; and the
cubic forms within the derived bound bondorder_w_ref.tol (absolute, not doubled), which stays below 5e-13.

Covered: thermal frames on both sides of the wave's batch of 64 entries and of 256 atoms at a first-shell cutoff and at half the box;
the l sets (2,), (12,), (4, 6) and (2, .., 12); the perfect fcc and simple-cubic lattices and isolated hcp, icosahedral and bcc
clusters against Steinhardt's table; more than 256 neighbours per centre; a sparse frame; coincident atoms; every neighbour in two
images; boxes that differ inside a batch; two launch chunks; a batch that the scratch cap splits; NULL outputs; determinism; a
permutation; a device ordinal out of range and an empty batch; the command line."""
import os

import numpy as np
import pytest

import bondorder_ref as R
import bondorder_w_ref as W
from neuralmelting_amd import _lib as B
from neuralmelting_amd import distr
from test_bondorder import BCC14, HCP
from test_bondorder_gpu import call as call2
from test_bondorder_gpu import cubic_integer, fcc_integer, liquid
from test_bondorder_w import ICO, KNOWN

pytestmark = pytest.mark.gpu

SENT = -7.25e300
ISENT = -77777777
NAMES = ('w3', 'wbar3', 'W3', 'q2', 'qbar2', 'Q2', 'nnb')
OLD = ('q2', 'qbar2', 'Q2', 'nnb')
CUBIC = (('w3', 'q2', 'q'), ('wbar3', 'qbar2', 'qbar'), ('W3', 'Q2', 'Q'))


def call(pos, box, ls, r_lo, r_hi, want=NAMES, device=0):
    """the raw ABI on sentinel-filled outputs, NULL for the outputs not in `want`; returns (rc, message, dict of the seven arrays)"""
    L = B.load()
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    box = np.ascontiguousarray(box, dtype=np.float32).reshape(-1)
    ls = np.ascontiguousarray(ls, dtype=np.int32)
    ns, n, nl = pos.shape[0], pos.shape[1], len(ls)
    out = {k: np.full((ns, n, nl), SENT) for k in ('w3', 'wbar3', 'q2', 'qbar2')}
    out.update({k: np.full((ns, nl), SENT) for k in ('W3', 'Q2')})
    out['nnb'] = np.full((ns, n), ISENT, dtype=np.int32)
    ptr = [(out[k].ctypes.data_as(B.c_int32_p if k == 'nnb' else B.c_double_p) if k in want else None) for k in NAMES]
    rc = L.nm_distr_bondorder_w(device, ns, n, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), float(r_lo), float(r_hi),
                                nl, ls.ctypes.data_as(B.c_int_p), *ptr)
    return rc, (L.nm_distr_last_error().decode() if rc else ''), out


def run(pos, box, ls, r_lo, r_hi):
    """all seven outputs, written completely, the four of nm_distr_bondorder equal to that function's bit for bit"""
    rc, msg, out = call(pos, box, ls, r_lo, r_hi)
    assert rc == 0, msg
    for k in NAMES:
        assert (out[k] != (ISENT if k == 'nnb' else SENT)).all(), k + ' is not written completely'
    rc, msg, old = call2(pos, box, ls, r_lo, r_hi)
    assert rc == 0, msg
    for k in OLD:
        assert out[k].tobytes() == old[k].tobytes(), k + ' differs from nm_distr_bondorder'
    return out


def compare(out, ref, ls, natoms):
    """the cubic forms against the restatement within the header's bound"""
    m = int(ref['nnb'].max())
    for k, sq, which in CUBIC:
        for i, l in enumerate(ls):
            tol = W.tol(l, ref[sq][..., i].astype(np.float64), m, natoms, which)
            assert tol.max() <= 5e-13
            err = np.abs(out[k][..., i].astype(R.LD) - ref[k][..., i]).astype(np.float64)
            print('%s l = %d: max |error| %.3g, smallest allowed %.3g, largest error / allowed %.3g (%d neighbours at most)'
                  % (k, l, err.max(), tol.min(), (err / np.maximum(tol, 1e-300)).max(), m))
            assert (err <= tol).all(), (k, l)


def check(pos, box, ls, r_lo, r_hi):
    """returns (outputs, restatement)"""
    pos = np.asarray(pos, dtype=np.float32)
    box = np.asarray(box, dtype=np.float32).reshape(-1)
    out = run(pos, box, ls, r_lo, r_hi)
    ref = W.bond_order_w(pos, box, ls, r_lo, r_hi)
    np.testing.assert_array_equal(out['nnb'], ref['nnb'])
    compare(out, ref, ls, pos.shape[1])
    return out, ref


def hat(out, k, sq):
    return out[k] / np.maximum(out[sq], 1e-300) ** 1.5


# ---- thermal frames
def thermal(rng, ns, n):
    """an fcc lattice of at least n sites with Gaussian displacements, its first n atoms: (pos, box, the first shell's r_hi)"""
    cells = max(2, int(np.ceil((n / 4.0) ** (1.0 / 3.0))))
    p, box = fcc_integer(cells)
    pos = np.array([(p[:n] + 0.12 * rng.normal(size=(n, 3))) % box for _ in range(ns)]).astype(np.float32)
    return pos, np.full(ns, box, dtype=np.float32), min(1.7071, 0.5 * float(box))


@pytest.mark.parametrize('shell', ('first', 'half'))
@pytest.mark.parametrize('n', (1, 2, 63, 64, 65, 257))
def test_thermal_frames(n, shell):
    rng = np.random.default_rng(9000 + n)
    pos, box, first = thermal(rng, 2, n)
    l = float(box.min())
    if shell == 'first':
        out, ref = check(pos, box, (4, 6), 1e-16 * l, first)
    else:
        out, ref = check(pos, box, (2, 6, 12), 1e-16 * l, 0.5 * l)
        if n >= 63:
            assert ref['nnb'].max() > (64 if n == 257 else 20)
    if n == 1:
        assert not out['nnb'].any() and not out['w3'].any() and not out['wbar3'].any() and not out['W3'].any()
    if n >= 63 and shell == 'first':
        assert np.abs(out['w3']).max() > 1e-6 and np.abs(out['W3']).max() > 1e-9


@pytest.mark.parametrize('ls', ((2,), (12,), (4, 6), (2, 4, 6, 8, 10, 12)))
def test_l_sets(ls):
    rng = np.random.default_rng(9100 + len(ls) + ls[0])
    pos, box = liquid(rng, 2, 150)
    l = float(box.min())
    out, ref = check(pos, box, ls, 1e-16 * l, 0.5 * l)
    assert ref['nnb'].max() > 64


# ---- lattices and clusters
def test_fcc_lattice_known_answers():
    pos, box = fcc_integer(4)
    out, ref = check(pos[None], [box], (4, 6), 0.0, 1.7)
    assert (out['nnb'] == 12).all()
    for i, want in enumerate(KNOWN['fcc12'][1:]):
        for k, sq, _ in CUBIC:
            assert np.abs(hat(out, k, sq)[..., i] - want).max() < 1e-6, (k, i)


def test_simple_cubic_lattice_has_bonds_on_the_poles():
    pos, box = cubic_integer(4)
    out, ref = check(pos[None], [box], (4, 6), 0.0, 1.2)
    assert (out['nnb'] == 6).all()
    for i, want in enumerate(KNOWN['sc6'][1:]):
        for k, sq, _ in CUBIC:
            assert np.abs(hat(out, k, sq)[..., i] - want).max() < 1e-6, (k, i)


@pytest.mark.parametrize('name', ('hcp12', 'ico12', 'bcc14'))
def test_isolated_cluster(name):
    """the centre atom (index 0) and its shell in a box of 10: every shell atom within r_hi = 2.2 <= box / 2 of the centre"""
    vec = {'hcp12': HCP, 'ico12': ICO / np.linalg.norm(ICO[0]), 'bcc14': BCC14}[name]
    pos = np.concatenate([np.zeros((1, 3)), vec]) + 5.0
    out, ref = check(pos[None], [10.0], (4, 6), 0.0, 2.2)
    assert out['nnb'][0, 0] == len(vec) == len(pos) - 1
    _, w4, w6 = KNOWN[name]
    if w4 is None:
        # q4 of the icosahedron vanishes but for the float32 rounding of the positions (q4 about 1e-7): the cubic form itself against 0
        assert out['q2'][0, 0, 0] < 1e-12 and abs(out['w3'][0, 0, 0]) <= W.tol(4, out['q2'][0, 0, 0], len(vec), len(pos), 'q') + 1e-18
    else:
        assert abs(hat(out, 'w3', 'q2')[0, 0, 0] - w4) < 1e-6
    assert abs(hat(out, 'w3', 'q2')[0, 0, 1] - w6) < 1e-6


# ---- paths and edge cases
def test_more_than_256_neighbours():
    """300 atoms inside a ball of diameter < l/2: 299 neighbours per centre, five batches of the wave's list"""
    rng = np.random.default_rng(9200)
    n, L = 300, 10.0
    u = rng.normal(size=(n, 3))
    u *= (2.4 * rng.random(n) ** (1 / 3) / np.linalg.norm(u, axis=1))[:, None]
    out, ref = check((u + 5.0).astype(np.float32)[None], [np.float32(L)], (4, 6), 1e-16 * L, 0.5 * L)
    assert (ref['nnb'] == 299).all()


def test_sparse_frame_with_empty_and_single_neighbour_shells():
    rng = np.random.default_rng(7300)
    pos, box = liquid(rng, 2, 100, rho=0.05)
    out, ref = check(pos, box, (4, 6), 1e-16, 0.9)
    assert (ref['nnb'] == 0).any() and (ref['nnb'] == 1).any()
    lone = ref['nnb'] == 0
    assert not out['w3'][lone].any()
    # a single bond: q_lm = Y_lm(n) and q2 = 1, so w3 = (l l l; 0 0 0) for every direction (take n along z: only m = 0 is left)
    for i, l in enumerate((4, 6)):
        want = float(W.wigner3j(l, l, l, 0, 0, 0))
        assert np.abs(out['w3'][..., i][ref['nnb'] == 1] - want).max() < 1e-12


def test_coincident_atoms():
    rng = np.random.default_rng(9300)
    pos, box = liquid(rng, 2, 120)
    pos[:, 1::2] = pos[:, 0::2]
    out, ref = check(pos, box, (4, 6), 0.0, 0.5 * float(box.min()))
    assert out['w3'][:, 0::2].tobytes() == out['w3'][:, 1::2].tobytes() and out['wbar3'][:, 0::2].tobytes() == out['wbar3'][:, 1::2].tobytes()


def test_every_neighbour_in_two_images():
    pos, box = cubic_integer(2)
    out, ref = check(pos[None], [box], (4, 6), 0.0, 1.0)
    assert (out['nnb'] == 6).all()
    assert np.abs(hat(out, 'w3', 'q2')[..., 0] - KNOWN['sc6'][1]).max() < 1e-6


def test_boxes_that_differ_inside_one_batch():
    rng = np.random.default_rng(9400)
    pos, box = liquid(rng, 4, 120, spread=0.5)
    out, ref = check(pos, box, (4, 6), 1e-16, 0.5 * float(box.min()))
    assert len({a.tobytes() for a in out['W3']}) == 4


def test_more_samples_than_one_launch_chunk():
    """4096 + 1 samples of 5 atoms: two launches, the second with one sample.  run() compares the four old outputs of every sample with
    nm_distr_bondorder; the samples around the seam equal a call of their own bit for bit and pass the restatement"""
    rng = np.random.default_rng(9500)
    pos, box = liquid(rng, 4097, 5, rho=0.8, spread=0.3)
    r_hi = 0.5 * float(box.min())
    big = run(pos, box, (4, 6), 1e-16, r_hi)
    pick = [0, 4095, 4096]
    out, ref = check(pos[pick], box[pick], (4, 6), 1e-16, r_hi)
    for k in NAMES:
        assert big[k][pick].tobytes() == out[k].tobytes(), k
    assert all(out['nnb'][s].sum() > 0 for s in range(3))


def test_scratch_cap_splits_the_batch():
    """4096 samples of 86 atoms with l = 2 .. 12: nc2 = 2 * (3 + 5 + 7 + 9 + 11 + 13) = 96 doubles per atom, so a sample's moments take
    86 * 96 * 8 = 66,048 B of the scratch, and 2^28 // 66,048 = 4064 of them fit under the cap of 256 MiB: launch chunks of 4064 and 32
    samples.  As in tests/test_bondorder_gpu.py this checks the results across the seam, not that the batch is split"""
    ls = (2, 4, 6, 8, 10, 12)
    rng = np.random.default_rng(9600)
    pos, box = liquid(rng, 4096, 86)
    assert float(box.min()) > 3.0
    big = run(pos, box, ls, 1e-16, 1.5)
    for sl in (slice(4060, 4068), slice(4095, 4096)):
        rc, msg, part = call(pos[sl], box[sl], ls, 1e-16, 1.5)
        assert rc == 0, msg
        for k in NAMES:
            assert big[k][sl].tobytes() == part[k].tobytes(), (k, sl)
    pick = [0, 4063, 4064, 4095]
    out, ref = check(pos[pick], box[pick], ls, 1e-16, 1.5)
    for k in NAMES:
        assert big[k][pick].tobytes() == out[k].tobytes(), k


# ---- calling conventions
def test_null_outputs():
    rng = np.random.default_rng(9700)
    pos, box = liquid(rng, 3, 100)
    l = float(box.min())
    full, ref = check(pos, box, (4, 6), 1e-16 * l, 0.4 * l)
    for k in NAMES:
        for want in ((k,), tuple(x for x in NAMES if x != k)):
            rc, msg, out = call(pos, box, (4, 6), 1e-16 * l, 0.4 * l, want=want)
            assert rc == 0, msg
            for x in NAMES:
                if x in want:
                    assert out[x].tobytes() == full[x].tobytes(), (want, x)
                else:
                    assert (out[x] == (ISENT if x == 'nnb' else SENT)).all(), (want, x)


def test_two_calls_are_equal_bit_for_bit():
    rng = np.random.default_rng(9800)
    pos, box = liquid(rng, 6, 300)
    l = float(box.min())
    a = run(pos, box, (4, 6, 12), 1e-16 * l, 0.5 * l)
    b = run(pos, box, (4, 6, 12), 1e-16 * l, 0.5 * l)
    for k in NAMES:
        assert a[k].tobytes() == b[k].tobytes(), k
    assert np.abs(a['W3']).sum() > 0


def test_permutation_of_the_atoms():
    """both orders lie within the bound of the exact value, so they differ by at most twice the bound"""
    rng = np.random.default_rng(9900)
    pos, box = liquid(rng, 2, 200)
    l = float(box.min())
    one, ref = check(pos, box, (4, 6), 1e-16 * l, 0.4 * l)
    p = rng.permutation(200)
    two = run(pos[:, p], box, (4, 6), 1e-16 * l, 0.4 * l)
    np.testing.assert_array_equal(two['nnb'], one['nnb'][:, p])
    m = int(one['nnb'].max())
    for i, lv in enumerate((4, 6)):
        for k, sq, which in CUBIC[:2]:
            assert (np.abs(two[k][:, :, i] - one[k][:, p, i]) <= 2 * W.tol(lv, ref[sq][:, p, i].astype(np.float64), m, 200, which)).all()
        assert (np.abs(two['W3'][:, i] - one['W3'][:, i]) <= 2 * W.tol(lv, ref['Q2'][:, i].astype(np.float64), m, 200, 'Q')).all()


def test_device_ordinal_out_of_range_and_empty_batch():
    rng = np.random.default_rng(8400)
    pos, box = liquid(rng, 2, 20)
    rc, msg, out = call(pos, box, (4, 6), 1e-16, 0.5 * float(box.min()), device=4096)
    assert rc == B.NM_ERR_ARG and msg.startswith('nm_distr_bondorder_w:') and 'device' in msg
    assert all((out[k] == (ISENT if k == 'nnb' else SENT)).all() for k in NAMES)
    rc, msg, out = call(pos[:0], box[:0], (4, 6), 1e-16, 1.0)
    assert rc == B.NM_OK, msg


# ---- the command line
def test_cli_writes_the_w_files(tmp_path, monkeypatch):
    """distr.main on a 2 x 2 grid of parsed frames (2 samples each, 108 atoms) with -bo, with -bo -bw and with -bo -bw -ba: the new files
    with the documented shapes and dtypes and the values of bond_order_w(); every other file byte-identical with and without -bw"""
    rng = np.random.default_rng(8600)
    pn, tn, sn, n = 2, 2, 2, 108
    new = ('bow', 'bowb', 'bowg')
    per_atom = ('bowa', 'bowba')
    ns = pn * tn * sn
    p, _ = fcc_integer(3)
    box = (4.8 + 0.03 * np.arange(ns)).astype(np.float32)
    pos = np.array([((p / 6.0 + 0.02 * rng.normal(size=p.shape)) % 1.0) * b for b in box]).astype(np.float32)
    natoms = np.full((pn, tn, sn), n, dtype=np.uint16)
    files = {}
    for sub, extra in (('bo', ['-bo']), ('bw', ['-bo', '-bw']), ('boa', ['-bo', '-ba']), ('bwa', ['-bo', '--bond_w', '-ba'])):
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
    assert sorted(set(files['bw']) - set(files['bo'])) == [base + x + '.npy' for x in sorted(new)]
    assert sorted(set(files['bwa']) - set(files['boa'])) == [base + x + '.npy' for x in sorted(new + per_atom)]
    for with_w, without in (('bw', 'bo'), ('bwa', 'boa')):
        for f in files[without]:
            assert files[with_w][f] == files[without][f], f
    l = float(box.min())
    w, wb, wg, q, qb, qg, nb = distr.bond_order_w(natoms.reshape(-1), box, pos, [4, 6], 1e-16 * l, 0.853553 / 3 * l)
    q0, qb0, qg0, nb0 = distr.bond_order(natoms.reshape(-1), box, pos, [4, 6], 1e-16 * l, 0.853553 / 3 * l)
    assert q.tobytes() == q0.tobytes() and qb.tobytes() == qb0.tobytes() and qg.tobytes() == qg0.tobytes() and nb.tobytes() == nb0.tobytes()
    assert w.shape == wb.shape == (ns, n, 2) and wg.shape == (ns, 2) and np.abs(w).max() <= 1.0 and np.abs(wb).max() <= 1.0
    load = lambda sub, x: np.load(str(tmp_path / sub / (base + x + '.npy')))
    for sub in ('bw', 'bwa'):
        for x, want in (('bow', w.mean(axis=1)), ('bowb', wb.mean(axis=1)), ('bowg', wg)):
            a = load(sub, x)
            assert a.dtype == np.float32 and a.shape == load(sub, 'boq').shape == (pn, tn, sn, 2)
            np.testing.assert_array_equal(a.reshape(ns, 2), want.astype(np.float32))
    bowa, bowba = load('bwa', 'bowa'), load('bwa', 'bowba')
    assert bowa.dtype == np.float32 and bowa.shape == (pn, tn, sn, n, 2) and bowba.dtype == np.float32 and bowba.shape == bowa.shape
    np.testing.assert_array_equal(bowa.reshape(ns, n, 2), w.astype(np.float32))
    np.testing.assert_array_equal(bowba.reshape(ns, n, 2), wb.astype(np.float32))
    # .bow.npy is the float32 of the float64 mean, the per-atom file the float32 of each value (|w| <= 1: each off by at most 2^-25)
    for mean, atoms in ((load('bwa', 'bow'), bowa), (load('bwa', 'bowb'), bowba)):
        assert np.abs(mean - atoms.mean(axis=3, dtype=np.float64)).max() <= 2.0 ** -24
    assert load('bw', 'bow')[..., 0].mean() < -0.02                            # thermal fcc: w4 < 0
