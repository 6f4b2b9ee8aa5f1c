"""Common neighbour analysis (include/nm_distr.h, nm_distr_cna) without a GPU: the known answers of the numpy restatement
tests/cna_ref.py (perfect fcc, bcc, hcp and the 13-atom icosahedron; fcc under noise below the derived bound), every signature
column on hand-made neighbour sets, the C-ABI's declaration, export, binding and refusals (which precede the device check and leave
the outputs alone), and the command line's flags, automatic radii, file names and shapes (with distr.cna replaced by the
restatement)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cna_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import distr
from neuralmelting_amd import reweight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISENT = -77777777
NAMES = ('type', 'sig', 'ntype', 'nsig')
SHAPE = {'type': lambda m, n: (m, n), 'sig': lambda m, n: (m, n, 8), 'ntype': lambda m, n: (m, 5), 'nsig': lambda m, n: (m, 8)}


def row(**kw):
    """a sig row from column names: row(c421=12)"""
    out = np.zeros(8, dtype=np.int64)
    for k, v in kw.items():
        out[getattr(R, k.upper())] = v
    return out


def fcc_integer(cells):
    """fcc with a0 = 2 on integer coordinates: exact in float32; box 2 * cells"""
    base = np.array([[0, 0, 0], [0, 1, 1], [1, 0, 1], [1, 1, 0]])
    g = np.arange(cells) * 2
    pos = (np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 1, 3) + base).reshape(-1, 3)
    return pos.astype(np.float32), np.float32(2 * cells)


def bcc_integer(cells):
    """bcc with a0 = 2 on integer coordinates; box 2 * cells"""
    base = np.array([[0, 0, 0], [1, 1, 1]])
    g = np.arange(cells) * 2
    pos = (np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 1, 3) + base).reshape(-1, 3)
    return pos.astype(np.float32), np.float32(2 * cells)


def hcp_block(cells=3):
    """ideal-c/a hcp with neighbour distance 1, cells^3 four-atom orthorhombic cells (1, sqrt 3, sqrt(8/3)) in the middle of a box of
    40 (no periodic image within reach); returns pos, box and the atom nearest the block's middle"""
    a, b, c = 1.0, np.sqrt(3.0), np.sqrt(8.0 / 3.0)
    base = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 5.0 / 6.0, 0.5], [0, 1.0 / 3.0, 0.5]]) * [a, b, c]
    g = np.stack(np.meshgrid(np.arange(cells), np.arange(cells), np.arange(cells), indexing='ij'), -1).reshape(-1, 1, 3) * [a, b, c]
    pos = (g + base).reshape(-1, 3)
    mid = pos.mean(axis=0)
    inner = int(np.argmin(((pos - mid) ** 2).sum(axis=1)))
    return (pos - mid + 20.0).astype(np.float32), np.float32(40.0), inner


def icosahedron():
    """a centre and its 12 vertices at distance 1 in the middle of a box of 20"""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = np.array([[0, s1, s2 * g] for s1 in (-1, 1) for s2 in (-1, 1)], dtype=np.float64)
    v = np.concatenate([v, np.roll(v, 1, axis=1), np.roll(v, 2, axis=1)]) / np.sqrt(1.0 + g * g)
    return (np.concatenate([np.zeros((1, 3)), v]) + 10.0).astype(np.float32), np.float32(20.0)


# ---- known answers of the restatement
def test_perfect_fcc():
    pos, box = fcc_integer(3)
    typ, sig, ntype, nsig = R.cna(pos[None], [box], 0.0, 0.5 * float(box), R.ADAPTIVE)
    assert (typ == R.FCC).all() and (sig == row(c421=12)).all()
    assert ntype.tolist() == [[0, 108, 0, 0, 0]] and nsig[0].tolist() == (108 * row(c421=12)).tolist()
    typ, sig, ntype, nsig = R.cna(pos[None], [box], 0.0, 0.853553 * 2.0, R.FIXED)
    assert (typ == R.FCC).all() and (sig == row(c421=12)).all() and ntype.tolist() == [[0, 108, 0, 0, 0]]


def test_perfect_bcc():
    pos, box = bcc_integer(3)
    typ, sig, ntype, nsig = R.cna(pos[None], [box], 0.0, 0.5 * float(box), R.ADAPTIVE)
    assert (typ == R.BCC).all() and (sig == row(c444=6, c666=8)).all() and ntype.tolist() == [[0, 0, 0, 54, 0]]
    typ, sig, ntype, nsig = R.cna(pos[None], [box], 0.0, 1.207 * 2.0, R.FIXED)
    assert (typ == R.BCC).all() and (sig == row(c444=6, c666=8)).all() and nsig[0].tolist() == (54 * row(c444=6, c666=8)).tolist()


def test_atom_inside_an_hcp_block():
    pos, box, inner = hcp_block()
    t, sig = R.centre(pos, box, inner, 0.0, 0.5 * float(box), R.ADAPTIVE)
    assert t == R.HCP and sig.tolist() == row(c421=6, c422=6).tolist()


def test_icosahedron():
    pos, box = icosahedron()
    typ, sig, ntype, nsig = R.cna(pos[None], [box], 0.0, 0.5 * float(box), R.ADAPTIVE)
    assert typ[0, 0] == R.ICO and sig[0, 0].tolist() == row(c555=12).tolist()
    assert (typ[0, 1:] == R.OTHER).all() and ntype.tolist() == [[12, 0, 0, 0, 1]]


def test_fcc_stays_fcc_below_the_noise_bound():
    """every coordinate displaced uniformly by at most delta = 0.015 a: a pair distance moves by at most 2 sqrt 3 delta, a local
    cutoff by 1.2071 times that, and the 0.1464 a between the first shell and the cutoff need delta < 0.0191 a"""
    rng = np.random.default_rng(20121)
    pos, box = fcc_integer(3)
    pos = (pos + 2.0 * 0.015 * (2.0 * rng.random(pos.shape) - 1.0)).astype(np.float32)
    typ, sig, ntype, nsig = R.cna(pos[None], [box], 0.0, 0.5 * float(box), R.ADAPTIVE)
    assert (typ == R.FCC).all() and ntype.tolist() == [[0, 108, 0, 0, 0]]


# ---- every signature column on a hand-made neighbour set
def _ring(n, r=1.0):
    a = 2 * np.pi * np.arange(n) / n
    return np.stack([r * np.cos(a), r * np.sin(a), np.zeros(n)], -1)


def hand_made(name):
    """vertices float32 [n][3] and the cutoff 1: vertex 0 sits at (0, 0, 1) and has the signature `name`; the other vertices all lie
    within the cutoff of it (its common neighbours), on a ring around it or on hand-picked points, at distances from each other that
    put exactly the wanted bonds within the cutoff"""
    k = np.array([[0.0, 0.0, 1.0]])
    if name == '421':       # four common neighbours, two separate bonds
        cn = np.array([[0.6, 0.0, 1.0], [0.6, 0.5, 1.0], [-0.6, 0.0, 1.0], [-0.6, -0.5, 1.0]])
    elif name == '422':     # a chain of two bonds and a lone neighbour
        cn = np.array([[0.7, 0.0, 1.0], [0.0, 0.0, 0.3], [-0.7, 0.0, 1.0], [0.0, 0.9, 1.0]])
    elif name == '444':     # a ring of four
        cn = _ring(4, 0.6) + [0, 0, 1.0]
    elif name == '666':     # a ring of six
        cn = _ring(6, 0.9) + [0, 0, 1.0]
    elif name == '555':     # a ring of five
        cn = _ring(5, 0.8) + [0, 0, 1.0]
    elif name == '544':     # a chain of five
        cn = (_ring(6, 0.9) + [0, 0, 1.0])[:5]
    elif name == '433':     # a chain of four
        cn = (_ring(6, 0.9) + [0, 0, 1.0])[:4]
    elif name == 'star':    # a hub bonded to three leaves that are not bonded to each other: 3 bonds, no path longer than 2
        cn = np.array([[0.0, 0.0, 1.5], [0.8, 0.0, 1.5], [-0.4, 0.7, 1.5], [-0.4, -0.7, 1.5]])
    elif name == 'other':   # three common neighbours without a bond
        cn = _ring(3, 0.9) + [0, 0, 1.0]
    return np.concatenate([k, cn]).astype(np.float32), 1.0


@pytest.mark.parametrize('name, want', [('421', (4, 2, 1)), ('422', (4, 2, 2)), ('444', (4, 4, 4)), ('666', (6, 6, 6)), ('555', (5, 5, 5)),
                                        ('544', (5, 4, 4)), ('433', (4, 3, 3)), ('star', (4, 3, 3)), ('other', (3, 0, 0))])
def test_signature_columns(name, want):
    vecs, rc = hand_made(name)
    adj = R.adjacency(vecs, 0.0, rc)
    assert adj[0] == set(range(1, len(vecs)))                                   # every other vertex is a common neighbour
    got = R.signature(adj, 0)
    assert got == want
    col = R.column(got)
    assert col == (R.COTHER if name == 'other' else R.C433 if name == 'star' else getattr(R, 'C' + name))
    if name == 'star':                                                         # nlc is the component's bond count: the star is no path
        hub = [m for m in adj[0] if len(adj[m] & adj[0]) == 3]
        assert len(hub) == 1 and all(len(adj[m] & adj[0]) == 1 for m in adj[0] if m != hub[0])


def test_all_eight_columns_come_up():
    cols = {R.column(R.signature(R.adjacency(hand_made(n)[0], 0.0, 1.0), 0)) for n in ('421', '422', '444', '666', '555', '544', '433', 'other')}
    assert cols == set(range(8))


# ---- the C-ABI
def call(pos, box, r_lo=1e-16, r_hi=1.4, mode=1, device=0, natoms=None, ns=None, null=()):
    """the raw ABI on sentinel-filled outputs; returns (rc, message, dict of the four arrays)"""
    L = B.load()
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    box = np.ascontiguousarray(box, dtype=np.float32)
    m, n = pos.shape[0], pos.shape[1]
    out = {k: np.full(SHAPE[k](m, n), ISENT, dtype=np.int32) for k in NAMES}
    ptr = {k: out[k].ctypes.data_as(B.c_int32_p) for k in NAMES}
    ptr.update(pos=pos.ctypes.data_as(B.c_float_p), box=box.ctypes.data_as(B.c_float_p))
    for k in null:
        ptr[k] = None
    rc = L.nm_distr_cna(device, m if ns is None else ns, n if natoms is None else natoms, ptr['pos'], ptr['box'], float(r_lo),
                        float(r_hi), mode, *(ptr[k] for k in NAMES))
    return rc, (L.nm_distr_last_error().decode() if rc else ''), out


def test_symbol_is_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, 'include', 'nm_distr.h')).read()
    assert re.search(r'#define\s+NM_CNA_FIXED\s+0\b', txt) and re.search(r'#define\s+NM_CNA_ADAPTIVE\s+1\b', txt)
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    assert re.search(r'\bint\s+nm_distr_cna\s*\(', txt)
    assert 'nm_distr_cna' in B.DISTR_SYMBOLS
    assert hasattr(C.CDLL(B.LIB_PATH), 'nm_distr_cna')
    f = B.load().nm_distr_cna
    assert f.restype is C.c_int
    assert f.argtypes == [C.c_int, C.c_int, C.c_int, B.c_float_p, B.c_float_p, C.c_double, C.c_double, C.c_int,
                          B.c_int32_p, B.c_int32_p, B.c_int32_p, B.c_int32_p]
    assert distr.CNA_MODES == {'fixed': R.FIXED, 'adaptive': R.ADAPTIVE}


REFUSED = {
    'ns-1': dict(ns=-1), 'natoms0': dict(natoms=0), 'natoms4096': dict(natoms=4096), 'mode-1': dict(mode=-1), 'mode2': dict(mode=2),
    'r_lo-negative': dict(r_lo=-1e-3), 'r_lo-nan': dict(r_lo=float('nan')), 'r_hi-equal-r_lo': dict(r_lo=1.0, r_hi=1.0),
    'r_hi-nan': dict(r_hi=float('nan')), 'r_hi-beyond-half-the-smaller-box': dict(box=[3.0, 2.7], r_hi=1.4),
    'box-zero': dict(box=[3.0, 0.0]), 'box-negative': dict(box=[-3.0, 3.0]), 'box-nan': dict(box=[3.0, float('nan')]),
    'box-inf': dict(box=[float('inf'), 3.0]), 'null-pos': dict(null=('pos',)), 'null-box': dict(null=('box',)),
    'all-outputs-null': dict(null=NAMES), 'device-1': dict(device=-1),
}


@pytest.mark.parametrize('mode', (0, 1))
@pytest.mark.parametrize('case', sorted(REFUSED))
def test_refusals_precede_the_device_check(case, mode):
    kw = dict(REFUSED[case])
    kw.setdefault('mode', mode)
    rng = np.random.default_rng(5)
    box = np.array(kw.pop('box', [3.0, 3.0]), dtype=np.float32)
    pos = (rng.random((2, 8, 3)) * 2.9).astype(np.float32)
    rc, msg, out = call(pos, box, **kw)
    assert rc == B.NM_ERR_ARG
    assert msg.startswith('nm_distr_cna:')
    for k in NAMES:
        assert (out[k] == ISENT).all(), k


def test_valid_call_without_a_device_is_a_hip_error():
    """as nm_distr_bondorder: NM_ERR_HIP where that entry finds no device, also for an empty batch, and NM_OK where it finds one"""
    rng = np.random.default_rng(6)
    pos = (rng.random((2, 8, 3)) * 3.0).astype(np.float32)
    box = np.full(2, 3.0, dtype=np.float32)
    L = B.load()
    ls = np.array([6], dtype=np.int32)
    nnb = np.zeros((2, 8), dtype=np.int32)
    for ns in (2, 0):
        sibling = L.nm_distr_bondorder(0, ns, 8, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), 1e-16, 1.4, 1,
                                       ls.ctypes.data_as(B.c_int_p), None, None, None, nnb.ctypes.data_as(B.c_int32_p))
        assert sibling in (B.NM_OK, B.NM_ERR_HIP)
        for mode in (0, 1):
            rc, msg, out = call(pos, box, ns=ns, mode=mode)
            assert rc == sibling, msg
            if rc == B.NM_ERR_HIP:
                assert msg.startswith('nm_distr_cna:') and 'no HIP device' in msg
                for k in NAMES:
                    assert (out[k] == ISENT).all(), k
    if sibling == B.NM_ERR_HIP:
        with pytest.raises(RuntimeError, match='nm_distr_cna'):
            distr.cna(np.full(2, 8), box, pos, 1e-16, 1.4, 'adaptive')


# ---- the command line
def test_parse_args_cna_flags():
    a = distr.parse_args([])
    assert a.common_neighbours is False and a.cna_mode == 'adaptive' and a.cna_radius == 0.0 and a.cna_atoms is False
    a = distr.parse_args(['-cn'])
    assert a.common_neighbours is True and a.cna_mode == 'adaptive' and a.solid is False and a.bond_order is False
    a = distr.parse_args(['--common_neighbours', '--cna_mode', 'fixed', '--cna_radius', '0.25', '--cna_atoms'])
    assert a.common_neighbours is True and a.cna_mode == 'fixed' and a.cna_radius == 0.25 and a.cna_atoms is True
    a = distr.parse_args(['-cn', '-cm', 'adaptive', '-cr', '0.5', '-ca'])
    assert a.cna_mode == 'adaptive' and a.cna_radius == 0.5 and a.cna_atoms is True
    for bad in (['-cm', 'both'], ['-cm'], ['-cr', '0.51'], ['-cr', '-0.1'], ['-cr', 'nan'], ['-cr'], ['-cm', '1']):
        with pytest.raises(SystemExit):
            distr.parse_args(['-cn'] + bad)


def test_the_cna_flags_are_new():
    opts = [s for act in distr._parser()._actions for s in act.option_strings]
    assert len(opts) == len(set(opts))
    for f in ('-cn', '-cm', '-cr', '-ca', '--common_neighbours', '--cna_mode', '--cna_radius', '--cna_atoms'):
        assert f in opts


def test_help_says_that_the_automatic_radius_is_not_validated():
    txt = re.sub(r'\s+', ' ', distr._parser().format_help())
    at = txt.index('--cna_radius')
    assert 'has not yet been measured' in txt[at:txt.index('--cna_atoms')]


def test_automatic_radius():
    """-cr 0: fixed takes bond_cutoff's first fcc shell, adaptive min(0.5, 1.3 / SZ); an explicit value passes through"""
    for n, sz in ((32, 2), (108, 3), (256, 4), (500, 5), (2048, 8)):
        assert distr.cna_radius(0.0, n, 'fixed') == distr.bond_cutoff(0.0, n) == 0.853553 / sz
        assert distr.cna_radius(0.0, n, 'adaptive') == min(0.5, 1.3 / sz)
    assert distr.cna_radius(0.0, 32, 'adaptive') == 0.5 and distr.cna_radius(0.0, 4, 'adaptive') == 0.5
    assert distr.cna_radius(0.3, 4, 'fixed') == 0.3 and distr.cna_radius(0.5, 256, 'adaptive') == 0.5
    with pytest.raises(ValueError, match='-cr'):
        distr.cna_radius(0.0, 4, 'fixed')                                     # one cell: 0.85 of the box
    for bad in (0.6, -0.1):
        with pytest.raises(ValueError):
            distr.cna_radius(bad, 256, 'adaptive')


def write_run(d, name, pn, tn, sn, pos, box):
    pref = str(d / ('%s.lj.fcc.lammps' % name))
    n = pos.shape[-2]
    np.save(pref + '.virial.trgt.npy', np.linspace(1, 8, pn, dtype=np.float32))
    np.save(pref + '.temp.trgt.npy', np.linspace(0.25, 2.5, tn, dtype=np.float32))
    np.save(pref + '.natoms.npy', np.full((pn, tn, sn), n, dtype=np.uint16))
    np.save(pref + '.box.npy', np.asarray(box, dtype=np.float32).reshape(pn, tn, sn))
    np.save(pref + '.pos.npy', np.asarray(pos, dtype=np.float32).reshape(pn, tn, sn, n, 3))
    return pref


def test_main_refuses_a_bad_radius_before_any_file_is_written(tmp_path, monkeypatch):
    write_run(tmp_path, 'd1', 1, 1, 1, np.zeros((1, 4, 3)), [2.0])
    monkeypatch.chdir(tmp_path)
    before = sorted(os.listdir(tmp_path))
    for extra in (['-cn', '-cm', 'fixed'], ['-cn', '-cr', '0.7'], ['-cn', '-cm', 'neither']):
        with pytest.raises(SystemExit):                                       # 4 atoms: the automatic fixed cutoff is 0.85 of the box
            distr.main(['-n', 'd1', '-e', 'LJ'] + extra)
        assert sorted(os.listdir(tmp_path)) == before


def test_main_writes_the_cna_files(tmp_path, monkeypatch):
    """distr.main with -cn on a 2 x 1 grid of 2 samples each (32-atom fcc crystals and ideal gases in turn), the kernels replaced by
    the restatement (distr.cna) and by zeros (distr.histograms): the five files, with -ca the sixth, their shapes, dtypes and values,
    the radius each mode hands on, and that the reweighting stage's loader of -ob accepts the four fractions"""
    rng = np.random.default_rng(77)
    pn, tn, sn, n = 2, 1, 2, 32
    ns = pn * tn * sn
    p, _ = fcc_integer(2)
    box = (4.0 + 0.25 * np.arange(ns)).astype(np.float32)
    pos = np.array([(p / 4.0 if s % 2 == 0 else rng.random(p.shape)) * b for s, b in enumerate(box)]).astype(np.float32)
    seen = []

    def fake_cna(natoms, box_, pos_, r_lo, r_hi, mode, device=0):
        seen.append((r_lo, r_hi, mode))
        return R.cna(pos_, box_, r_lo, r_hi, distr.CNA_MODES[mode])

    def fake_histograms(natoms, box_, pos_, r, rv, device=0, **kw):
        return np.zeros((ns, len(r)), dtype=np.float32), np.zeros((ns,) + 3 * (rv.shape[1] - 1,), dtype=np.float32)

    monkeypatch.setattr(distr, 'cna', fake_cna)
    monkeypatch.setattr(distr, 'histograms', fake_histograms)
    l = float(box.min())
    base = 'd2.lj.fcc.lammps.'
    for sub, extra, mode, cut in (('a', ['-cn'], 'adaptive', 0.5), ('f', ['-cn', '-cm', 'fixed', '-ca'], 'fixed', 0.853553 / 2),
                                  ('r', ['-cn', '-cr', '0.45', '-ca'], 'adaptive', 0.45)):
        d = tmp_path / sub
        d.mkdir()
        write_run(d, 'd2', pn, tn, sn, pos, box)
        monkeypatch.chdir(d)
        before = set(os.listdir(d))
        distr.main(['-n', 'd2', '-e', 'LJ', '-sb', '8', '-cb', '2'] + extra)
        assert seen[-1] == (1e-16 * l, cut * l, mode)
        new = sorted(set(os.listdir(d)) - before)
        cna_files = ['cnb', 'cnf', 'cnh', 'cni', 'cns'] + (['cnta'] if '-ca' in extra else [])
        assert [f for f in new if '.cn' in f] == [base + x + '.npy' for x in cna_files]
        assert sorted(f for f in new if '.cn' not in f) == [base + x + '.npy' for x in ('cdf', 'dn', 'dni', 'r', 'rdf', 'rv')]
        typ, sig, ntype, nsig = R.cna(pos, box, 1e-16 * l, cut * l, distr.CNA_MODES[mode])
        load = lambda x: np.load(str(d / (base + x + '.npy')))
        for x, t in (('cnf', R.FCC), ('cnh', R.HCP), ('cnb', R.BCC), ('cni', R.ICO)):
            a = load(x)
            assert a.dtype == np.float32 and a.shape == (pn, tn, sn)
            np.testing.assert_array_equal(a.reshape(ns), (ntype[:, t] / np.float64(n)).astype(np.float32))
        assert (load('cnf').reshape(ns)[0::2] == 1.0).all() and (load('cnf').reshape(ns)[1::2] < 0.2).all()
        obs = reweight.load_observables(str(d / base[:-1]), ['cnf', 'cnh', 'cnb', 'cni'], (pn, tn, sn))   # reweight -ob takes them as they are
        assert len(obs) == 4 and np.array_equal(obs[0], load('cnf'))
        cns = load('cns')
        assert cns.dtype == np.float32 and cns.shape == (pn, tn, sn, 8)
        tot = nsig.sum(axis=1)
        for s in range(ns):
            want = nsig[s] / np.float64(tot[s]) if tot[s] else np.zeros(8)
            np.testing.assert_array_equal(cns.reshape(ns, 8)[s], want.astype(np.float32))
        assert (cns.reshape(ns, 8)[0::2, R.C421] == 1.0).all()
        if '-ca' in extra:
            ta = load('cnta')
            assert ta.dtype == np.int8 and ta.shape == (pn, tn, sn, n)
            np.testing.assert_array_equal(ta.reshape(ns, n), typ)


def test_shares_are_zero_where_nothing_is_counted(tmp_path, monkeypatch):
    """a sample without a counted entry (adaptive mode, fewer than 12 entries everywhere) has a zero row in .cns.npy, not a NaN"""
    pos = np.array([[[0.1, 0.1, 0.1], [1.0, 1.0, 1.0], [2.0, 2.5, 3.0], [3.0, 1.5, 0.5]]], dtype=np.float32)
    monkeypatch.setattr(distr, 'cna', lambda natoms, box_, pos_, r_lo, r_hi, mode, device=0: R.cna(pos_, box_, r_lo, r_hi, distr.CNA_MODES[mode]))
    monkeypatch.setattr(distr, 'histograms', lambda natoms, box_, pos_, r, rv, device=0, **kw: (
        np.zeros((1, len(r)), dtype=np.float32), np.zeros((1,) + 3 * (rv.shape[1] - 1,), dtype=np.float32)))
    write_run(tmp_path, 'd3', 1, 1, 1, pos, [4.0])
    monkeypatch.chdir(tmp_path)
    distr.main(['-n', 'd3', '-e', 'LJ', '-sb', '8', '-cb', '2', '-cn'])
    cns = np.load(str(tmp_path / 'd3.lj.fcc.lammps.cns.npy'))
    assert cns.shape == (1, 1, 1, 8) and not cns.any()
    assert not np.load(str(tmp_path / 'd3.lj.fcc.lammps.cnf.npy')).any()
