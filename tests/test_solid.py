"""Solid-like atoms and crystal clusters (include/nm_distr.h, nm_distr_solid) without a GPU: the long-double restatement
tests/solid_ref.py against an independent route (the bond values by the addition theorem, a Legendre polynomial of the angles between
bond pairs and no harmonics; the clusters by scipy.sparse.csgraph.connected_components), its known answers (the integer fcc lattice,
a lone pair, an atom without neighbours), the C-ABI's declaration, export, binding and refusals (which precede the device check and
leave the outputs alone), and the command line's flags."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.special as sp
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components

import bondorder_ref as R
import solid_ref as S
from neuralmelting_amd import _lib as B
from neuralmelting_amd import distr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISENT = -77777777
NAMES = ('nconn', 'label', 'nsolid', 'nclus', 'largest')


def fcc_integer(cells):
    base = np.array([[0, 0, 0], [0, 1, 1], [1, 0, 1], [1, 1, 0]])
    g = np.arange(cells) * 2
    pos = (np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 1, 3) + base).reshape(-1, 3)
    return pos.astype(np.float32), np.float32(2 * cells)


# ---- the restatement against an independent route
def legendre_route(pos, box, l, r_lo, r_hi):
    """per entry (centre-major) the bond value by the addition theorem: sum_m Y_lm(n) conj Y_lm(n') = (2l+1)/(4 pi) P_l(n . n'), so
    s(c, a) = sum_jk P_l(n_j . n'_k) / sqrt(sum_jj' P_l(n_j . n_j') sum_kk' P_l(n'_k . n'_k')) over the bonds j of c and k of a"""
    n = len(pos)
    ent = [R.neighbours(pos, box, c, r_lo, r_hi) for c in range(n)]
    un = [R.unit(e[0]).astype(np.float64) for e in ent]
    P = lambda x, y: sp.eval_legendre(l, np.clip(x @ y.T, -1.0, 1.0)).sum()
    self = [P(u, u) if len(u) else 0.0 for u in un]
    out = []
    for c in range(n):
        for a in ent[c][1]:
            d = np.sqrt(self[c] * self[a])
            out.append(P(un[c], un[a]) / d if d > 0 else 0.0)
    return np.array(out)


@pytest.mark.parametrize('l', (4, 6, 12))
def test_restatement_equals_legendre_and_csgraph(l):
    rng = np.random.default_rng(900 + l)
    n, box = 70, np.float32(5.5)
    pos = (rng.random((n, 3)) * box).astype(np.float32)
    ref = S.solid(pos[None], [box], l, 1e-16, 1.5, 0.3, 3)
    want = legendre_route(pos, box, l, 1e-16, 1.5)
    assert len(want) == len(ref['s']) > 300
    assert np.abs(ref['s'].astype(np.float64) - want).max() < 1e-12
    solid = ref['nconn'][0] >= 3
    assert 5 < solid.sum() < n                                                 # a non-trivial partition
    keep = solid[ref['centre']] & solid[ref['atom']]
    g = coo_matrix((np.ones(keep.sum()), (ref['centre'][keep], ref['atom'][keep])), shape=(n, n))
    ncomp, comp = connected_components(g, directed=False)
    label = np.full(n, -1)
    for k in np.unique(comp[solid]):
        label[solid & (comp == k)] = np.flatnonzero(solid & (comp == k)).min()
    np.testing.assert_array_equal(ref['label'][0], label)
    sizes = np.bincount(label[label >= 0])
    assert ref['nsolid'][0] == solid.sum() and ref['nclus'][0] == (sizes > 0).sum() and ref['largest'][0] == sizes.max()
    assert ref['nclus'][0] > 1


def test_decided_is_a_strict_margin():
    s = np.array([0.5, 0.5 + 1e-9, 0.5 - 1e-9, 0.9], dtype=R.LD)
    assert S.decided(s, np.full(4, 1e-10), 0.5).tolist() == [False, True, True, True]
    assert S.decided(s, np.full(4, 2e-9), 0.5).tolist() == [False, False, False, True]


# ---- known answers
def test_integer_fcc_is_one_cluster():
    pos, box = fcc_integer(4)
    ref = S.solid(pos[None], [box], 6, 0.0, 1.7, 0.5, 8)
    assert (ref['nnb'] == 12).all() and (ref['nconn'] == 12).all() and (ref['label'] == 0).all()
    assert ref['nsolid'][0] == 256 and ref['nclus'][0] == 1 and ref['largest'][0] == 256
    assert np.abs(ref['s'].astype(np.float64) - 1.0).max() < 1e-15 and S.undecided(ref, 0.5) == 0


def test_lone_pair():
    """two atoms with one bond each, opposite: q(a) = (-1)^l q(c), so s = 1 for even l and -1 for odd l"""
    pos = np.array([[[3.0, 3.5, 4.0], [3.6, 3.1, 4.7]]], dtype=np.float32)
    for l in range(1, 13):
        ref = S.solid(pos, [np.float32(10.0)], l, 0.0, 2.0, 0.5, 1)
        assert np.abs(ref['s'].astype(np.float64) - (-1.0) ** l).max() < 1e-15
        if l % 2 == 0:
            assert ref['nconn'].tolist() == [[1, 1]] and ref['label'].tolist() == [[0, 0]]
            assert (ref['nsolid'][0], ref['nclus'][0], ref['largest'][0]) == (2, 1, 2)
        else:
            assert ref['nconn'].tolist() == [[0, 0]] and ref['label'].tolist() == [[-1, -1]]
            assert (ref['nsolid'][0], ref['nclus'][0], ref['largest'][0]) == (0, 0, 0)


def test_an_atom_without_neighbours():
    pos = np.array([[[8.0, 8.0, 8.0], [3.0, 3.5, 4.0], [3.6, 3.1, 4.7]]], dtype=np.float32)
    ref = S.solid(pos, [np.float32(12.0)], 6, 0.0, 2.0, 0.5, 1)
    assert ref['nnb'].tolist() == [[0, 1, 1]] and ref['nconn'].tolist() == [[0, 1, 1]] and ref['label'].tolist() == [[-1, 1, 1]]
    assert (ref['nsolid'][0], ref['nclus'][0], ref['largest'][0]) == (2, 1, 2)
    assert S.undecided(ref, 0.5) == 0


# ---- the C-ABI
def call(pos, box, l=6, r_lo=1e-16, r_hi=1.4, s_min=0.5, n_min=8, device=0, natoms=None, ns=None, null=()):
    """the raw ABI on sentinel-filled outputs; returns (rc, message, dict of the five arrays)"""
    L = B.load()
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    box = np.ascontiguousarray(box, dtype=np.float32)
    m, n = pos.shape[0], pos.shape[1]
    out = {k: np.full((m, n) if k in ('nconn', 'label') else (m,), ISENT, dtype=np.int32) for k in NAMES}
    ptr = {k: out[k].ctypes.data_as(B.c_int32_p) for k in NAMES}
    ptr.update(pos=pos.ctypes.data_as(B.c_float_p), box=box.ctypes.data_as(B.c_float_p))
    for k in null:
        ptr[k] = None
    rc = L.nm_distr_solid(device, m if ns is None else ns, n if natoms is None else natoms, ptr['pos'], ptr['box'], float(r_lo),
                          float(r_hi), l, float(s_min), n_min, *(ptr[k] for k in NAMES))
    return rc, (L.nm_distr_last_error().decode() if rc else ''), out


def test_symbol_is_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, 'include', 'nm_distr.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    assert re.search(r'\bint\s+nm_distr_solid\s*\(', txt)
    assert 'nm_distr_solid' in B.DISTR_SYMBOLS
    assert hasattr(C.CDLL(B.LIB_PATH), 'nm_distr_solid')
    f = B.load().nm_distr_solid
    assert f.restype is C.c_int
    assert f.argtypes == [C.c_int, C.c_int, C.c_int, B.c_float_p, B.c_float_p, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int,
                          B.c_int32_p, B.c_int32_p, B.c_int32_p, B.c_int32_p, B.c_int32_p]


REFUSED = {
    'ns-1': dict(ns=-1), 'natoms0': dict(natoms=0), 'natoms4096': dict(natoms=4096), 'l0': dict(l=0), 'l13': dict(l=13), 'l-1': dict(l=-1),
    's_min-below': dict(s_min=-1.0000001), 's_min-one': dict(s_min=1.0), 's_min-nan': dict(s_min=float('nan')),
    's_min-inf': dict(s_min=float('inf')), 'n_min0': dict(n_min=0), 'n_min-negative': dict(n_min=-3),
    'r_lo-negative': dict(r_lo=-1e-3), 'r_lo-nan': dict(r_lo=float('nan')), 'r_hi-equal-r_lo': dict(r_lo=1.0, r_hi=1.0),
    'r_hi-nan': dict(r_hi=float('nan')), 'r_hi-beyond-half-the-smaller-box': dict(box=[3.0, 2.7], r_hi=1.4),
    'box-zero': dict(box=[3.0, 0.0]), 'box-negative': dict(box=[-3.0, 3.0]), 'box-nan': dict(box=[3.0, float('nan')]),
    'box-inf': dict(box=[float('inf'), 3.0]), 'null-pos': dict(null=('pos',)), 'null-box': dict(null=('box',)),
    'all-outputs-null': dict(null=NAMES), 'device-1': dict(device=-1),
}


@pytest.mark.parametrize('case', sorted(REFUSED))
def test_refusals_precede_the_device_check(case):
    kw = dict(REFUSED[case])
    rng = np.random.default_rng(5)
    box = np.array(kw.pop('box', [3.0, 3.0]), dtype=np.float32)
    pos = (rng.random((2, 8, 3)) * 2.9).astype(np.float32)
    rc, msg, out = call(pos, box, **kw)
    assert rc == B.NM_ERR_ARG
    assert msg.startswith('nm_distr_solid:')
    for k in NAMES:
        assert (out[k] == ISENT).all(), k


def test_the_ends_of_the_threshold_range_are_accepted():
    """s_min = -1 and the largest double below 1 pass the argument checks: what comes back is the device's answer"""
    rng = np.random.default_rng(6)
    pos = (rng.random((2, 8, 3)) * 3.0).astype(np.float32)
    box = np.full(2, 3.0, dtype=np.float32)
    for s_min in (-1.0, np.nextafter(1.0, 0.0)):
        rc, msg, out = call(pos, box, s_min=s_min, n_min=1)
        assert rc in (B.NM_OK, B.NM_ERR_HIP), msg


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
        rc, msg, out = call(pos, box, ns=ns)
        assert rc == sibling, msg
        if rc == B.NM_ERR_HIP:
            assert msg.startswith('nm_distr_solid:') and 'no HIP device' in msg
            for k in NAMES:
                assert (out[k] == ISENT).all(), k
    if sibling == B.NM_ERR_HIP:
        with pytest.raises(RuntimeError, match='nm_distr_solid'):
            distr.solid(np.full(2, 8), box, pos, 6, 1e-16, 1.4, 0.5, 8)


# ---- the command line
def test_parse_args_solid_flags():
    a = distr.parse_args([])
    assert a.solid is False and a.solid_l == 6 and a.solid_threshold == 0.5 and a.solid_connections == 8 and a.solid_atoms is False
    a = distr.parse_args(['-so'])
    assert a.solid is True and a.solid_atoms is False and a.bond_order is False
    a = distr.parse_args(['--solid', '--solid_l', '4', '--solid_threshold', '-1', '--solid_connections', '1', '--solid_atoms', '-bc', '0.25'])
    assert a.solid is True and a.solid_l == 4 and a.solid_threshold == -1.0 and a.solid_connections == 1 and a.solid_atoms is True
    assert a.bond_cutoff == 0.25
    a = distr.parse_args(['-so', '-sl', '12', '-st', '0.7', '-sx', '7', '-sa'])
    assert a.solid_l == 12 and a.solid_threshold == 0.7 and a.solid_connections == 7 and a.solid_atoms is True
    for bad in (['-sl', '0'], ['-sl', '13'], ['-sl', '2.5'], ['-sl'], ['-st', '1'], ['-st', '1.5'], ['-st', '-1.01'], ['-st', 'nan'],
                ['-st'], ['-sx', '0'], ['-sx', '-2'], ['-sx', '1.5'], ['-sx']):
        with pytest.raises(SystemExit):
            distr.parse_args(['-so'] + bad)


def test_help_says_that_the_defaults_are_not_validated():
    txt = re.sub(r'\s+', ' ', distr._parser().format_help())
    assert txt.count('has not been measured') == 2


def test_the_solid_flags_are_new():
    """none of the five flags is one of lammps_distr.py's or of the earlier additions"""
    opts = [s for act in distr._parser()._actions for s in act.option_strings]
    assert len(opts) == len(set(opts))
    for f in ('-so', '-sl', '-st', '-sx', '-sa', '--solid', '--solid_l', '--solid_threshold', '--solid_connections', '--solid_atoms'):
        assert f in opts


def test_main_refuses_bad_flags_and_a_bad_shell_before_any_file_is_written(tmp_path, monkeypatch):
    pref = str(tmp_path / 'd1.lj.fcc.lammps')
    np.save(pref + '.virial.trgt.npy', np.ones(1, dtype=np.float32))
    np.save(pref + '.temp.trgt.npy', np.ones(1, dtype=np.float32))
    np.save(pref + '.natoms.npy', np.full((1, 1, 1), 4, dtype=np.uint16))
    np.save(pref + '.box.npy', np.full((1, 1, 1), 2.0, dtype=np.float32))
    np.save(pref + '.pos.npy', np.zeros((1, 1, 1, 4, 3), dtype=np.float32))
    monkeypatch.chdir(tmp_path)
    before = sorted(os.listdir(tmp_path))
    for extra in (['-so'], ['-so', '-bc', '0.3', '-st', '1.0'], ['-so', '-bc', '0.3', '-sx', '0'], ['-so', '-bc', '0.3', '-sl', '13']):
        with pytest.raises(SystemExit):                                       # 4 atoms: the automatic shell is 0.85 of the box
            distr.main(['-n', 'd1', '-e', 'LJ'] + extra)
        assert sorted(os.listdir(tmp_path)) == before
