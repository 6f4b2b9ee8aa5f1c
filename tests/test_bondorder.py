"""Steinhardt bond-order parameters (include/nm_distr.h, nm_distr_bondorder) without a GPU: the long-double restatement
tests/bondorder_ref.py against scipy's spherical harmonics and against the addition theorem (a route without harmonics), the
known answers of the fcc, hcp, bcc and simple-cubic shells, also rotated, the perfect lattice (qbar = q = Q) and the lone pair;
the kernel's route to the harmonics (normalised recurrence times powers of n_x + i n_y) in float64 against the restatement within
the derived per-bond bound; the C-ABI's declaration, export, binding and refusals (which precede the device check and leave the
outputs alone); the command line's flags and the automatic cutoff."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.special as sp

import bondorder_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import distr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -7.25e300
ISENT = -77777777

S2, S3 = np.sqrt(2.0), np.sqrt(3.0)
FCC = np.array([[1, 1, 0], [1, -1, 0], [-1, 1, 0], [-1, -1, 0], [1, 0, 1], [1, 0, -1], [-1, 0, 1], [-1, 0, -1], [0, 1, 1], [0, 1, -1],
                [0, -1, 1], [0, -1, -1]], dtype=np.float64)
_ring = np.array([[np.cos(k * np.pi / 3), np.sin(k * np.pi / 3), 0.0] for k in range(6)])
_cap = np.array([[np.cos(np.pi / 2 + k * 2 * np.pi / 3) / S3, np.sin(np.pi / 2 + k * 2 * np.pi / 3) / S3, np.sqrt(2.0 / 3.0)] for k in range(3)])
HCP = np.concatenate([_ring, _cap, _cap * np.array([1.0, 1.0, -1.0])])
BCC8 = np.array([[a, b, c] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)], dtype=np.float64)
SC = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)
BCC14 = np.concatenate([BCC8, 2 * SC])
KNOWN = {'fcc12': (FCC, 0.190941, 0.574524), 'hcp12': (HCP, 0.097222, 0.484762), 'bcc8': (BCC8, 0.509175, 0.628539),
         'bcc14': (BCC14, 0.036370, 0.510688), 'sc6': (SC, 0.763763, 0.353553)}


def rotation(rng):
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    return q * np.sign(np.linalg.det(q))


def directions(rng, n):
    """random unit vectors and the poles, the equator's axes and directions a rounding away from the poles"""
    v = rng.normal(size=(n, 3))
    special = np.array([[0, 0, 1], [0, 0, -1], [1, 0, 0], [0, -1, 0], [1e-9, 0, 1], [0, -1e-12, -1], [1e-160, 1e-170, 1]], dtype=np.float64)
    return np.concatenate([v, special])


def scipy_ylm(l, m, n):
    """scipy's Y_lm at the unit vectors n (float64): sph_harm_y(l, m, polar, azimuth), or the older sph_harm(m, l, azimuth, polar)"""
    polar = np.arctan2(np.hypot(n[:, 0], n[:, 1]), n[:, 2])                   # an arccos would lose the angle next to the poles
    az = np.arctan2(n[:, 1], n[:, 0])
    if hasattr(sp, 'sph_harm_y'):
        return sp.sph_harm_y(l, m, polar, az)
    return sp.sph_harm(m, l, az, polar)


def kernel_route(v, l):
    """the kernel's arithmetic in float64 (neuralmelting_amd/csrc/nm_distr.h): n = v * (1 / sqrt(|v|^2)), N_l^m by the normalised
    recurrence from constants rounded once from long double, times (n_x + i n_y)^m; returns (re, im) float64 [M][l+1]"""
    v = np.asarray(v, dtype=np.float64)
    rinv = 1.0 / np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])
    nx, ny, nz = v[:, 0] * rinv, v[:, 1] * rinv, v[:, 2] * rinv
    re = np.zeros((len(v), l + 1))
    im = np.zeros((len(v), l + 1))
    c = np.sqrt(1 / (4 * R.PI))
    pr, pi = np.ones(len(v)), np.zeros(len(v))
    for m in range(l + 1):
        if m > 0:
            c = -c * np.sqrt(R.LD(2 * m + 1) / R.LD(2 * m))
            pr, pi = pr * nx - pi * ny, pr * ny + pi * nx
        p0, p1 = np.full(len(v), float(c)), np.zeros(len(v))
        for k in range(m + 1, l + 1):
            a = float(np.sqrt(R.LD(4 * k * k - 1) / R.LD(k * k - m * m)))
            b = float(np.sqrt(R.LD((k - 1) * (k - 1) - m * m) / R.LD(4 * (k - 1) * (k - 1) - 1)))
            p0, p1 = a * (nz * p0 - b * p1), p0
        re[:, m], im[:, m] = p0 * pr, p0 * pi
    return re, im


# ---- the restatement's harmonics
@pytest.mark.parametrize('l', range(1, 13))
def test_restatement_harmonics_equal_scipy(l):
    rng = np.random.default_rng(100 + l)
    n = directions(rng, 200)
    n = n / np.linalg.norm(n, axis=1)[:, None]
    re, im = R.harmonics(R.unit(n), l)
    for m in range(l + 1):
        want = scipy_ylm(l, m, n)
        err = np.abs((re[:, m].astype(np.float64) + 1j * im[:, m].astype(np.float64)) - want).max()
        assert err < 2e-13, (l, m, err)          # scipy's own float64 error and that of the two angles
    # the poles exactly: Y_l0 = +-sqrt((2l+1)/4 pi), every m > 0 vanishes
    pre, pim = R.harmonics(np.array([[0, 0, 1], [0, 0, -1]], dtype=R.LD), l)
    top = np.sqrt((2 * l + 1) / (4 * np.pi))
    assert abs(float(pre[0, 0]) - top) < 1e-15 and abs(float(pre[1, 0]) - (-1) ** l * top) < 1e-15
    assert not pre[:, 1:].any() and not pim.any()


@pytest.mark.parametrize('l', range(1, 13))
def test_kernel_route_is_within_the_per_bond_bound(l):
    """the empirical check of the derived bound e(l), not a test of the HIP code: kernel_route is a host transcription of the
    kernel's arithmetic (the normalised recurrence times the powers of n_x + i n_y, in float64 from float32 components of any
    length); its error in the vector (Y_lm)_m relative to the vector's norm, against the restatement, stays below e(l), bonds on and
    next to the z axis included.  The kernel itself is compared with the restatement in tests/test_bondorder_gpu.py."""
    rng = np.random.default_rng(200 + l)
    v = (directions(rng, 4000) * rng.uniform(0.3, 9.0, size=(4007, 1))).astype(np.float32)
    v[-1] = (1e-30, -1e-30, 3.0)
    re, im = kernel_route(v, l)
    wre, wim = R.harmonics(R.unit(v), l)
    d = (re - wre) ** 2 + (im - wim) ** 2
    err = np.sqrt((d[:, 0] + 2 * d[:, 1:].sum(axis=1)).astype(np.float64)) / np.sqrt((2 * l + 1) / (4 * np.pi))
    print('l = %2d: largest normalised error of a bond %.3g, bound e(l) = %.3g' % (l, err.max(), R.e_bond(l)))
    assert err.max() <= R.e_bond(l)
    assert 4 * max(R.bounds(l, 529, 4095)) <= 1e-12                          # twice 2 e, at the most neighbours the GPU tests reach


# ---- the addition theorem: q2 = (1/Nb^2) sum_jk P_l(n_j . n_k), no harmonics
def addition_theorem(vectors, l):
    n = R.unit(vectors).astype(np.float64)
    return sp.eval_legendre(l, np.clip(n @ n.T, -1.0, 1.0)).sum() / len(n) ** 2


@pytest.mark.parametrize('l', range(1, 13))
def test_restatement_equals_the_addition_theorem(l):
    rng = np.random.default_rng(300 + l)
    for vec in (FCC, HCP, BCC8, BCC14, SC, rng.normal(size=(37, 3)), rng.normal(size=(2, 3))):
        got = float(R.shell_q2(vec, l))
        assert abs(got - addition_theorem(vec, l)) < 3e-14, l


# ---- known answers
@pytest.mark.parametrize('name', sorted(KNOWN))
def test_known_shells(name):
    vec, q4, q6 = KNOWN[name]
    rng = np.random.default_rng(400)
    for rot in (np.eye(3), rotation(rng), rotation(rng)):
        w = vec @ rot.T
        assert abs(float(np.sqrt(R.shell_q2(w, 4))) - q4) < 1e-6
        assert abs(float(np.sqrt(R.shell_q2(w, 6))) - q6) < 1e-6
        assert abs(float(R.shell_q2(w, 2))) < 1e-30                          # q2 vanishes on all of these shells


def test_hcp_shell_is_a_close_packing():
    d = np.linalg.norm(HCP[:, None] - HCP[None], axis=2)
    assert np.allclose(np.linalg.norm(HCP, axis=1), 1.0) and np.isclose(d[d > 1e-9].min(), 1.0)


def fcc_integer(cells):
    base = np.array([[0, 0, 0], [0, 1, 1], [1, 0, 1], [1, 1, 0]])
    g = np.arange(cells) * 2
    pos = (np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 1, 3) + base).reshape(-1, 3)
    return pos.astype(np.float32), np.float32(2 * cells)


def test_perfect_lattice_has_qbar_equal_q_equal_Q():
    pos, box = fcc_integer(2)
    q2, b2, g2, nnb = R.bond_order2(pos[None], [box], (2, 4, 6), 0.0, 1.7)
    assert (nnb == 12).all()
    for i, want in enumerate((0.0, 0.190941, 0.574524)):
        for x in (q2[0, :, i], b2[0, :, i], g2[0, i:i + 1]):
            assert np.abs(np.sqrt(np.abs(x)).astype(np.float64) - want).max() < 1e-6
        assert np.abs(q2[0, :, i] - b2[0, :, i]).max() < 1e-18 and np.abs(q2[0, :, i] - g2[0, i]).max() < 1e-18


def test_lone_pair():
    """two atoms: q_l = 1 for every l; the two bonds are opposite, so qbar_l = Q_l = 1 for even l and 0 for odd l"""
    rng = np.random.default_rng(500)
    pos = np.array([[[3.0, 3.5, 4.0], [3.0, 3.5, 4.0]]], dtype=np.float32)
    pos[0, 1] += rotation(rng)[0].astype(np.float32)
    ls = tuple(range(1, 13))
    q2, b2, g2, nnb = R.bond_order2(pos, [np.float32(10.0)], ls, 0.0, 2.0)
    assert (nnb == 1).all()
    even = np.array([1.0 - l % 2 for l in ls])
    assert np.abs(q2 - 1.0).max() < 1e-17 and np.abs(b2 - even).max() < 1e-17 and np.abs(g2 - even).max() < 1e-17


def test_an_atom_in_two_images_counts_twice():
    """a simple-cubic grid of spacing 1 in a box of 2 with r_hi = 1: each of the 6 neighbour directions is reached in two images"""
    g = np.arange(2)
    pos = np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3).astype(np.float32)
    q2, b2, g2, nnb = R.bond_order2(pos[None], [np.float32(2.0)], (4, 6), 0.0, 1.0)
    assert (nnb == 6).all()
    assert np.abs(np.sqrt(q2[0, :, 0]).astype(np.float64) - 0.763763).max() < 1e-6


# ---- the C-ABI
def call(pos, box, ls, r_lo=1e-16, r_hi=1.4, device=0, natoms=None, ns=None, nl=None, null=()):
    """the raw ABI on sentinel-filled outputs; returns (rc, message, q2, qbar2, Q2, nnb)"""
    L = B.load()
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    box = np.ascontiguousarray(box, dtype=np.float32)
    ls = np.ascontiguousarray(ls, dtype=np.int32)
    n, w = pos.shape[1], max(len(ls), 1)
    q2 = np.full((pos.shape[0], n, w), SENT)
    b2 = np.full((pos.shape[0], n, w), SENT)
    g2 = np.full((pos.shape[0], w), SENT)
    nnb = np.full((pos.shape[0], n), ISENT, dtype=np.int32)
    ptr = dict(pos=pos.ctypes.data_as(B.c_float_p), box=box.ctypes.data_as(B.c_float_p), ls=ls.ctypes.data_as(B.c_int_p),
               q2=q2.ctypes.data_as(B.c_double_p), qbar2=b2.ctypes.data_as(B.c_double_p), Q2=g2.ctypes.data_as(B.c_double_p),
               nnb=nnb.ctypes.data_as(B.c_int32_p))
    for k in null:
        ptr[k] = None
    rc = L.nm_distr_bondorder(device, pos.shape[0] if ns is None else ns, n if natoms is None else natoms, ptr['pos'], ptr['box'],
                              float(r_lo), float(r_hi), len(ls) if nl is None else nl, ptr['ls'], ptr['q2'], ptr['qbar2'], ptr['Q2'],
                              ptr['nnb'])
    return rc, (L.nm_distr_last_error().decode() if rc else ''), q2, b2, g2, nnb


def test_symbol_is_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, 'include', 'nm_distr.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    assert re.search(r'\bint\s+nm_distr_bondorder\s*\(', txt)
    assert 'nm_distr_bondorder' in B.DISTR_SYMBOLS
    assert hasattr(C.CDLL(B.LIB_PATH), 'nm_distr_bondorder')
    f = B.load().nm_distr_bondorder
    assert f.restype is C.c_int
    assert f.argtypes == [C.c_int, C.c_int, C.c_int, B.c_float_p, B.c_float_p, C.c_double, C.c_double, C.c_int, B.c_int_p,
                          B.c_double_p, B.c_double_p, B.c_double_p, B.c_int32_p]


REFUSED = {
    'ns-1': dict(ns=-1), 'natoms0': dict(natoms=0), 'natoms4096': dict(natoms=4096), 'nl0': dict(nl=0), 'nl7': dict(ls=(1, 2, 3, 4, 5, 6, 7)),
    'l0': dict(ls=(0, 4)), 'l13': dict(ls=(6, 13)), 'l-repeated': dict(ls=(4, 4)), 'l-decreasing': dict(ls=(6, 4)),
    'r_lo-negative': dict(r_lo=-1e-3), 'r_lo-nan': dict(r_lo=float('nan')), 'r_hi-equal-r_lo': dict(r_lo=1.0, r_hi=1.0),
    'r_hi-nan': dict(r_hi=float('nan')), 'r_hi-beyond-half-the-smaller-box': dict(box=[3.0, 2.7], r_hi=1.4),
    'box-zero': dict(box=[3.0, 0.0]), 'box-negative': dict(box=[-3.0, 3.0]), 'box-nan': dict(box=[3.0, float('nan')]),
    'box-inf': dict(box=[float('inf'), 3.0]), 'null-pos': dict(null=('pos',)), 'null-box': dict(null=('box',)), 'null-ls': dict(null=('ls',)),
    'all-outputs-null': dict(null=('q2', 'qbar2', 'Q2', 'nnb')), 'device-1': dict(device=-1),
}


@pytest.mark.parametrize('case', sorted(REFUSED))
def test_refusals_precede_the_device_check(case):
    kw = dict(REFUSED[case])
    rng = np.random.default_rng(5)
    box = np.array(kw.pop('box', [3.0, 3.0]), dtype=np.float32)
    pos = (rng.random((2, 8, 3)) * 2.9).astype(np.float32)
    rc, msg, q2, b2, g2, nnb = call(pos, box, kw.pop('ls', (4, 6)), **kw)
    assert rc == B.NM_ERR_ARG
    assert msg.startswith('nm_distr_bondorder:')
    assert (q2 == SENT).all() and (b2 == SENT).all() and (g2 == SENT).all() and (nnb == ISENT).all()


def test_valid_call_without_a_device_is_a_hip_error():
    """as nm_distr_sfactor: NM_ERR_HIP where that entry finds no device, also for an empty batch, and NM_OK where it finds one"""
    rng = np.random.default_rng(6)
    pos = (rng.random((2, 8, 3)) * 3.0).astype(np.float32)
    box = np.full(2, 3.0, dtype=np.float32)
    z = np.zeros((2, 5))
    L = B.load()
    sibling = L.nm_distr_sfactor(0, 2, 8, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), 2,
                                 z.ctypes.data_as(B.c_double_p), None)
    assert sibling in (B.NM_OK, B.NM_ERR_HIP)
    for ns in (2, 0):
        rc, msg, q2, b2, g2, nnb = call(pos, box, (4, 6), ns=ns)
        assert rc == sibling, msg
        if rc == B.NM_ERR_HIP:
            assert msg.startswith('nm_distr_bondorder:') and 'no HIP device' in msg
            assert (q2 == SENT).all() and (b2 == SENT).all() and (g2 == SENT).all() and (nnb == ISENT).all()
    if sibling == B.NM_ERR_HIP:
        with pytest.raises(RuntimeError, match='nm_distr_bondorder'):
            distr.bond_order(np.full(2, 8), box, pos, (4, 6), 1e-16, 1.4)


# ---- the command line
def test_parse_args_bond_order_flags():
    a = distr.parse_args([])
    assert a.bond_order is False and a.bond_l == [4, 6] and a.bond_cutoff == 0.0 and a.bond_atoms is False
    a = distr.parse_args(['-bo'])
    assert a.bond_order is True and a.bond_l == [4, 6] and a.bond_atoms is False
    a = distr.parse_args(['--bond_order', '--bond_l', '6', '2', '12', '--bond_cutoff', '0.25', '--bond_atoms'])
    assert a.bond_order is True and a.bond_l == [2, 6, 12] and a.bond_cutoff == 0.25 and a.bond_atoms is True
    a = distr.parse_args(['-bo', '-bl', '1', '-bc', '0.5', '-ba'])
    assert a.bond_l == [1] and a.bond_cutoff == 0.5 and a.bond_atoms is True
    for bad in (['-bc', '0.51'], ['-bc', '-0.1'], ['-bc', 'nan'], ['-bl', '0'], ['-bl', '13'], ['-bl', '4', '4'], ['-bl', '2.5'],
                ['-bl', '1', '2', '3', '4', '5', '6', '7'], ['-bl']):
        with pytest.raises(SystemExit):
            distr.parse_args(['-bo'] + bad)


def test_automatic_cutoff_is_the_first_fcc_shell():
    for cells in (2, 3, 4, 5, 8):
        cut = distr.bond_cutoff(0.0, 4 * cells ** 3)
        assert cut == 0.853553 / cells
        # midway between the first and second neighbour distances, a0 / sqrt(2) and a0, of cells cells per box edge
        assert abs(cut - 0.5 * (1 / S2 + 1.0) / cells) < 1e-6 / cells
    assert distr.bond_cutoff(0.0, 500) == 0.853553 / 5 and distr.bond_cutoff(0.3, 500) == 0.3
    for natoms in (1, 4, 13):                                                 # one cell per edge: 0.85 of the box, beyond 0.5
        with pytest.raises(ValueError):
            distr.bond_cutoff(0.0, natoms)
    with pytest.raises(ValueError):
        distr.bond_cutoff(0.6, 500)


def test_main_refuses_an_automatic_cutoff_beyond_half_the_box(tmp_path, monkeypatch):
    """4 atoms: the automatic value is 0.85 of the box; the parser's error ends the run before anything is computed or written"""
    pref = str(tmp_path / 'd1.lj.fcc.lammps')
    np.save(pref + '.virial.trgt.npy', np.ones(1, dtype=np.float32))
    np.save(pref + '.temp.trgt.npy', np.ones(1, dtype=np.float32))
    np.save(pref + '.natoms.npy', np.full((1, 1, 1), 4, dtype=np.uint16))
    np.save(pref + '.box.npy', np.full((1, 1, 1), 2.0, dtype=np.float32))
    np.save(pref + '.pos.npy', np.zeros((1, 1, 1, 4, 3), dtype=np.float32))
    monkeypatch.chdir(tmp_path)
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(SystemExit):
        distr.main(['-n', 'd1', '-e', 'LJ', '-bo'])
    assert sorted(os.listdir(tmp_path)) == before
