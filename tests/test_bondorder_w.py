"""Steinhardt's third-order invariants (include/nm_distr.h, nm_distr_bondorder_w) without a GPU: the 3j symbols of the restatement
tests/bondorder_w_ref.py against sympy and against their sum rule, the known w4 and w6 of the fcc, hcp, bcc, simple-cubic and
icosahedral shells (Steinhardt, Nelson and Ronchetti 1983, Table I), also rotated, the properties of the cubic form (zero for odd l,
|w| <= 1, real), the kernel's arithmetic in float64 against the restatement within the derived bound; the C-ABI's declaration, export,
binding and refusals (which precede the device check and leave the outputs alone); the command line's flags."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bondorder_ref as R
import bondorder_w_ref as W
from neuralmelting_amd import _lib as B
from neuralmelting_amd import distr
from test_bondorder import BCC14, BCC8, FCC, HCP, SC, rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -7.25e300
ISENT = -77777777
LD = R.LD

_phi = (1.0 + np.sqrt(5.0)) / 2.0
ICO = np.array([[0, a, b * _phi] for a in (-1, 1) for b in (-1, 1)] + [[a, b * _phi, 0] for a in (-1, 1) for b in (-1, 1)]
               + [[a * _phi, 0, b] for a in (-1, 1) for b in (-1, 1)], dtype=np.float64)
# shell: (vectors, w4 hat, w6 hat); None where q4 vanishes and the ratio means nothing
KNOWN = {'fcc12': (FCC, -0.159317, -0.013161), 'hcp12': (HCP, 0.134097, -0.012442), 'bcc14': (BCC14, 0.159317, 0.013161),
         'bcc8': (BCC8, -0.159317, 0.013161), 'sc6': (SC, 0.159317, 0.013161), 'ico12': (ICO, None, -0.169754)}


# ---- the restatement's 3j symbols
@pytest.mark.parametrize('l', range(1, 13))
def test_symbols_equal_sympy(l):
    wigner = pytest.importorskip('sympy.physics.wigner')
    worst = 0.0
    for m1 in range(-l, l + 1):
        for m2 in range(max(-l, -l - m1), min(l, l - m1) + 1):
            want = wigner.wigner_3j(l, l, l, m1, m2, -m1 - m2)
            worst = max(worst, abs(float(W.wigner3j(l, l, l, m1, m2, -m1 - m2) - LD(str(want.evalf(40))))))
    print('l = %d: largest difference %.3g' % (l, worst))
    assert worst < 1e-18


@pytest.mark.parametrize('l', range(0, 13))
def test_symbols_obey_the_sum_rule(l):
    """sum_{m1, m2} (l l l; m1 m2 m3)^2 = 1, exactly in fractions; every symbol vanishes for odd l with m = (0, 0, 0)"""
    total = sum(W.wigner3j_squared(l, l, l, m1, m2, -m1 - m2)[1] for m1 in range(-l, l + 1) for m2 in range(-l, l + 1))
    assert total == 1
    if l % 2:
        assert W.wigner3j_squared(l, l, l, 0, 0, 0)[0] == 0


def test_term_counts():
    """the symbols that do not vanish, in the kernels' order: 3 l^2 + 3 l + 1 triples, twelve accidental zeros at l = 8"""
    for l, n in zip((2, 4, 6, 8, 10, 12), (19, 61, 127, 205, 331, 469)):
        m1, m2, m3, sym = W.table(l)
        assert len(sym) == n == W.n_terms(l) and (sym != 0).all() and (m1 + m2 + m3 == 0).all()
        assert n == 3 * l * l + 3 * l + 1 - (12 if l == 8 else 0)
        order = list(zip(m1.tolist(), m2.tolist()))
        assert order == sorted(order)
        assert abs(float((sym * sym).sum()) - 1.0) < 1e-17


# ---- known answers on ideal shells
@pytest.mark.parametrize('name', sorted(KNOWN))
def test_known_shells(name):
    vec, w4, w6 = KNOWN[name]
    rng = np.random.default_rng(400)
    for rot in (np.eye(3), rotation(rng), rotation(rng)):
        v = vec @ rot.T
        for l, want in ((4, w4), (6, w6)):
            w3, q2 = W.shell(v, l)
            if want is None:                                                  # the icosahedron's q4 = 0: w3 itself vanishes
                assert abs(float(q2)) < 1e-30 and abs(float(w3)) < 1e-45
            else:
                assert abs(float(w3 / q2 ** LD(1.5)) - want) < 1e-6, (name, l)


def test_icosahedron_is_regular():
    n = ICO / np.linalg.norm(ICO, axis=1)[:, None]
    d = np.sort(np.round(n @ n.T, 12), axis=1)
    assert len(ICO) == 12 and np.allclose(d[:, -2], 1 / np.sqrt(5.0)) and np.allclose(d[:, 0], -1.0)


# ---- properties
@pytest.mark.parametrize('l', range(1, 13))
def test_cubic_form_properties(l):
    """for random vectors with a_-m = (-1)^m conj(a_m): the triple sum is real, vanishes for odd l, and |w hat| <= 1"""
    rng = np.random.default_rng(600 + l)
    re, im = rng.normal(size=(20, l + 1)).astype(LD), rng.normal(size=(20, l + 1)).astype(LD)
    im[:, 0] = 0                                                              # a_0 is real
    a = W.full(re, im, l)
    t = W.cubic_general(a, l)
    norm3 = (np.abs(a) ** 2).sum(axis=-1) ** LD(1.5)
    assert float(np.abs(t.imag / norm3).max()) < 1e-17
    if l % 2:
        assert float(np.abs(t / norm3).max()) < 1e-17
        generic = rng.normal(size=(5, 2 * l + 1)).astype(LD) + 1j * rng.normal(size=(5, 2 * l + 1)).astype(LD)
        g = W.cubic_general(generic.astype(W.CLD), l)                          # no symmetry of the vector is needed
        assert float(np.abs(g).max()) < 1e-16 * float((np.abs(generic) ** 2).sum(axis=-1).max() ** 1.5)
    else:
        w = W.cubic(re, im, l) / R.invariant(re, im, l) ** LD(1.5)
        assert float(np.abs(w - t.real / norm3).max()) < 1e-17                # the table's route equals the plain triple sum
        assert float(np.abs(w).max()) <= 1.0 and float(np.abs(w).max()) > 1e-3


def test_rotation_changes_w_by_rounding_only():
    rng = np.random.default_rng(700)
    vec = rng.normal(size=(13, 3))
    for l in (2, 4, 6, 8, 10, 12):
        one = W.w_hat(vec, l)
        for _ in range(3):
            assert abs(W.w_hat(vec @ rotation(rng).T, l) - one) < 1e-13 * l * l, l   # the rotation matrix itself is float64


# ---- the kernel's arithmetic in float64 against the restatement
def kernel_route(re, im, l):
    """nm_distr_w.h's contraction transcribed: coefficients (4 pi / (2l+1))^(3/2) (3j) rounded once to float64, float64 complex
    products, real part, plain float64 sum in the table's order (the tree's order differs, the bound covers any order)"""
    m1, m2, m3, sym = W.table(l)
    coef = ((4 * R.PI / LD(2 * l + 1)) ** LD(1.5) * sym).astype(np.float64)
    a = W.full(re, im, l).astype(np.complex128)
    a1, a2, a3 = a[..., m1 + l], a[..., m2 + l], a[..., m3 + l]
    pr = a1.real * a2.real - a1.imag * a2.imag
    pi = a1.real * a2.imag + a1.imag * a2.real
    term = coef * (pr * a3.real - pi * a3.imag)
    t = np.zeros(term.shape[:-1])
    for k in range(term.shape[-1]):
        t = t + term[..., k]
    return t


@pytest.mark.parametrize('l', (2, 4, 6, 8, 10, 12))
def test_kernel_route_is_within_the_rounding_part_of_the_bound(l):
    """not a test of the HIP code (tests/test_bondorder_w_gpu.py is): float64 vectors taken as exact (e = 0), so the bound is its
    rounding part (n_l + 12) u x^(3/2)"""
    rng = np.random.default_rng(800 + l)
    re, im = rng.normal(size=(300, l + 1)), rng.normal(size=(300, l + 1))
    im[:, 0] = 0
    scale = np.sqrt((2 * l + 1) / (4 * np.pi)) * rng.random(300) / np.sqrt(re[:, 0] ** 2 + 2 * (re[:, 1:] ** 2 + im[:, 1:] ** 2).sum(axis=1))
    re, im = re * scale[:, None], im * scale[:, None]                          # q2 uniform in (0, 1)
    x = R.invariant(re.astype(LD), im.astype(LD), l)
    err = np.abs(kernel_route(re, im, l).astype(LD) - W.cubic(re.astype(LD), im.astype(LD), l)).astype(np.float64)
    allowed = (W.n_terms(l) + 12) * W.U * x.astype(np.float64) ** 1.5
    print('l = %2d: largest error / allowed %.3g' % (l, (err / allowed).max()))
    assert (err <= allowed).all()
    assert W.tol(l, 1.0, 529, 4095, 'Q') < 5e-13                              # the header's figure


# ---- the C-ABI
NAMES = ('w3', 'wbar3', 'W3', 'q2', 'qbar2', 'Q2', 'nnb')


def call(pos, box, ls, r_lo=1e-16, r_hi=1.4, device=0, natoms=None, ns=None, nl=None, null=()):
    """the raw ABI on sentinel-filled outputs; returns (rc, message, dict of the seven arrays)"""
    L = B.load()
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    box = np.ascontiguousarray(box, dtype=np.float32)
    ls = np.ascontiguousarray(ls, dtype=np.int32)
    n, w = pos.shape[1], max(len(ls), 1)
    out = {k: np.full((pos.shape[0], n, w), SENT) for k in ('w3', 'wbar3', 'q2', 'qbar2')}
    out.update({k: np.full((pos.shape[0], w), SENT) for k in ('W3', 'Q2')})
    out['nnb'] = np.full((pos.shape[0], n), ISENT, dtype=np.int32)
    ptr = dict(pos=pos.ctypes.data_as(B.c_float_p), box=box.ctypes.data_as(B.c_float_p), ls=ls.ctypes.data_as(B.c_int_p))
    ptr.update({k: out[k].ctypes.data_as(B.c_int32_p if k == 'nnb' else B.c_double_p) for k in NAMES})
    for k in null:
        ptr[k] = None
    rc = L.nm_distr_bondorder_w(device, pos.shape[0] if ns is None else ns, n if natoms is None else natoms, ptr['pos'], ptr['box'],
                                float(r_lo), float(r_hi), len(ls) if nl is None else nl, ptr['ls'], *(ptr[k] for k in NAMES))
    return rc, (L.nm_distr_last_error().decode() if rc else ''), out


def untouched(out):
    return all((out[k] == (ISENT if k == 'nnb' else SENT)).all() for k in NAMES)


def test_symbol_is_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, 'include', 'nm_distr.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    assert re.search(r'\bint\s+nm_distr_bondorder_w\s*\(', txt)
    assert 'nm_distr_bondorder_w' in B.DISTR_SYMBOLS
    assert hasattr(C.CDLL(B.LIB_PATH), 'nm_distr_bondorder_w')
    f = B.load().nm_distr_bondorder_w
    assert f.restype is C.c_int
    assert f.argtypes == [C.c_int, C.c_int, C.c_int, B.c_float_p, B.c_float_p, C.c_double, C.c_double, C.c_int, B.c_int_p] \
        + [B.c_double_p] * 6 + [B.c_int32_p]


# case: (arguments, a word of the message)
REFUSED = {
    'ns-1': (dict(ns=-1), 'bad argument'), 'natoms0': (dict(natoms=0), 'natoms'), 'natoms4096': (dict(natoms=4096), 'natoms'),
    'nl0': (dict(nl=0), 'nl'), 'nl7': (dict(ls=(2, 4, 6, 8, 10, 12, 14)), 'nl'), 'l0': (dict(ls=(0, 4)), 'strictly'),
    'l14': (dict(ls=(6, 14)), 'strictly'), 'l-repeated': (dict(ls=(4, 4)), 'strictly'), 'l-decreasing': (dict(ls=(6, 4)), 'strictly'),
    'l-odd': (dict(ls=(4, 5)), 'antisymmetric'), 'l-odd-alone': (dict(ls=(1,)), 'odd'), 'l-odd-first': (dict(ls=(3, 6)), 'even'),
    'r_lo-negative': (dict(r_lo=-1e-3), 'r_lo'), 'r_lo-nan': (dict(r_lo=float('nan')), 'r_lo'),
    'r_hi-equal-r_lo': (dict(r_lo=1.0, r_hi=1.0), 'r_lo'), 'r_hi-nan': (dict(r_hi=float('nan')), 'r_hi'),
    'r_hi-beyond-half-the-smaller-box': (dict(box=[3.0, 2.7], r_hi=1.4), 'half'),
    'box-zero': (dict(box=[3.0, 0.0]), 'box'), 'box-negative': (dict(box=[-3.0, 3.0]), 'box'), 'box-nan': (dict(box=[3.0, float('nan')]), 'box'),
    'box-inf': (dict(box=[float('inf'), 3.0]), 'box'), 'null-pos': (dict(null=('pos',)), 'bad argument'),
    'null-box': (dict(null=('box',)), 'bad argument'), 'null-ls': (dict(null=('ls',)), 'bad argument'),
    'all-outputs-null': (dict(null=NAMES), 'seven'), 'device-1': (dict(device=-1), 'device'),
}


@pytest.mark.parametrize('case', sorted(REFUSED))
def test_refusals_precede_the_device_check(case):
    kw, word = REFUSED[case]
    kw = dict(kw)
    rng = np.random.default_rng(5)
    box = np.array(kw.pop('box', [3.0, 3.0]), dtype=np.float32)
    pos = (rng.random((2, 8, 3)) * 2.9).astype(np.float32)
    rc, msg, out = call(pos, box, kw.pop('ls', (4, 6)), **kw)
    assert rc == B.NM_ERR_ARG
    assert msg.startswith('nm_distr_bondorder_w:') and word in msg, msg
    assert untouched(out)


def test_refusals_come_in_the_order_of_nm_distr_bondorder():
    """a call wrong in several ways at once: each entry point names the same first fault (the odd l stands with the other faults of
    ls, before the shell and the boxes)"""
    from test_bondorder import call as call2
    rng = np.random.default_rng(6)
    pos = (rng.random((2, 8, 3)) * 2.9).astype(np.float32)
    cases = (dict(natoms=0, nl=0, ls=(6, 4), r_lo=-1.0), dict(nl=0, ls=(6, 4), r_lo=-1.0, box=[3.0, -1.0]),
             dict(ls=(6, 4), r_lo=-1.0, box=[3.0, -1.0]), dict(r_lo=-1.0, box=[3.0, -1.0]), dict(box=[3.0, -1.0], r_hi=9.0),
             dict(r_hi=9.0, device=-1), dict(device=-1))
    for kw in cases:
        kw = dict(kw)
        box = np.array(kw.pop('box', [3.0, 3.0]), dtype=np.float32)
        ls = kw.pop('ls', (4, 6))
        rc, msg, out = call(pos, box, ls, **kw)
        rc2, msg2 = call2(pos, box, ls, **kw)[:2]
        assert rc == rc2 == B.NM_ERR_ARG and untouched(out)
        assert msg.split(': ', 1)[1] == msg2.split(': ', 1)[1], (msg, msg2)
    rc, msg, out = call(pos, np.array([3.0, 3.0], dtype=np.float32), (3, 4), r_lo=-1.0)
    assert rc == B.NM_ERR_ARG and 'odd' in msg and untouched(out)


def test_valid_call_without_a_device_is_a_hip_error():
    """as nm_distr_bondorder: NM_ERR_HIP where that entry finds no device, also for an empty batch, and NM_OK where it finds one"""
    from test_bondorder import call as call2
    rng = np.random.default_rng(6)
    pos = (rng.random((2, 8, 3)) * 3.0).astype(np.float32)
    box = np.full(2, 3.0, dtype=np.float32)
    sibling = call2(pos, box, (4, 6))[0]
    assert sibling in (B.NM_OK, B.NM_ERR_HIP)
    for ns in (2, 0):
        rc, msg, out = call(pos, box, (4, 6), ns=ns)
        assert rc == sibling, msg
        if rc == B.NM_ERR_HIP:
            assert msg.startswith('nm_distr_bondorder_w:') and 'no HIP device' in msg and untouched(out)
    if sibling == B.NM_ERR_HIP:
        with pytest.raises(RuntimeError, match='nm_distr_bondorder_w'):
            distr.bond_order_w(np.full(2, 8), box, pos, (4, 6), 1e-16, 1.4)


# ---- the command line
def test_parse_args_bond_w_flags():
    assert distr.parse_args([]).bond_w is False and distr.parse_args(['-bo']).bond_w is False
    a = distr.parse_args(['-bo', '-bw'])
    assert a.bond_w is True and a.bond_l == [4, 6]
    a = distr.parse_args(['--bond_order', '--bond_w', '--bond_l', '12', '2', '--bond_atoms'])
    assert a.bond_w is True and a.bond_l == [2, 12] and a.bond_atoms is True
    assert distr.parse_args(['-bo', '-bl', '3', '5']).bond_l == [3, 5]          # odd values stay fine without -bw
    for bad in (['-bw'], ['-bw', '-bl', '4', '6'], ['-bo', '-bw', '-bl', '5'], ['-bo', '-bw', '-bl', '4', '7'], ['-bo', '-bw', '-bl', '1']):
        with pytest.raises(SystemExit):
            distr.parse_args(bad)
