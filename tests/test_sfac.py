"""Static structure factor (include/nm_distr.h, nm_distr_sfactor) without a GPU: the C-ABI's declaration, export, binding and
refusals (which precede the device check and leave the outputs alone); the shells by brute force; the long-double restatement
tests/sfac_ref.py against an independent float64 direct evaluation and against the fcc known answer; the command line's flags."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sfac_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import distr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -7.25e300


def call(pos, box, qmax, device=0, natoms=None, ns=None, null=()):
    """the raw ABI on sentinel-filled outputs; returns (rc, message, sf_sum, sf_max)"""
    L = B.load()
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    box = np.ascontiguousarray(box, dtype=np.float32)
    nsh = max(1, min(qmax, 40)) ** 2 + 1
    ssum = np.full((pos.shape[0], nsh), SENT, dtype=np.float64)
    smax = np.full((pos.shape[0], nsh), SENT, dtype=np.float64)
    ptr = dict(pos=pos.ctypes.data_as(B.c_float_p), box=box.ctypes.data_as(B.c_float_p), sum=ssum.ctypes.data_as(B.c_double_p),
               max=smax.ctypes.data_as(B.c_double_p))
    for k in null:
        ptr[k] = None
    rc = L.nm_distr_sfactor(device, pos.shape[0] if ns is None else ns, pos.shape[1] if natoms is None else natoms, ptr['pos'],
                            ptr['box'], qmax, ptr['sum'], ptr['max'])
    return rc, (L.nm_distr_last_error().decode() if rc else ''), ssum, smax


def test_symbol_is_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, 'include', 'nm_distr.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    assert re.search(r'\bint\s+nm_distr_sfactor\s*\(', txt)
    assert 'nm_distr_sfactor' in B.DISTR_SYMBOLS
    assert hasattr(C.CDLL(B.LIB_PATH), 'nm_distr_sfactor')
    f = B.load().nm_distr_sfactor
    assert f.restype is C.c_int
    assert f.argtypes == [C.c_int, C.c_int, C.c_int, B.c_float_p, B.c_float_p, C.c_int, B.c_double_p, B.c_double_p]


REFUSED = {
    'ns-1': dict(ns=-1), 'natoms0': dict(natoms=0), 'natoms4096': dict(natoms=4096), 'qmax0': dict(qmax=0), 'qmax-1': dict(qmax=-1),
    'qmax33': dict(qmax=33), 'box-zero': dict(box=[3.0, 0.0]), 'box-negative': dict(box=[-3.0, 3.0]),
    'box-nan': dict(box=[3.0, float('nan')]), 'box-inf': dict(box=[float('inf'), 3.0]), 'null-pos': dict(null=('pos',)),
    'null-box': dict(null=('box',)), 'both-outputs-null': dict(null=('sum', 'max')), 'device-1': dict(device=-1),
}


@pytest.mark.parametrize('case', sorted(REFUSED))
def test_refusals_precede_the_device_check(case):
    kw = dict(REFUSED[case])
    rng = np.random.default_rng(5)
    box = np.array(kw.pop('box', [3.0, 3.0]), dtype=np.float32)
    pos = (rng.random((2, 8, 3)) * 2.9).astype(np.float32)
    rc, msg, ssum, smax = call(pos, box, kw.pop('qmax', 4), **kw)
    assert rc == B.NM_ERR_ARG
    assert msg.startswith('nm_distr_sfactor:')
    assert (ssum == SENT).all() and (smax == SENT).all()


def test_valid_call_without_a_device_is_a_hip_error():
    """as nm_distr_angles: NM_ERR_HIP where that entry finds no device, also for an empty batch, and NM_OK where it finds one"""
    rng = np.random.default_rng(6)
    pos = (rng.random((2, 8, 3)) * 3.0).astype(np.float32)
    box = np.full(2, 3.0, dtype=np.float32)
    ce = np.ascontiguousarray(np.cos(np.linspace(1e-16, np.pi, 16)))
    adf = np.zeros((2, 16), dtype=np.uint64)
    L = B.load()
    sibling = L.nm_distr_angles(0, 2, 8, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), 1e-16, 1.5, 16,
                                ce.ctypes.data_as(B.c_double_p), adf.ctypes.data_as(B.c_uint64_p))
    assert sibling in (B.NM_OK, B.NM_ERR_HIP)
    for ns in (2, 0):
        rc, msg, ssum, smax = call(pos, box, 4, ns=ns)
        assert rc == sibling, msg
        if rc == B.NM_ERR_HIP:
            assert msg.startswith('nm_distr_sfactor:') and 'no HIP device' in msg
            assert (ssum == SENT).all() and (smax == SENT).all()
    if sibling == B.NM_ERR_HIP:
        with pytest.raises(RuntimeError, match='nm_distr_sfactor'):
            distr.sfactor(np.full(2, 8), box, pos, 4)


@pytest.mark.parametrize('qmax,nshell,nvec', ((1, 1, 6), (8, 54, 2 * 1054), (16, 214, 2 * 8538)))
def test_shells_equal_a_brute_force_count(qmax, nshell, nvec):
    count = {}
    for h in range(-qmax, qmax + 1):
        for k in range(-qmax, qmax + 1):
            for l in range(-qmax, qmax + 1):
                n2 = h * h + k * k + l * l
                if 1 <= n2 <= qmax * qmax:
                    count[n2] = count.get(n2, 0) + 1
    shells, mult = distr.sfactor_shells(qmax)
    assert shells.dtype == np.int64 and mult.dtype == np.int64
    assert shells.tolist() == sorted(count) and mult.tolist() == [count[n] for n in sorted(count)]
    assert len(shells) == nshell and mult.sum() == nvec
    # Legendre: exactly the n2 = 4^a (8 b + 7) are no sum of three squares
    empty = set(range(1, qmax * qmax + 1)) - set(shells.tolist())
    for n in range(1, qmax * qmax + 1):
        m = n
        while m % 4 == 0:
            m //= 4
        assert (m % 8 == 7) == (n in empty)
    v, n2 = R.vectors(qmax)
    assert len(v) == nvec and np.array_equal(np.unique(n2), shells)


def test_shells_refuse_a_qmax_out_of_range():
    for bad in (0, 33):
        with pytest.raises(ValueError):
            distr.sfactor_shells(bad)


def test_restatement_equals_a_float64_direct_evaluation():
    """20 atoms, qmax 8: S = |sum_a exp(-2 pi i q . u_a)|^2 / N one vector at a time in complex128, no tables, no phase reduction"""
    rng = np.random.default_rng(7)
    n, qmax = 20, 8
    box = np.float32(3.7)
    pos = (rng.random((n, 3)) * box).astype(np.float32)
    u = pos.astype(np.float64) / np.float64(box)
    v, n2 = R.vectors(qmax)
    direct = np.array([abs(np.exp(-2j * np.pi * (u @ q.astype(np.float64))).sum()) ** 2 / n for q in v])
    got = R.per_vector(pos, box, qmax)[0]
    t = R.tol(n, qmax, float(np.abs(u).max()))
    assert t < 2e-12
    err = float(np.abs(got - direct).max())
    print('restatement against float64 direct: max |dS| = %.3g, tolerance %.3g' % (err, t))
    assert err <= t
    ssum, smax = R.shells(pos, box, qmax)
    for k in (1, 9, 27, 64):
        assert abs(float(ssum[0, k]) - direct[n2 == k].sum()) <= t * (n2 == k).sum()
        assert abs(float(smax[0, k]) - direct[n2 == k].max()) <= t
    assert ssum[0, 0] == 0 and ssum[0, 7] == 0 and smax[0, 28] == 0               # 7 and 28 = 4 * 7 are empty shells
    # S(-q) = S(q)
    order = {tuple(q): i for i, q in enumerate(v.tolist())}
    mirror = np.array([order[tuple(-q)] for q in v])
    assert float(np.abs(got - got[mirror]).max()) < 1e-17 * n


def test_restatement_gives_the_fcc_known_answer():
    """fcc on integer coordinates (a0 = 2, box 2 * cells): S = N where h, k, l are multiples of cells whose quotients share
    their parity, 0 elsewhere"""
    cells, qmax = 2, 8
    base = np.array([[0, 0, 0], [0, 1, 1], [1, 0, 1], [1, 1, 0]])
    g = np.arange(cells) * 2
    pos = (np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 1, 3) + base).reshape(-1, 3).astype(np.float32)
    n = len(pos)
    assert n == 32
    sv = R.per_vector(pos, np.float32(2 * cells), qmax)[0]
    v, n2 = R.vectors(qmax)
    w = v // cells
    bragg = (v % cells == 0).all(axis=1) & (w[:, 0] % 2 == w[:, 1] % 2) & (w[:, 1] % 2 == w[:, 2] % 2)
    assert bragg.sum() > 0 and (n2[bragg] == 12).sum() == 8
    assert float(np.abs(sv - np.where(bragg, n, 0)).max()) < 1e-15


# ---- the command line
def test_parse_args_structure_factor_flags():
    a = distr.parse_args([])
    assert a.structure_factor is False and a.q_max == 16
    a = distr.parse_args(['-sf'])
    assert a.structure_factor is True and a.q_max == 16
    a = distr.parse_args(['--structure_factor', '--q_max', '8'])
    assert a.structure_factor is True and a.q_max == 8
    assert distr.parse_args(['-sq', '1']).q_max == 1 and distr.parse_args(['-sq', '32']).q_max == 32
    for bad in ('0', '33', '-1', '2.5'):
        with pytest.raises(SystemExit):
            distr.parse_args(['-sf', '-sq', bad])
