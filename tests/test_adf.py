"""Angular distribution (include/nm_distr.h, nm_distr_angles) without a GPU: the numpy restatement tests/adf_ref.py against
a plain triple loop, known answers on perfect fcc lattices, the cosine-table bins against np.histogram(arccos), the triplet
total; the C-ABI's export, binding and refusals (which precede the device check); the command line's new flags."""
import ctypes as C
import math

import numpy as np
import pytest

import adf_ref as A
from distr_ref import BR
from neuralmelting_amd import _lib as B
from neuralmelting_amd import distr, lattice

SENT = 0xDEADBEEFDEADBEEF


def triple_loop(pos, box, cos_edges, r_lo, r_hi):
    """the definition, one scalar operation at a time (np.float32 scalars for the float32 part, Python floats for float64)"""
    n = len(pos)
    nb = len(cos_edges)
    adf = [0] * nb
    trip = 0
    for c in range(n):
        nbr = []
        for j in range(27):
            for a in range(n):
                v = [pos[a][t] - (pos[c][t] + np.float32(box) * np.float32(BR[j][t])) for t in range(3)]
                assert all(type(x) is np.float32 for x in v)
                d2 = v[0] * v[0]
                d2 = d2 + v[1] * v[1]
                d2 = d2 + v[2] * v[2]
                d = float(np.sqrt(d2))
                if r_lo < d <= r_hi:
                    nbr.append([float(x) for x in v])
        for i in range(len(nbr)):
            for j in range(i + 1, len(nbr)):
                (x1, y1, z1), (x2, y2, z2) = nbr[i], nbr[j]
                n1 = (x1 * x1 + y1 * y1) + z1 * z1
                n2 = (x2 * x2 + y2 * y2) + z2 * z2
                dot = (x1 * x2 + y1 * y2) + z1 * z2
                cth = min(1.0, max(-1.0, dot / math.sqrt(n1 * n2)))
                trip += 1
                for k in range(nb - 1):
                    if cos_edges[k] >= cth > cos_edges[k + 1] or (k == nb - 2 and cth == cos_edges[nb - 1]):
                        adf[k + 1] += 1
    return np.array(adf, dtype=np.int64), trip


@pytest.mark.parametrize('n,seed', ((1, 0), (2, 1), (5, 2), (9, 3), (12, 4), (12, 5)))
def test_restatement_equals_triple_loop(n, seed):
    rng = np.random.default_rng(seed)
    box = np.float32(2.0 + rng.random())
    pos = (rng.random((n, 3)) * box).astype(np.float32)
    if seed == 5:                                                            # integer grid: right angles, straight lines, ties
        box = np.float32(4.0)
        pos = rng.permutation(64)[:n, None] // np.array([16, 4, 1]) % 4
        pos = pos.astype(np.float32)
    l = float(box)
    for ce, r_lo, r_hi in ((A.angle_domain(16)[1], 1e-16 * l, 0.5 * l), (A.angle_domain(2)[1], 0.0, 0.4 * l),
                           (np.array([0.9, 0.5, 0.0, -0.25, -0.5]), 0.2 * l, 0.5 * l)):
        got, trip = A.counts(pos[None], [box], ce, r_lo, r_hi)
        want, wtrip = triple_loop(pos, box, ce, r_lo, r_hi)
        np.testing.assert_array_equal(got[0], want)
        assert trip[0] == wtrip and got[0, 0] == 0
    assert n < 5 or wtrip > 0


def perfect_fcc(cells, a0):
    b = np.float32(cells * a0)
    return (lattice.fcc_fractional(cells) * b).astype(np.float32), b


@pytest.mark.parametrize('cells,el', ((4, 'LJ'), (5, 'Al')))
def test_fcc_first_shell_known_answer(cells, el):
    """12 nearest neighbours: 66 pairs per atom, 24 at 60, 12 at 90, 24 at 120 and 6 at 180 degrees; with 62 edges
    (a[k] = k pi / 61) these angles lie inside bins 20, 30, 40 and 60, i.e. entries 21, 31, 41, 61"""
    a0 = lattice.lattice_constant(el)
    pos, b = perfect_fcc(cells, a0)
    n = len(pos)
    a, ce = A.angle_domain(62)
    adf, trip = A.counts(pos[None], [b], ce, 1e-16 * float(b), 0.85 * a0)
    want = np.zeros(62, dtype=np.int64)
    want[[21, 31, 41, 61]] = np.array([24, 12, 24, 6]) * n
    np.testing.assert_array_equal(adf[0], want)
    assert trip[0] == 66 * n == adf[0].sum()


@pytest.mark.parametrize('n,sbins', ((60, 64), (150, 64), (256, 64), (60, 32), (150, 32)))
def test_cosine_table_equals_arccos_histogram(n, sbins):
    """seeded random frames, shell (1e-16 l, l/2]: the cosine-table counts are np.histogram(np.arccos(cth), a) exactly (a
    condition on the fixture: no angle of these frames lies within an acos rounding of an edge), every triplet lands in a
    bin (cos_edges spans [-1, 1] exactly), and the total is the sum over the centres of M (M - 1) / 2"""
    rng = np.random.default_rng(4000 + n + sbins)
    box = np.float32((n / 0.9) ** (1 / 3))
    pos = (rng.random((1, n, 3)) * box).astype(np.float32)
    a, ce = A.angle_domain(sbins)
    assert ce[0] == 1.0 and ce[-1] == -1.0 and (np.diff(ce) < 0).all()
    l = float(box)
    got, trip = A.counts(pos, [box], ce, 1e-16 * l, 0.5 * l)
    ref, _ = A.counts(pos, [box], ce, 1e-16 * l, 0.5 * l, angle_edges=a)
    np.testing.assert_array_equal(got, ref)
    m = np.array([len(A.neighbours(pos[0], box, c, 1e-16 * l, 0.5 * l)) for c in range(n)])
    assert trip[0] == (m * (m - 1) // 2).sum() == got.sum()
    assert trip[0] > 0.1 * n ** 3                                            # M ~ 0.52 n


# ---- the C-ABI
def call(pos, box, r_lo, r_hi, ce, device=0, natoms=None, abins=None, null=None, ns=None):
    L = B.load()
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    box = np.ascontiguousarray(box, dtype=np.float32)
    ce = np.ascontiguousarray(ce, dtype=np.float64)
    nb = len(ce) if abins is None else abins
    out = np.full((pos.shape[0], max(nb, len(ce))), SENT, dtype=np.uint64)
    ptr = dict(pos=pos.ctypes.data_as(B.c_float_p), box=box.ctypes.data_as(B.c_float_p), ce=ce.ctypes.data_as(B.c_double_p),
               adf=out.ctypes.data_as(B.c_uint64_p))
    if null:
        ptr[null] = None
    rc = L.nm_distr_angles(device, pos.shape[0] if ns is None else ns, pos.shape[1] if natoms is None else natoms, ptr['pos'],
                           ptr['box'], r_lo, r_hi, nb, ptr['ce'], ptr['adf'])
    return rc, (L.nm_distr_last_error().decode() if rc else ''), out


def test_symbol_is_exported_and_bound():
    assert 'nm_distr_angles' in B.DISTR_SYMBOLS
    raw = C.CDLL(B.LIB_PATH)
    assert hasattr(raw, 'nm_distr_angles')
    f = B.load().nm_distr_angles
    assert f.restype is C.c_int and len(f.argtypes) == 10
    assert f.argtypes[5] is C.c_double and f.argtypes[6] is C.c_double and f.argtypes[9] is B.c_uint64_p


_CE = A.angle_domain(16)[1]
REFUSED = {
    'natoms0': dict(natoms=0), 'natoms4096': dict(natoms=4096), 'abins1': dict(abins=1), 'abins257': dict(ce=np.linspace(1, -1, 257)),
    'edges-equal': dict(ce=np.array([1.0, 0.5, 0.5, -1.0])), 'edges-increasing': dict(ce=_CE[::-1]),
    'edges-nan': dict(ce=np.array([1.0, np.nan, -1.0])), 'r_lo-negative': dict(r_lo=-0.1), 'r_lo-equals-r_hi': dict(r_lo=1.0, r_hi=1.0),
    'r_lo-above-r_hi': dict(r_lo=1.5, r_hi=1.0), 'r_hi-nan': dict(r_hi=float('nan')), 'r_hi-above-half-box': dict(r_hi=1.5001),
    'r_hi-above-half-smallest-box': dict(r_hi=1.5, box=[3.0, 2.9]), 'null-pos': dict(null='pos'), 'null-box': dict(null='box'),
    'null-edges': dict(null='ce'), 'null-adf': dict(null='adf'), 'device-1': dict(device=-1), 'ns-1': dict(ns=-1),
}


@pytest.mark.parametrize('case', sorted(REFUSED))
def test_refusals_precede_the_device_check(case):
    kw = dict(REFUSED[case])
    rng = np.random.default_rng(5)
    box = np.array(kw.pop('box', [3.0, 3.0]), dtype=np.float32)
    pos = (rng.random((2, 8, 3)) * 2.9).astype(np.float32)
    rc, msg, out = call(pos, box, kw.pop('r_lo', 1e-16), kw.pop('r_hi', 1.5), kw.pop('ce', _CE), **kw)
    assert rc == B.NM_ERR_ARG
    assert msg.startswith('nm_distr_angles:')
    assert (out == SENT).all()


def test_valid_call_without_a_device_is_a_hip_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip('a GPU is present')
    rng = np.random.default_rng(6)
    pos = (rng.random((2, 8, 3)) * 3.0).astype(np.float32)
    for ns in (2, 0):
        rc, msg, out = call(pos, np.full(2, 3.0), 1e-16, 1.5, _CE, ns=ns)
        assert rc == B.NM_ERR_HIP and msg.startswith('nm_distr_angles:') and 'no HIP device' in msg
        assert (out == SENT).all()
    with pytest.raises(RuntimeError, match='nm_distr_angles'):
        distr.angles(np.full(2, 8), np.full(2, 3.0), pos, A.angle_domain(16)[0], 1e-16, 1.5)


# ---- the command line
def test_parse_args_angular_flags():
    a = distr.parse_args([])
    assert a.angular is False and a.angular_cutoff == 0.5
    a = distr.parse_args(['-ad'])
    assert a.angular is True and a.angular_cutoff == 0.5
    a = distr.parse_args(['--angular', '--angular_cutoff', '0.2125'])
    assert a.angular is True and a.angular_cutoff == 0.2125
    assert distr.parse_args(['-ac', '0.5']).angular_cutoff == 0.5
    for bad in ('0', '0.0', '-0.1', '0.5000001', '1', 'nan'):
        with pytest.raises(SystemExit):
            distr.parse_args(['-ad', '-ac', bad])
