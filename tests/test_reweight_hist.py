"""Reweighted histograms (include/nm_reweight_hist.h) without a GPU: the C-ABI's declaration, export, binding and refusals (which
precede the device check and leave the outputs alone); the longdouble restatement tests/reweight_hist_ref.py against np.histogram
and against the Erlang known answer of the Gamma set; equal_weight and the command line's flags."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import reweight_hist_ref as H
import reweight_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import reweight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -7.25e300


def test_symbol_is_declared_exported_and_bound():
    txt = open(os.path.join(ROOT, 'include', 'nm_reweight_hist.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    assert sorted(set(re.findall(r'\b(nm_[a-z_0-9]+)\s*\(', txt))) == sorted(B.REWEIGHT_HIST_SYMBOLS) == ['nm_reweight_histogram']
    assert '#include "nm_reweight_hist.h"' in open(os.path.join(ROOT, 'include', 'nm_reweight.h')).read()
    assert hasattr(C.CDLL(B.LIB_PATH), 'nm_reweight_histogram')
    fn = B.load().nm_reweight_histogram
    assert fn.restype is C.c_int and len(fn.argtypes) == 18
    assert [fn.argtypes[i] for i in (0, 1, 9, 12, 14)] == [C.c_int] * 5 and fn.argtypes[6] is C.c_int64 and fn.argtypes[4] is B.c_int64_p
    assert all(fn.argtypes[i] is B.c_double_p for i in (2, 3, 5, 7, 8, 10, 11, 13, 15, 16, 17))


# ---- the raw ABI on sentinel-filled outputs
def base():
    rng = np.random.default_rng(12)
    return dict(b=np.array([1.0, 1.2, 1.5]), c=np.array([0.5, 0.6, 0.7]), count=np.array([3, 0, 5], dtype=np.int64),
                e=rng.gamma(4.0, 1.0, 8), v=rng.gamma(3.0, 1.0, 8), f=np.array([0.0, 0.5, 1.0]), tb=np.array([1.1, 1.3]),
                tc=np.array([0.55, 0.65]), x=rng.random((2, 8)), edges=np.array([[0.0, 0.25, 0.5, 1.0], [-1.0, 0.0, 0.5, 2.0]]))


def _p(a, null, key, typ=B.c_double_p):
    return None if key in null else a.ctypes.data_as(typ)


def call(a, device=0, nstates=None, nsamples=None, ntargets=None, nq=2, nbins=3, null=()):
    L = B.load()
    nt = a['tb'].size
    hist, outside = np.full((nt, 2, 3), SENT), np.full((nt, 2, 2), SENT)
    rc = L.nm_reweight_histogram(device, a['b'].size if nstates is None else nstates, _p(a['b'], null, 'b'), _p(a['c'], null, 'c'),
                                 _p(a['count'], null, 'count', B.c_int64_p), _p(a['f'], null, 'f'),
                                 a['e'].size if nsamples is None else nsamples, _p(a['e'], null, 'e'), _p(a['v'], null, 'v'),
                                 nt if ntargets is None else ntargets, _p(a['tb'], null, 'tb'), _p(a['tc'], null, 'tc'), nq,
                                 _p(a['x'], null, 'x'), nbins, _p(a['edges'], null, 'edges'), _p(hist, null, 'hist'),
                                 _p(outside, null, 'outside'))
    untouched = (hist == SENT).all() and (outside == SENT).all()
    return rc, (L.nm_reweight_last_error().decode() if rc else ''), untouched


def _with(key, index, value):
    def change(a):
        a[key] = a[key].copy()
        a[key][index] = value
    return change


REFUSED = {
    # what nm_reweight_expect refuses
    'nstates0': dict(nstates=0), 'nstates4097': dict(nstates=4097), 'nsamples0': dict(nsamples=0), 'nsamples-1': dict(nsamples=-1),
    'count-negative': dict(change=lambda a: a.update(count=np.array([9, -1, 0], dtype=np.int64))),
    'count-sum-low': dict(change=_with('count', 0, 2)), 'count-sum-high': dict(change=_with('count', 1, 1)),
    'count-overflow': dict(change=lambda a: a.update(count=np.array([2 ** 62, 2 ** 62, 8], dtype=np.int64))),
    'b-nan': dict(change=_with('b', 1, np.nan)), 'c-inf': dict(change=_with('c', 2, np.inf)), 'e-inf': dict(change=_with('e', 7, -np.inf)),
    'v-nan': dict(change=_with('v', 0, np.nan)), 'f-nan': dict(change=_with('f', 2, np.nan)), 'f-inf': dict(change=_with('f', 0, np.inf)),
    'null-b': dict(null=('b',)), 'null-c': dict(null=('c',)), 'null-count': dict(null=('count',)), 'null-e': dict(null=('e',)),
    'null-v': dict(null=('v',)), 'null-f': dict(null=('f',)), 'device-1': dict(device=-1),
    'ntargets0': dict(ntargets=0), 'ntargets65537': dict(ntargets=65537), 'tb-nan': dict(change=_with('tb', 1, np.nan)),
    'tc-inf': dict(change=_with('tc', 0, np.inf)), 'null-tb': dict(null=('tb',)), 'null-tc': dict(null=('tc',)),
    # its own
    'nq0': dict(nq=0), 'nq9': dict(nq=9), 'nq-1': dict(nq=-1), 'nbins0': dict(nbins=0), 'nbins1025': dict(nbins=1025), 'nbins-2': dict(nbins=-2),
    'null-x': dict(null=('x',)), 'null-edges': dict(null=('edges',)), 'null-hist': dict(null=('hist',)),
    'x-nan': dict(change=_with('x', (1, 3), np.nan)), 'x-inf': dict(change=_with('x', (0, 0), np.inf)),
    'edge-nan': dict(change=_with('edges', (0, 1), np.nan)), 'edge-inf': dict(change=_with('edges', (1, 3), np.inf)),
    'edges-equal': dict(change=_with('edges', (1, 1), 0.5)), 'edges-decreasing': dict(change=_with('edges', (0, 2), 0.1)),
    'edges-equal-at-the-end': dict(change=_with('edges', (0, 3), 0.5)),
}


@pytest.mark.parametrize('case', sorted(REFUSED))
def test_refusals_precede_the_device_check(case):
    kw = dict(REFUSED[case])
    a = base()
    kw.pop('change', lambda a: None)(a)
    rc, msg, untouched = call(a, **kw)
    assert rc == B.NM_ERR_ARG, (rc, msg)
    assert msg.startswith('nm_reweight_histogram:'), msg
    assert untouched


def test_more_samples_than_the_accumulator_admits_are_refused():
    """the limit is 2^28 (include/nm_reweight_hist.h), at least the 2^24 asked for: one sample more is refused before e, v or x
    are read (they are 8 long here), by the count alone"""
    a = base()
    a['count'] = np.array([2 ** 28 + 1, 0, 0], dtype=np.int64)
    rc, msg, untouched = call(a, nsamples=2 ** 28 + 1)
    assert rc == B.NM_ERR_ARG and msg.startswith('nm_reweight_histogram:') and '2^28' in msg and untouched
    assert '2^28' in open(os.path.join(ROOT, 'include', 'nm_reweight_hist.h')).read()


def test_a_valid_call_without_a_device_is_a_hip_error():
    """NM_ERR_HIP where the library finds no device (outputs untouched, no host fallback), NM_OK where it finds one; outside
    may be null"""
    a = base()
    rc, msg, untouched = call(a)
    assert rc in (B.NM_OK, B.NM_ERR_HIP), msg
    rc2, msg2, _ = call(a, null=('outside',))
    assert rc2 == rc, msg2
    if rc == B.NM_ERR_HIP:
        assert msg.startswith('nm_reweight_histogram:') and 'no HIP device' in msg and untouched
        with pytest.raises(RuntimeError, match='nm_reweight_histogram'):
            reweight.histogram(a['b'], a['c'], a['count'], a['f'], a['e'], a['v'], a['tb'], a['tc'], a['x'], a['edges'])
    with pytest.raises(ValueError):
        reweight.histogram(a['b'], a['c'], a['count'], a['f'], a['e'], a['v'], a['tb'], a['tc'], a['x'][:, :7], a['edges'])


# ---- the restatement
EDGES = np.array([-1.0, -0.5, -0.125, 0.0, 0.25, 0.75, 1.0, 2.5])


def _one_state(x):
    """one state, the target equal to it: every weight is 1/N"""
    n = x.size
    rng = np.random.default_rng(n)
    one = np.array([1.25]), np.array([0.5])
    return H.histogram(one[0], one[1], np.array([n]), np.array([0.0]), rng.gamma(4.0, 1.0, n), rng.gamma(3.0, 1.0, n), one[0], one[1],
                       x[None, :], EDGES[None, :])


@pytest.mark.parametrize('case', ('random', 'on-every-edge', 'on-the-last-edge', 'outside'))
def test_restatement_against_numpy_histogram(case):
    rng = np.random.default_rng(5)
    x = {'random': rng.uniform(-1.0, 2.5, 1000), 'on-every-edge': np.repeat(EDGES, 3), 'on-the-last-edge': np.full(7, EDGES[-1]),
         'outside': np.concatenate([rng.uniform(-3.0, 4.0, 500), np.nextafter(EDGES[[0, -1]], [-9.0, 9.0])])}[case]
    n = x.size
    hist, outside, ess = _one_state(x)
    want = np.histogram(x, EDGES)[0]
    below, above = int((x < EDGES[0]).sum()), int((x > EDGES[-1]).sum())
    assert want.sum() + below + above == n
    tol = H.tol(n, 1, 0.0, 1.0) * n                     # U: a common factor of all weights cancels in the restatement
    assert np.abs((hist[0, 0] * n).astype(np.float64) - want).max() <= tol
    assert abs(float(outside[0, 0, 0] * n) - below) <= tol and abs(float(outside[0, 0, 1] * n) - above) <= tol
    assert abs(float(ess[0]) - n) <= 1e-9 * n
    if case == 'on-every-edge':
        assert want.tolist() == [3, 3, 3, 3, 3, 3, 6]   # a value on an edge opens the bin; the last edge closes the last bin
    if case == 'outside':
        assert below > 1 and above > 1 and want.sum() < n


def test_restatement_gives_the_erlang_known_answer():
    """The Gamma set (6 x 6000 samples, exact f, the 11 targets): e ~ Gamma(8, 1/tb) at a target, so the probability of a bin is a
    difference of the closed-form Erlang distribution function.  16 bins on [0, 3 a / tb_min]; every bin within 5 standard errors
    sqrt(p (1 - p) / ess) of the restatement's own ess.  Observed with the fixed seed: the largest deviation is 2.9 standard
    errors."""
    b, c, count, e, v = R.gamma_set()
    tb, tc = R.gamma_targets()
    edges = np.linspace(0.0, 3.0 * R.GAMMA_A / tb.min(), 17)
    hist, outside, ess = H.histogram(b, c, count, R.gamma_exact_f(), e, v, tb, tc, e[None, :], edges[None, :])
    cdf = np.array([H.erlang_cdf(R.GAMMA_A, t, edges) for t in tb])
    p = np.diff(cdf, axis=1)
    sigma = np.sqrt(p * (1.0 - p) / ess.astype(np.float64)[:, None])
    dev = np.abs(hist[:, 0].astype(np.float64) - p)
    print('restatement against the Erlang bins: largest deviation %.3g standard errors; ess %.0f .. %.0f' % (
        (dev / sigma).max(), float(ess.min()), float(ess.max())))
    assert p.shape == (11, 16) and (p > 0).all() and abs(p.sum(axis=1) + 1.0 - cdf[:, -1] - 1.0).max() < 1e-12
    assert (dev <= 5.0 * sigma).all()
    assert (outside[:, 0, 0] == 0).all()
    pa = 1.0 - cdf[:, -1]
    assert (np.abs(outside[:, 0, 1].astype(np.float64) - pa) <= 5.0 * np.sqrt(pa * (1.0 - pa) / ess.astype(np.float64)) + 1e-12).all()
    total = hist[:, 0].sum(axis=1) + outside[:, 0].sum(axis=1)
    assert np.abs(total.astype(np.float64) - 1.0).max() <= 1e-15


def test_erlang_cdf_and_codes():
    assert abs(H.erlang_cdf(1, 2.0, 0.5) - (1 - np.exp(-1.0))) < 1e-15
    assert abs(H.erlang_cdf(2, 1.0, 1.0) - (1 - 2 * np.exp(-1.0))) < 1e-15
    assert H.codes([-2.0, -1.0, -0.5, 2.4, 2.5, 2.6], EDGES).tolist() == [-1, 0, 1, 6, 6, 7]
    assert H.tol(10, 3, 2.0, 0.5) == R.tol_map(10, 3, 2.0) + 10 * 2.0 ** -96


# ---- equal_weight
def test_equal_weight():
    t = np.array([1.0, 1.5, 2.0, 3.0, 4.0])
    above = np.array([[0.125, 0.25, 0.625, 0.9, 1.0], # between two grid points: 1.5 + 0.5 * 0.25 / 0.375
                      [0.9, 0.5, 0.2, 0.1, 0.0],      # a value exactly 1/2
                      [0.0, 0.1, 0.2, 0.3, 0.4],      # no crossing
                      [0.25, 0.75, 0.25, 0.75, 0.1],  # more than one: the first
                      [0.2, 0.5, 0.5, 0.5, 0.8],      # a flat stretch at 1/2: where it is reached
                      [0.5, 0.5, 0.5, 0.5, 0.5],      # flat throughout: none
                      [0.5, 0.5, 0.7, 0.2, 0.1]])     # leaving a flat start
    got = reweight.equal_weight(t, above)
    assert got.shape == (7,) and got.dtype == np.float64
    assert got[0] == 1.5 + 0.5 * (0.25 / 0.375)
    assert got[1] == 1.5 and np.isnan(got[2]) and got[3] == 1.25 and got[4] == 1.5 and np.isnan(got[5]) and got[6] == 1.5
    assert np.isnan(reweight.equal_weight(np.array([1.0]), np.array([[0.5]]))).all()           # a single temperature has no pair
    assert reweight.equal_weight(t, above[0]).tolist() == [got[0]]                              # one pressure as a vector


def test_linear_edges_and_cut_weight():
    x = np.array([[1.0, 3.0, 2.0, 1.5], [4.0, 4.0, 4.0, 4.0]])
    edges = reweight.linear_edges(x, 4)
    assert np.array_equal(edges[0], np.linspace(1.0, 3.0, 5)) and np.array_equal(edges[1], np.linspace(3.5, 4.5, 5))
    hist = np.arange(16.0).reshape(2, 2, 4)
    above, at = reweight.cut_weight(hist, edges, 2.2)           # the nearest edge is 2.0, the bins 2 and 3 lie at or above it
    assert at == 2.0 and above.tolist() == [2.0 + 3.0, 10.0 + 11.0]
    assert reweight.cut_weight(hist, edges, -7.0)[1] == 1.0 and reweight.cut_weight(hist, edges, 7.0)[0].tolist() == [0.0, 0.0]


# ---- flags
def test_cli_flags(capsys):
    a = reweight.parse_args([])
    assert (a.histogram, a.histogram_bins, a.histogram_cut) == ([], 128, None)
    a = reweight.parse_args(['-hq', 'sof', 'pe', 'vol', '-hb', '64', '-hx', '0.5'])
    assert (a.histogram, a.histogram_bins, a.histogram_cut) == (['sof', 'pe', 'vol'], 64, 0.5)
    assert reweight.parse_args(['-hq'] + ['x'] * 8 + ['-hb', '1024']).histogram_bins == 1024
    for bad in (['-hx', '0.5'], ['-hq'] + ['x'] * 9, ['-hq', 'pe', '-hb', '0'], ['-hq', 'pe', '-hb', '1025'], ['-hq'], ['-hq', 'pe', '-hx', 'nan']):
        with pytest.raises(SystemExit) as err:
            reweight.parse_args(bad)
        assert err.value.code == 2                      # argparse's error
    assert '-hx needs -hq' in capsys.readouterr().err
    assert reweight.SUFFIXES == ('rwf', 'rwi', 'rwt', 'rwg', 'rwh', 'rwv', 'rwc', 'rwn', 'rwo', 'rwm')
    assert reweight.HIST_SUFFIXES == ('rwx', 'rwp', 'rwa', 'rwe')


def test_cli_refuses_a_bad_histogram_name_before_writing(tmp_path, monkeypatch):
    prefix = str(tmp_path / 'rw.lj.fcc.lammps')
    rng = np.random.default_rng(1)
    np.save(prefix + '.virial.trgt.npy', np.linspace(1, 2, 2, dtype=np.float32))
    np.save(prefix + '.temp.trgt.npy', np.linspace(1, 2, 4, dtype=np.float32))
    np.save(prefix + '.pe.npy', rng.random((2, 4, 20)).astype(np.float32))
    np.save(prefix + '.vol.npy', rng.random((2, 4, 20)).astype(np.float32))
    np.save(prefix + '.natoms.npy', np.full((2, 4, 20), 32, dtype=np.uint16))
    monkeypatch.chdir(tmp_path)
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(SystemExit, match='-hq cnf: .*cnf.npy is missing'):
        reweight.main(['-n', 'rw', '-hq', 'pe', 'cnf'])
    assert sorted(os.listdir(tmp_path)) == before
