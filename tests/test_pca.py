"""The principal component stage without a GPU (include/nm_pca.h, neuralmelting_amd/pca.py): the interface, every refusal that
precedes the device check on sentinel-filled outputs, the stage's own error channel, the host pipeline against tests/pca_ref.py,
and the command line's refusals."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pca_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import pca

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -7.25e300


def test_header_symbols_are_exported_and_bound():
    txt = open(os.path.join(ROOT, 'include', 'nm_pca.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    syms = sorted(set(re.findall(r'\b(nm_[a-z_0-9]+)\s*\(', txt)))
    assert syms == sorted(B.PCA_SYMBOLS) and len(syms) == 4
    raw = C.CDLL(B.LIB_PATH)
    for s in syms:
        assert hasattr(raw, s), s
    L = B.load()
    assert L.nm_pca_moments.restype is C.c_int and len(L.nm_pca_moments.argtypes) == 8
    assert L.nm_pca_project.restype is C.c_int and len(L.nm_pca_project.argtypes) == 10
    assert L.nm_pca_last_error.restype is C.c_char_p


# ---- the raw ABI on sentinel-filled outputs
def base():
    rng = np.random.default_rng(5)
    return dict(x=rng.random((6, 3)).astype(np.float32), mean=rng.random(3), inv_scale=rng.random(3) + 0.5, comp=rng.random((2, 3)))


def _p(a, null, key, typ=B.c_double_p):
    return None if key in null else a.ctypes.data_as(typ)


def call_moments(a, device=0, nsamples=None, nfeat=None, null=()):
    L = B.load()
    n, d = a['x'].shape
    out = dict(mean=np.full(d, SENT), lo=np.full(d, SENT), hi=np.full(d, SENT), gram=np.full((d, d), SENT))
    rc = L.nm_pca_moments(device, n if nsamples is None else nsamples, d if nfeat is None else nfeat, _p(a['x'], null, 'x', B.c_float_p),
                          _p(out['mean'], null, 'mean'), _p(out['lo'], null, 'lo'), _p(out['hi'], null, 'hi'), _p(out['gram'], null, 'gram'))
    return rc, (L.nm_pca_last_error().decode() if rc else ''), all((v == SENT).all() for v in out.values())


def call_project(a, device=0, nsamples=None, nfeat=None, ncomp=None, null=()):
    L = B.load()
    n, nc = a['x'].shape[0], a['comp'].shape[0]
    out = dict(z=np.full((n, nc), SENT), norm2=np.full(n, SENT))
    rc = L.nm_pca_project(device, n if nsamples is None else nsamples, a['x'].shape[1] if nfeat is None else nfeat,
                          _p(a['x'], null, 'x', B.c_float_p), _p(a['mean'], null, 'mean'), _p(a['inv_scale'], null, 'inv_scale'),
                          nc if ncomp is None else ncomp, _p(a['comp'], null, 'comp'), _p(out['z'], null, 'z'), _p(out['norm2'], null, 'norm2'))
    return rc, (L.nm_pca_last_error().decode() if rc else ''), all((v == SENT).all() for v in out.values())


def _with(key, index, value):
    def change(a):
        a[key] = a[key].copy()
        a[key][index] = value
    return change


COMMON = {
    'nfeat0': dict(nfeat=0), 'nfeat-1': dict(nfeat=-1), 'nfeat4097': dict(nfeat=4097), 'nsamples1': dict(nsamples=1), 'nsamples0': dict(nsamples=0),
    'nsamples-5': dict(nsamples=-5), 'size-over-2^40': dict(nsamples=2 ** 40 // 3 + 1), 'size-far-over': dict(nsamples=2 ** 62),
    'null-x': dict(null=('x',)), 'device-1': dict(device=-1),
}
MOMENTS_ONLY = {'null-mean': dict(null=('mean',)), 'null-lo': dict(null=('lo',)), 'null-hi': dict(null=('hi',)), 'null-gram': dict(null=('gram',))}
PROJECT_ONLY = {
    'ncomp0': dict(ncomp=0), 'ncomp-1': dict(ncomp=-1), 'ncomp65': dict(ncomp=65), 'ncomp-above-nfeat': dict(ncomp=4),
    'mean-nan': dict(change=_with('mean', 1, np.nan)), 'inv_scale-inf': dict(change=_with('inv_scale', 2, np.inf)),
    'comp-nan': dict(change=_with('comp', (1, 2), np.nan)), 'comp-inf': dict(change=_with('comp', (0, 0), -np.inf)),
    'null-mean': dict(null=('mean',)), 'null-inv_scale': dict(null=('inv_scale',)), 'null-comp': dict(null=('comp',)), 'null-z': dict(null=('z',)),
}


def _refused(fn, cases, case):
    kw = dict(cases[case])
    a = base()
    kw.pop('change', lambda a: None)(a)
    rc, msg, untouched = fn(a, **kw)
    assert rc == B.NM_ERR_ARG, (rc, msg)
    assert msg.startswith(fn.__name__.replace('call_', 'nm_pca_') + ':'), msg
    assert untouched


@pytest.mark.parametrize('case', sorted({**COMMON, **MOMENTS_ONLY}))
def test_moments_refusals_precede_the_device_check(case):
    _refused(call_moments, {**COMMON, **MOMENTS_ONLY}, case)


@pytest.mark.parametrize('case', sorted({**COMMON, **PROJECT_ONLY}))
def test_project_refusals_precede_the_device_check(case):
    _refused(call_project, {**COMMON, **PROJECT_ONLY}, case)


def test_the_stage_has_an_error_channel_of_its_own():
    L = B.load()
    assert call_moments(base(), nfeat=0)[0] == B.NM_ERR_ARG
    mine = L.nm_pca_last_error()
    assert mine.startswith(b'nm_pca_moments:')
    d = np.zeros(4)
    dp = d.ctypes.data_as(B.c_double_p)
    assert L.nm_reweight_solve(0, 0, dp, dp, None, 1, dp, dp, 1e-9, 1, dp, None, None, None) == B.NM_ERR_ARG
    assert L.nm_distr_histograms(0, 0, 0, None, None, 0, None, 0, None, None, None) != B.NM_OK
    theirs = (L.nm_reweight_last_error(), L.nm_distr_last_error())
    assert theirs[0].startswith(b'nm_reweight_solve:') and theirs[1].startswith(b'nm_distr_histograms:')
    assert L.nm_pca_last_error() == mine                                 # they left it alone
    assert call_project(base(), ncomp=0)[0] == B.NM_ERR_ARG
    assert L.nm_pca_last_error().startswith(b'nm_pca_project:')
    assert (L.nm_reweight_last_error(), L.nm_distr_last_error()) == theirs     # and it left them alone


def test_valid_calls_without_a_device_are_hip_errors():
    """NM_ERR_HIP where the library finds no device (outputs untouched, no host fallback), NM_OK where it finds one"""
    a = base()
    seen = set()
    for fn, name in ((call_moments, 'nm_pca_moments'), (call_project, 'nm_pca_project')):
        rc, msg, untouched = fn(a)
        assert rc in (B.NM_OK, B.NM_ERR_HIP), msg
        seen.add(rc)
        if rc == B.NM_ERR_HIP:
            assert msg.startswith(name + ':') and 'no HIP device' in msg and untouched
    assert len(seen) == 1
    rc, msg, _ = call_project(a, null=('norm2',))                        # norm2 may be null
    assert {rc} == seen, msg
    if seen == {B.NM_ERR_HIP}:
        with pytest.raises(RuntimeError, match='nm_pca_moments'):
            pca.moments(a['x'])
        with pytest.raises(RuntimeError, match='nm_pca_project'):
            pca.project(a['x'], a['mean'], a['inv_scale'], a['comp'])


# ---- the host pipeline, from given moments
def _moments(x):
    """float64 moments of x (N, D) float32 as the device would hand them over (to rounding)"""
    m = np.asarray(R.mean(x), dtype=np.float64)
    return m, x.min(axis=0).astype(np.float64), x.max(axis=0).astype(np.float64), np.asarray(R.gram(x, m)[0], dtype=np.float64)


def _data(n=400, seed=3):
    """planted variances 9, 4, 1 along three orthogonal directions of six features, two constant columns, an offset"""
    rng = np.random.default_rng(seed)
    q = np.linalg.qr(rng.standard_normal((6, 6)))[0][:3]
    x = (rng.standard_normal((n, 3)) * np.array([3.0, 2.0, 1.0])) @ q + 0.01 * rng.standard_normal((n, 6)) + 5.0
    x = np.concatenate([x, np.full((n, 1), 2.5), x[:, :1] * 0.0], axis=1)
    return x.astype(np.float32)


@pytest.mark.parametrize('scaler', pca.SCALERS)
def test_fit_equals_the_restatement(scaler):
    x = _data()
    n = x.shape[0]
    m, lo, hi, g = _moments(x)
    s, comp, pcv = pca.fit(lo, hi, g, n, scaler, 4)
    rs, rcomp, rw, rshare = R.fit(lo, hi, g, n, scaler, 4)
    assert s.dtype == comp.dtype == pcv.dtype == np.float64 and comp.shape == (4, 8) and pcv.shape == (2, 4)
    np.testing.assert_array_equal(s, rs)
    if scaler == 'global':
        assert (s == hi.max() - lo.min()).all()
    if scaler in ('standard', 'minmax'):
        assert s[6] == 1.0 and s[7] == 1.0 and (s[:6] > 0).all()                 # the two constant columns
    np.testing.assert_allclose(pcv[0], rw, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(pcv[1], rshare, rtol=1e-12, atol=1e-14)
    assert (np.diff(pcv[0]) <= 0).all() and (pcv[0] >= 0).all() and pcv[1].sum() <= 1.0 + 1e-12
    np.testing.assert_allclose(comp @ comp.T, np.eye(4), atol=1e-12)           # unit and orthogonal
    for c in range(3):                                                          # the three planted directions, to a sign
        assert min(np.abs(comp[c] - rcomp[c]).max(), np.abs(comp[c] + rcomp[c]).max()) < 1e-10
    assert np.abs(comp[:3, 6:]).max() < 1e-12                                   # a constant column carries no variance
    if scaler == 'none':
        np.testing.assert_allclose(pcv[0][:3], [9.0, 4.0, 1.0], rtol=0.25)


def test_global_scaler_refuses_constant_data():
    with pytest.raises(ValueError, match='nothing to scale'):
        pca.scales('global', np.full(3, 2.0), np.full(3, 2.0), np.zeros((3, 3)), 5)


def test_negative_eigenvalues_of_round_off_size_are_clipped():
    """a rank-one Gram matrix with its null space perturbed below zero: eigh returns small negative eigenvalues"""
    v = np.array([3.0, -1.0, 2.0, 0.5])
    g = np.outer(v, v) * 7.0
    g -= 1e-15 * np.eye(4)
    assert np.linalg.eigvalsh(g).min() < 0.0
    s, comp, pcv = pca.fit(np.zeros(4), np.ones(4), g, 8, 'none', 4)
    assert (pcv[0] >= 0.0).all() and (pcv[0][1:] == 0.0).all() and pcv[0][0] > 0.0
    assert pcv[1][0] == 1.0 and (pcv[1][1:] == 0.0).all()
    rs, rcomp, rw, rshare = R.fit(np.zeros(4), np.ones(4), g, 8, 'none', 4)
    np.testing.assert_allclose(pcv[0], rw, rtol=1e-12, atol=0)
    s, comp, pcv = pca.fit(np.zeros(2), np.ones(2), np.zeros((2, 2)), 8, 'none', 2)     # no variance at all: shares are 0, not NaN
    assert (pcv == 0.0).all()


def test_sign_rule_flips_and_breaks_ties():
    comp = np.array([[0.6, -0.8, 0.0], [0.0, 0.6, -0.8], [-0.8, 0.8, 0.1], [0.5, 0.5, -0.5]])
    hot, cold = np.array([1.0, -2.0, 0.25, 0.0]), np.array([-1.0, 2.0, 0.25, 0.0])
    sign = pca.orient(comp, hot, cold)
    # hot above cold: kept; below: flipped; equal: the largest entry positive, the FIRST of equal magnitudes decides
    np.testing.assert_array_equal(sign, [1.0, -1.0, -1.0, 1.0])
    T = np.array([0.5, 2.0, 1.0])                                                # the hottest column is index 1, the coldest 0
    z = np.zeros((2, 3, 5, 4))
    z[:, 1] = hot
    z[:, 0] = cold
    z[:, 2] = 99.0
    np.testing.assert_array_equal(R.orient(comp, z, T), sign)


# ---- the command line
def _write_grid(tmp_path, pn=2, tn=3, sn=6, feat=(2, 2)):
    prefix = str(tmp_path / 'pc.lj.fcc.lammps')
    rng = np.random.default_rng(1)
    np.save(prefix + '.virial.trgt.npy', np.linspace(1, 2, pn, dtype=np.float32))
    np.save(prefix + '.temp.trgt.npy', np.linspace(1, 2, tn, dtype=np.float32))
    np.save(prefix + '.pe.npy', rng.random((pn, tn, sn)).astype(np.float32))
    np.save(prefix + '.cdf.npy', rng.random((pn, tn, sn) + feat).astype(np.float32))
    return prefix


def test_cli_refusals_leave_nothing_written(tmp_path, monkeypatch):
    prefix = _write_grid(tmp_path)
    monkeypatch.chdir(tmp_path)
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(SystemExit, match=r'pc\.lj\.fcc\.lammps\.rdf\.npy is missing'):
        pca.main(['-n', 'pc', '-ft', 'rdf'])
    np.save(prefix + '.adf.npy', np.zeros((3, 3, 6, 4), dtype=np.float32))
    with pytest.raises(SystemExit, match=r'adf\.npy has shape \(3, 3, 6, 4\)'):
        pca.main(['-n', 'pc', '-ft', 'adf'])
    np.save(prefix + '.sf.npy', np.zeros((2, 3, 6), dtype=np.float32))           # no feature axis
    with pytest.raises(SystemExit, match=r'sf\.npy has shape'):
        pca.main(['-n', 'pc', '-ft', 'sf'])
    with pytest.raises(SystemExit, match=r'-ld 5 is more than the 4 features of .*cdf\.npy'):
        pca.main(['-n', 'pc', '-ld', '5'])
    with pytest.raises(SystemExit, match=r'-sk 6 -sd 1 leave 0 samples of .*cdf\.npy'):
        pca.main(['-n', 'pc', '-ld', '2', '-sk', '6'])
    os.remove(prefix + '.pe.npy')
    with pytest.raises(SystemExit, match=r'pe\.npy is missing'):
        pca.main(['-n', 'pc', '-ld', '2'])
    assert sorted(os.listdir(tmp_path)) == sorted(set(before + ['pc.lj.fcc.lammps.adf.npy', 'pc.lj.fcc.lammps.sf.npy']) - {'pc.lj.fcc.lammps.pe.npy'})


def test_cli_flags():
    a = pca.parse_args([])
    assert (a.feature, a.scaler, a.latent_dimension, a.skip, a.stride, a.device) == ('cdf', 'global', 8, 0, 1, 0)
    a = pca.parse_args(['-ft', 'rdf', '-sc', 'standard', '-ld', '3', '-sk', '5', '-sd', '2', '-dv', '1', '-n', 'x', '-e', 'Al', '-v'])
    assert (a.feature, a.scaler, a.latent_dimension, a.skip, a.stride, a.device, a.name, a.element, a.verbose) == (
        'rdf', 'standard', 3, 5, 2, 1, 'x', 'Al', True)
    for bad in (['-sk', '-1'], ['-sd', '0'], ['-ld', '0'], ['-ld', '65'], ['-sc', 'tanh']):
        with pytest.raises(SystemExit):
            pca.parse_args(bad)
