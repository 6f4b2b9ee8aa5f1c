"""Multistate reweighting (include/nm_reweight.h) without a GPU: the C-ABI's declaration, export, binding and refusals (which
precede the device check and leave the outputs alone); the longdouble restatement tests/reweight_ref.py against the Gamma known
answer; the host arithmetic of the command-line stage."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import reweight_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import remcmc, reweight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -7.25e300


def test_header_symbols_are_exported_and_bound():
    txt = open(os.path.join(ROOT, 'include', 'nm_reweight.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    syms = sorted(set(re.findall(r'\b(nm_[a-z_0-9]+)\s*\(', txt)))
    assert syms == sorted(B.REWEIGHT_SYMBOLS) and len(syms) == 3
    raw = C.CDLL(B.LIB_PATH)
    for s in syms:
        assert hasattr(raw, s), s
    L = B.load()
    assert L.nm_reweight_solve.restype is C.c_int and len(L.nm_reweight_solve.argtypes) == 14
    assert L.nm_reweight_expect.restype is C.c_int and len(L.nm_reweight_expect.argtypes) == 19
    assert L.nm_reweight_last_error.restype is C.c_char_p


# ---- the raw ABI on sentinel-filled outputs
def base():
    rng = np.random.default_rng(11)
    return dict(b=np.array([1.0, 1.2, 1.5]), c=np.array([0.5, 0.6, 0.7]), count=np.array([3, 0, 5], dtype=np.int64),
                e=rng.gamma(4.0, 1.0, 8), v=rng.gamma(3.0, 1.0, 8), f=np.array([0.0, 0.5, 1.0]), tb=np.array([1.1, 1.3]),
                tc=np.array([0.55, 0.65]), obs=rng.random((2, 8)))


def _p(a, null, key, typ=B.c_double_p):
    return None if key in null else a.ctypes.data_as(typ)


def call_solve(a, device=0, nstates=None, nsamples=None, tol=1e-9, max_iter=5, null=()):
    L = B.load()
    f = np.array(a['f'], dtype=np.float64)
    logd = np.full(a['e'].size, SENT)
    iters, delta = C.c_int(-77), C.c_double(SENT)
    rc = L.nm_reweight_solve(device, a['b'].size if nstates is None else nstates, _p(a['b'], null, 'b'), _p(a['c'], null, 'c'),
                             _p(a['count'], null, 'count', B.c_int64_p), a['e'].size if nsamples is None else nsamples,
                             _p(a['e'], null, 'e'), _p(a['v'], null, 'v'), tol, max_iter, _p(f, null, 'f'), _p(logd, null, 'logd'),
                             None if 'iters' in null else C.byref(iters), None if 'delta' in null else C.byref(delta))
    untouched = (np.array_equal(f, a['f'], equal_nan=True) and (logd == SENT).all() and iters.value == -77 and delta.value == SENT)
    return rc, (L.nm_reweight_last_error().decode() if rc else ''), untouched


def call_expect(a, device=0, nstates=None, nsamples=None, ntargets=None, nobs=2, null=()):
    L = B.load()
    nt = a['tb'].size
    out = dict(tf=np.full(nt, SENT), ess=np.full(nt, SENT), mean=np.full((nt, 2), SENT), cov=np.full((nt, 3), SENT),
               omean=np.full((nt, 8), SENT))
    rc = L.nm_reweight_expect(device, a['b'].size if nstates is None else nstates, _p(a['b'], null, 'b'), _p(a['c'], null, 'c'),
                              _p(a['count'], null, 'count', B.c_int64_p), _p(a['f'], null, 'f'),
                              a['e'].size if nsamples is None else nsamples, _p(a['e'], null, 'e'), _p(a['v'], null, 'v'),
                              nt if ntargets is None else ntargets, _p(a['tb'], null, 'tb'), _p(a['tc'], null, 'tc'), nobs,
                              _p(a['obs'], null, 'obs'), _p(out['tf'], null, 'tf'), _p(out['ess'], null, 'ess'),
                              _p(out['mean'], null, 'mean'), _p(out['cov'], null, 'cov'), _p(out['omean'], null, 'omean'))
    untouched = all((x == SENT).all() for x in out.values())
    return rc, (L.nm_reweight_last_error().decode() if rc else ''), untouched


def _with(key, index, value):
    def change(a):
        a[key] = a[key].copy()
        a[key][index] = value
    return change


COMMON = {
    'nstates0': dict(nstates=0), 'nstates4097': dict(nstates=4097), 'nsamples0': dict(nsamples=0), 'nsamples-1': dict(nsamples=-1),
    'count-negative': dict(change=lambda a: a.update(count=np.array([9, -1, 0], dtype=np.int64))),
    'count-sum-low': dict(change=_with('count', 0, 2)), 'count-sum-high': dict(change=_with('count', 1, 1)),
    'count-overflow': dict(change=lambda a: a.update(count=np.array([2 ** 62, 2 ** 62, 8], dtype=np.int64))),
    'b-nan': dict(change=_with('b', 1, np.nan)), 'c-inf': dict(change=_with('c', 2, np.inf)), 'e-inf': dict(change=_with('e', 7, -np.inf)),
    'v-nan': dict(change=_with('v', 0, np.nan)), 'f-nan': dict(change=_with('f', 2, np.nan)), 'f-inf': dict(change=_with('f', 0, np.inf)),
    'null-b': dict(null=('b',)), 'null-c': dict(null=('c',)), 'null-count': dict(null=('count',)), 'null-e': dict(null=('e',)),
    'null-v': dict(null=('v',)), 'null-f': dict(null=('f',)), 'device-1': dict(device=-1),
}
SOLVE_ONLY = {
    'tol-negative': dict(tol=-1e-300), 'tol-nan': dict(tol=np.nan), 'max_iter0': dict(max_iter=0), 'max_iter-3': dict(max_iter=-3),
    'null-iters': dict(null=('iters',)), 'null-delta': dict(null=('delta',)),
}
EXPECT_ONLY = {
    'ntargets0': dict(ntargets=0), 'ntargets65537': dict(ntargets=65537), 'nobs-1': dict(nobs=-1), 'nobs9': dict(nobs=9),
    'tb-nan': dict(change=_with('tb', 1, np.nan)), 'tc-inf': dict(change=_with('tc', 0, np.inf)), 'null-tb': dict(null=('tb',)),
    'null-tc': dict(null=('tc',)), 'null-tf': dict(null=('tf',)), 'null-ess': dict(null=('ess',)), 'null-mean': dict(null=('mean',)),
    'null-cov': dict(null=('cov',)), 'null-obs': dict(null=('obs',)), 'null-omean': dict(null=('omean',)),
}


def _refused(fn, cases, case):
    kw = dict(cases[case])
    a = base()
    kw.pop('change', lambda a: None)(a)
    rc, msg, untouched = fn(a, **kw)
    assert rc == B.NM_ERR_ARG, (rc, msg)
    assert msg.startswith(fn.__name__.replace('call_', 'nm_reweight_') + ':'), msg
    assert untouched


@pytest.mark.parametrize('case', sorted({**COMMON, **SOLVE_ONLY}))
def test_solve_refusals_precede_the_device_check(case):
    _refused(call_solve, {**COMMON, **SOLVE_ONLY}, case)


@pytest.mark.parametrize('case', sorted({**COMMON, **EXPECT_ONLY}))
def test_expect_refusals_precede_the_device_check(case):
    _refused(call_expect, {**COMMON, **EXPECT_ONLY}, case)


def test_valid_calls_without_a_device_are_hip_errors():
    """NM_ERR_HIP where the library finds no device (outputs untouched, no host fallback), NM_OK where it finds one"""
    a = base()
    seen = set()
    for fn, name in ((call_solve, 'nm_reweight_solve'), (call_expect, 'nm_reweight_expect')):
        rc, msg, untouched = fn(a)
        assert rc in (B.NM_OK, B.NM_ERR_HIP), msg
        seen.add(rc)
        if rc == B.NM_ERR_HIP:
            assert msg.startswith(name + ':') and 'no HIP device' in msg and untouched
    assert len(seen) == 1                                               # both entries see the same machine
    rc, msg, _ = call_expect(a, nobs=0, null=('obs', 'omean'))          # both may be null without observables
    assert {rc} == seen, msg
    if seen == {B.NM_ERR_HIP}:
        with pytest.raises(RuntimeError, match='nm_reweight_solve'):
            reweight.solve(a['b'], a['c'], a['count'], a['e'], a['v'])
        with pytest.raises(RuntimeError, match='nm_reweight_expect'):
            reweight.expect(a['b'], a['c'], a['count'], a['f'], a['e'], a['v'], a['tb'], a['tc'])


# ---- the restatement
def test_restatement_gives_the_gamma_known_answer():
    """K = 6 overlapping Gamma states, 6000 samples per state (reweight_ref.gamma_set): the restatement's fixed point and its
    moments at the six states and the five points between them must lie within HALF the marks the GPU tests use (0.05 absolute in
    f, 5 % relative in the moments; cov_ev, whose exact value is 0, relative to sqrt(var_e var_v)).  Observed with 6000 per state:
    f 0.0178, means 0.52 %, variances 1.25 %, cov_ev 1.01 %; with 2000 per state the variances are off by 3.7 %, which is why the
    count is 6000."""
    b, c, count, e, v = R.gamma_set()
    assert count.tolist() == [6000] * 6
    f, _ = R.solve(b, c, count, R.gamma_start(b, c, count, e, v), e, v)
    assert f[0] == 0
    df = float(np.abs(f - R.gamma_exact_f()).max())
    tb, tc = R.gamma_targets()
    ex = R.expect(b, c, count, f, e, v, tb, tc)
    mean, cov = R.gamma_exact_moments(tb, tc)
    got_mean, got_cov = ex['mean'].astype(np.float64), ex['cov'].astype(np.float64)
    dm = float(np.abs(got_mean / mean - 1).max())
    dv = float(np.abs(got_cov[:, [0, 2]] / cov[:, [0, 2]] - 1).max())
    dc = float(np.abs(got_cov[:, 1] / np.sqrt(cov[:, 0] * cov[:, 2])).max())
    print('restatement against the known answer: f %.4f, means %.4f, variances %.4f, cov_ev %.4f' % (df, dm, dv, dc))
    assert df <= 0.025 and dm <= 0.025 and dv <= 0.025 and dc <= 0.025
    ess = ex['ess'].astype(np.float64)
    assert (ess <= e.size).all() and (ess[:6] >= 6000 / 6).all()
    # a fixed point: one more application moves it by rounding only
    again = R.apply_map(b, c, count, f, e, v)[0].astype(np.float64)
    assert float(np.abs(again - f).max()) <= 1e-12


def test_restatement_against_a_direct_float64_evaluation():
    """K = 3 (one state unsampled), N = 8: the definitions written out with explicit loops"""
    a = base()
    f_new, logd = R.apply_map(a['b'], a['c'], a['count'], a['f'], a['e'], a['v'])
    u = a['b'][:, None] * a['e'][None, :] + a['c'][:, None] * a['v'][None, :]
    want_ld = np.array([np.log(sum(a['count'][k] * np.exp(a['f'][k] - u[k, n]) for k in (0, 2))) for n in range(8)])
    big = np.array([-np.log(np.exp(-u[i] - want_ld).sum()) for i in range(3)])
    assert np.abs(logd.astype(np.float64) - want_ld).max() < 1e-13
    assert np.abs(f_new.astype(np.float64) - (big - big[0])).max() < 1e-13
    ex = R.expect(a['b'], a['c'], a['count'], a['f'], a['e'], a['v'], a['tb'], a['tc'], a['obs'])
    ut = a['tb'][1] * a['e'] + a['tc'][1] * a['v']
    w = np.exp(-ut - want_ld)
    assert abs(float(ex['tf'][1]) + np.log(w.sum())) < 1e-13
    w /= w.sum()
    assert abs(float(ex['ess'][1]) - 1 / (w * w).sum()) < 1e-12
    assert abs(float(ex['mean'][1, 0]) - (w * a['e']).sum()) < 1e-13
    assert abs(float(ex['cov'][1, 1]) - (w * (a['e'] - (w * a['e']).sum()) * (a['v'] - (w * a['v']).sum())).sum()) < 1e-13
    assert abs(float(ex['omean'][1, 1]) - (w * a['obs'][1]).sum()) < 1e-13
    assert R.tol_map(8, 3, 2.0) == (8 + 3 + 64) * 2.0 ** -53 + 32 * 2.0 ** -53


# ---- the stage's host arithmetic
@pytest.mark.parametrize('el', ('LJ', 'Al'))
def test_states_equal_init_constant(el):
    P = np.linspace(1, 8, 3, dtype=np.float32)
    T = np.linspace(0.25, 2.5, 4, dtype=np.float32) * (1 if el == 'LJ' else 400)
    b, c = reweight.states(P, T, el)
    assert b.shape == c.shape == (12,) and b.dtype == c.dtype == np.float64
    for i in range(3):
        for j in range(4):
            et, pf = remcmc.init_constant(P, T, el, i, j)
            assert b[i * 4 + j] == 1.0 / et and c[i * 4 + j] == pf
    tfine, tb, tc = reweight.fine_targets(P, T, el, 7)
    assert tfine.shape == (7,) and tb.shape == tc.shape == (3, 7)
    assert tfine[0] == float(T[0]) and tfine[-1] == float(T[-1])
    assert np.array_equal(tb[:, 0], b.reshape(3, 4)[:, 0]) and np.array_equal(tc[:, -1], c.reshape(3, 4)[:, -1])


def test_curves_map_known_moments_to_the_ten_arrays():
    pn, tg, natoms = 2, 5, 32
    tfine = np.linspace(0.5, 1.5, tg)
    tb = np.tile(1.0 / tfine, (pn, 1))
    tc = np.array([[2.0], [4.0]]) * tb
    rng = np.random.default_rng(3)
    ex = dict(tf=rng.random(pn * tg), ess=rng.random(pn * tg) * 100, mean=rng.random((pn * tg, 2)) * 10,
              cov=np.tile([2.0, 0.5, 1.0], (pn * tg, 1)), omean=rng.random((pn * tg, 2)))
    ex['cov'][3] = [50.0, 0.0, 0.0]            # row 0 peaks at the fine temperature 3
    ex['cov'][tg + 4] = [0.0, 0.0, 50.0]       # row 1 at its end: written as it is
    f = np.arange(6.0).reshape(2, 3)
    out = reweight.curves(f, 17, 3e-10, 1e-9, tfine, tb, tc, ex, natoms)
    assert sorted(out) == sorted(reweight.SUFFIXES) and len(out) == 10
    assert np.array_equal(out['rwf'], f) and out['rwi'].tolist() == [17.0, 3e-10, 1e-9] and np.array_equal(out['rwt'], tfine)
    assert np.array_equal(out['rwg'], ex['tf'].reshape(pn, tg)) and np.array_equal(out['rwn'], ex['ess'].reshape(pn, tg))
    mean = ex['mean'].reshape(pn, tg, 2)
    press = np.array([[2.0], [4.0]])
    np.testing.assert_allclose(out['rwh'], (mean[..., 0] + press * mean[..., 1]) / natoms, rtol=1e-15)
    np.testing.assert_allclose(out['rwv'], mean[..., 1] / natoms, rtol=1e-15)
    np.testing.assert_allclose(out['rwc'][0, 0], (2.0 + 2 * 2.0 * 0.5 + 4.0 * 1.0) * tb[0, 0] ** 2 / natoms, rtol=1e-15)
    np.testing.assert_allclose(out['rwc'][1, 4], 16.0 * tb[1, 4] ** 2 * 50.0 / natoms, rtol=1e-15)
    assert out['rwo'].shape == (pn, tg, 2) and np.array_equal(out['rwo'].reshape(-1, 2), ex['omean'])
    assert out['rwm'].tolist() == [tfine[3], tfine[4]]
    for key in reweight.SUFFIXES:
        assert out[key].dtype == np.float64


def _write_grid(tmp_path, pn=2, tn=4, sn=20):
    prefix = str(tmp_path / 'rw.lj.fcc.lammps')
    rng = np.random.default_rng(1)
    np.save(prefix + '.virial.trgt.npy', np.linspace(1, 2, pn, dtype=np.float32))
    np.save(prefix + '.temp.trgt.npy', np.linspace(1, 2, tn, dtype=np.float32))
    np.save(prefix + '.pe.npy', rng.random((pn, tn, sn)).astype(np.float32))
    np.save(prefix + '.vol.npy', rng.random((pn, tn, sn)).astype(np.float32))
    np.save(prefix + '.natoms.npy', np.full((pn, tn, sn), 32, dtype=np.uint16))
    return prefix


def test_cli_refuses_a_bad_observable_before_writing(tmp_path, monkeypatch):
    prefix = _write_grid(tmp_path)
    monkeypatch.chdir(tmp_path)
    before = sorted(os.listdir(tmp_path))
    with pytest.raises(SystemExit, match='sof.npy is missing'):
        reweight.main(['-n', 'rw', '-ob', 'sof'])
    np.save(prefix + '.sol.npy', np.zeros((2, 4, 19), dtype=np.float32))
    with pytest.raises(SystemExit, match='has shape'):
        reweight.main(['-n', 'rw', '-ob', 'sol'])
    assert sorted(os.listdir(tmp_path)) == sorted(before + ['rw.lj.fcc.lammps.sol.npy'])


def test_cli_flags(capsys):
    a = reweight.parse_args([])
    assert (a.skip, a.stride, a.temperature_grid, a.tolerance, a.max_iterations, a.observables) == (0, 1, 256, 1e-9, 20000, [])
    a = reweight.parse_args(['-sk', '5', '-sd', '2', '-tg', '16', '-rt', '1e-6', '-ri', '9', '-ob', 'sof', 'sol'])
    assert (a.skip, a.stride, a.temperature_grid, a.tolerance, a.max_iterations, a.observables) == (5, 2, 16, 1e-6, 9, ['sof', 'sol'])
    for bad in (['-sk', '-1'], ['-sd', '0'], ['-tg', '0'], ['-tg', '65537'], ['-ri', '0'], ['-rt', '-1'], ['-ob'] + ['x'] * 9):
        with pytest.raises(SystemExit):
            reweight.parse_args(bad)
    with pytest.raises(SystemExit):
        reweight.parse_args(['-h'])
    text = ' '.join(capsys.readouterr().out.split())
    assert 'kinetic 3/2 is NOT included' in text and 'not bracketed' in text and 'has not been measured' in text
