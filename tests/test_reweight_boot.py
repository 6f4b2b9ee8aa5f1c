"""Block-bootstrap replicates of the reweighting (include/nm_reweight_boot.h) without a GPU: the C-ABI's declaration, export,
binding and refusals (which precede the device check and leave the outputs alone); the longdouble restatement
tests/reweight_boot_ref.py against reweight_ref on all-ones multiplicities and on a materialised multiset; the statistical
inefficiency, the block multiplicities and the flags of the command-line stage."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import reweight_boot_ref as BR
import reweight_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import reweight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -7.25e300
U16P = C.POINTER(C.c_uint16)


def test_header_declares_exactly_two_functions_exported_and_bound():
    txt = open(os.path.join(ROOT, 'include', 'nm_reweight_boot.h')).read()
    assert '#include "nm_reweight.h"' in txt
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    syms = sorted(set(re.findall(r'\b(nm_[a-z_0-9]+)\s*\(', txt)))
    assert syms == sorted(B.REWEIGHT_BOOT_SYMBOLS) == ['nm_reweight_boot_expect', 'nm_reweight_boot_solve']
    raw = C.CDLL(B.LIB_PATH)
    for s in syms:
        assert hasattr(raw, s), s
    L = B.load()
    assert L.nm_reweight_boot_solve.restype is C.c_int and len(L.nm_reweight_boot_solve.argtypes) == 17
    assert L.nm_reweight_boot_expect.restype is C.c_int and len(L.nm_reweight_boot_expect.argtypes) == 22


# ---- the raw ABI on sentinel-filled outputs
def base():
    rng = np.random.default_rng(11)
    return dict(b=np.array([1.0, 1.2, 1.5]), c=np.array([0.5, 0.6, 0.7]), count=np.array([3, 0, 5], dtype=np.int64),
                e=rng.gamma(4.0, 1.0, 8), v=rng.gamma(3.0, 1.0, 8), f=np.array([0.0, 0.5, 1.0]), tb=np.array([1.1, 1.3]),
                tc=np.array([0.55, 0.65]), obs=rng.random((2, 8)),
                mult=np.array([[1] * 8, [2, 0, 1, 1, 3, 0, 0, 1]], dtype=np.uint16), fr=np.array([[0.0, 0.5, 1.0], [0.0, 0.6, 0.9]]))


def _p(a, null, key, typ=B.c_double_p):
    return None if key in null else a.ctypes.data_as(typ)


def call_boot_solve(a, device=0, nstates=None, nsamples=None, nrep=None, tol=1e-9, max_iter=5, null=()):
    L = B.load()
    nr = a['mult'].shape[0]
    fr, delta = np.full((nr, a['b'].size), SENT), np.full(nr, SENT)
    iters, status = np.full(nr, -77, dtype=np.intc), np.full(nr, -77, dtype=np.intc)
    rc = L.nm_reweight_boot_solve(device, a['b'].size if nstates is None else nstates, _p(a['b'], null, 'b'), _p(a['c'], null, 'c'),
                                  _p(a['count'], null, 'count', B.c_int64_p), a['e'].size if nsamples is None else nsamples,
                                  _p(a['e'], null, 'e'), _p(a['v'], null, 'v'), _p(a['f'], null, 'f'), nr if nrep is None else nrep,
                                  _p(a['mult'], null, 'mult', U16P), tol, max_iter, _p(fr, null, 'fr'), _p(iters, null, 'iters', B.c_int_p),
                                  _p(delta, null, 'delta'), _p(status, null, 'status', B.c_int_p))
    untouched = (fr == SENT).all() and (delta == SENT).all() and (iters == -77).all() and (status == -77).all()
    return rc, (L.nm_reweight_last_error().decode() if rc else ''), untouched


def call_boot_expect(a, device=0, nstates=None, nsamples=None, nrep=None, ntargets=None, nobs=2, null=()):
    L = B.load()
    nr, nt = a['mult'].shape[0], a['tb'].size
    out = dict(tf=np.full((nr, nt), SENT), ess=np.full((nr, nt), SENT), mean=np.full((nr, nt, 2), SENT), cov=np.full((nr, nt, 3), SENT),
               omean=np.full((nr, nt, 8), SENT))
    rc = L.nm_reweight_boot_expect(device, a['b'].size if nstates is None else nstates, _p(a['b'], null, 'b'), _p(a['c'], null, 'c'),
                                   _p(a['count'], null, 'count', B.c_int64_p), _p(a['f'], null, 'f'),
                                   a['e'].size if nsamples is None else nsamples, _p(a['e'], null, 'e'), _p(a['v'], null, 'v'),
                                   nr if nrep is None else nrep, _p(a['mult'], null, 'mult', U16P), _p(a['fr'], null, 'fr'),
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
    'nrep0': dict(nrep=0), 'nrep-1': dict(nrep=-1), 'nrep1025': dict(nrep=1025), 'null-mult': dict(null=('mult',)),
    'null-fr': dict(null=('fr',)), 'mult-sum-low': dict(change=_with('mult', (1, 0), 1)), 'mult-sum-high': dict(change=_with('mult', (0, 7), 2)),
}
SOLVE_ONLY = {
    'tol-negative': dict(tol=-1e-300), 'tol-nan': dict(tol=np.nan), 'max_iter0': dict(max_iter=0), 'max_iter-3': dict(max_iter=-3),
    'null-iters': dict(null=('iters',)), 'null-delta': dict(null=('delta',)), 'null-status': dict(null=('status',)),
}
EXPECT_ONLY = {
    'ntargets0': dict(ntargets=0), 'ntargets65537': dict(ntargets=65537), 'nobs-1': dict(nobs=-1), 'nobs9': dict(nobs=9),
    'tb-nan': dict(change=_with('tb', 1, np.nan)), 'tc-inf': dict(change=_with('tc', 0, np.inf)), 'null-tb': dict(null=('tb',)),
    'null-tc': dict(null=('tc',)), 'null-tf': dict(null=('tf',)), 'null-ess': dict(null=('ess',)), 'null-mean': dict(null=('mean',)),
    'null-cov': dict(null=('cov',)), 'null-obs': dict(null=('obs',)), 'null-omean': dict(null=('omean',)),
    'fr-inf': dict(change=_with('fr', (1, 2), np.inf)), 'fr-minus-inf': dict(change=_with('fr', (0, 0), -np.inf)),
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
def test_boot_solve_refusals_precede_the_device_check(case):
    _refused(call_boot_solve, {**COMMON, **SOLVE_ONLY}, case)


@pytest.mark.parametrize('case', sorted({**COMMON, **EXPECT_ONLY}))
def test_boot_expect_refusals_precede_the_device_check(case):
    _refused(call_boot_expect, {**COMMON, **EXPECT_ONLY}, case)


def test_valid_calls_and_a_nan_in_fr_pass_the_argument_checks():
    """NM_ERR_HIP where the library finds no device (outputs untouched, no host fallback), NM_OK where it finds one; a NaN in fr
    is not a refusal"""
    a = base()
    seen = set()
    for fn, name in ((call_boot_solve, 'nm_reweight_boot_solve'), (call_boot_expect, 'nm_reweight_boot_expect')):
        rc, msg, untouched = fn(a)
        assert rc in (B.NM_OK, B.NM_ERR_HIP), msg
        seen.add(rc)
        if rc == B.NM_ERR_HIP:
            assert msg.startswith(name + ':') and 'no HIP device' in msg and untouched
    assert len(seen) == 1
    _with('fr', (1, 1), np.nan)(a)
    rc, msg, _ = call_boot_expect(a, nobs=0, null=('obs', 'omean'))
    assert {rc} == seen, msg
    if seen == {B.NM_ERR_HIP}:
        with pytest.raises(RuntimeError, match='nm_reweight_boot_solve'):
            reweight.boot_solve(a['b'], a['c'], a['count'], a['e'], a['v'], a['f'], a['mult'])
        with pytest.raises(RuntimeError, match='nm_reweight_boot_expect'):
            reweight.boot_expect(a['b'], a['c'], a['count'], a['f'], a['e'], a['v'], a['mult'], a['fr'], a['tb'], a['tc'])


# ---- the restatement
def _small(k, n, seed):
    rng = np.random.default_rng(seed)
    b, c = np.sort(1.0 + 0.5 * rng.random(k)), 0.5 + 0.3 * rng.random(k)
    e, v = rng.gamma(4.0, 1.0, n), rng.gamma(3.0, 1.0, n)
    count = np.bincount(rng.integers(0, k, n), minlength=k).astype(np.int64)
    return b, c, count, e, v, rng.normal(0.0, 0.5, k), rng


def test_restatement_with_all_ones_is_the_map_of_reweight_ref():
    b, c, count, e, v, f, _ = _small(5, 257, 1)
    got, _ = BR.apply_map(b, c, count, f, e, v, np.ones(257, dtype=np.uint16))
    want, _ = R.apply_map(b, c, count, f, e, v)
    assert float(np.abs(got - want).max()) <= 16 * 2.0 ** -64 * 257
    tb, tc = np.array([1.1, 1.4]), np.array([0.6, 0.7])
    obs = np.stack([e * e, np.ones(257)])
    x, y = BR.expect(b, c, count, f, e, v, np.ones(257), tb, tc, obs), R.expect(b, c, count, f, e, v, tb, tc, obs)
    for key in y:
        assert float(np.abs(x[key] - y[key]).max()) <= 1e-15 * max(1.0, float(np.abs(y[key]).max())), key


def test_restatement_equals_the_materialised_multiset():
    """np.repeat(samples, mult) with the SAME counts: logd of a sample does not depend on the multiset, F sums over it.  The
    materialised problem centres on other means, which moves nothing in exact arithmetic."""
    b, c, count, e, v, f, rng = _small(6, 300, 2)
    mult = rng.multinomial(300, np.full(300, 1 / 300)).astype(np.uint16)
    assert (mult == 0).any() and mult.max() > 1
    got, _ = BR.apply_map(b, c, count, f, e, v, mult)
    want, _ = R.apply_map(b, c, count, f, np.repeat(e, mult), np.repeat(v, mult))
    assert float(np.abs(got - want).max()) <= 1e-15
    tb, tc = np.array([1.2]), np.array([0.65])
    obs = rng.normal(size=(1, 300))
    x = BR.expect(b, c, count, f, e, v, mult, tb, tc, obs)
    y = R.expect(b, c, count, f, np.repeat(e, mult), np.repeat(v, mult), tb, tc, np.repeat(obs, mult, axis=1))
    for key in y:
        assert float(np.abs(x[key] - y[key]).max()) <= 1e-14 * max(1.0, float(np.abs(y[key]).max())), key
    # the float64 iteration of the restatement counts as the longdouble one does
    base, _ = R.solve(b, c, count, f, e, v)
    exact, inexact = BR.solve(b, c, count, base, e, v, mult), BR.solve(b, c, count, base, e, v, mult, exact=False)
    assert abs(len(exact[0]) - len(inexact[0])) <= 1 and exact[1][-1] <= 1e-12 and 2 <= len(exact[0]) < 50
    assert float(np.abs(exact[0][-1] - inexact[0][-1]).max()) <= 1e-11


# ---- the stage's host arithmetic
def _ar1(n, rho, seed):
    rng = np.random.default_rng(seed)
    x = np.zeros(n)
    for i in range(1, n):
        x[i] = rho * x[i - 1] + rng.normal()
    return x


@pytest.mark.parametrize('n,rho,seed', ((200, 0.0, 1), (300, 0.8, 2), (257, 0.95, 3), (2, 0.5, 4)))
def test_statistical_inefficiency_against_the_plain_sum(n, rho, seed):
    x = _ar1(n, rho, seed)
    got, want = reweight.statistical_inefficiency(x), BR.inefficiency(x)
    assert got >= 1.0 and abs(got - want) <= 1e-12 * want
    if rho >= 0.8:
        assert got > 2.0


def test_statistical_inefficiency_exact_cases():
    assert reweight.statistical_inefficiency(np.full(50, 3.5)) == 1.0
    assert reweight.statistical_inefficiency(np.array([1.0, -1.0] * 25)) == 1.0
    assert reweight.statistical_inefficiency(np.array([2.0])) == 1.0
    assert BR.inefficiency([3.5] * 9) == BR.inefficiency([1.0, -1.0] * 9) == BR.inefficiency([2.0]) == 1.0


def test_block_multiplicities():
    sn, L = 101, np.array([1, 7, 101, 5000, 13])
    m = reweight.block_multiplicities(sn, L, 6, 42)
    assert m.shape == (6, 5, sn) and m.dtype == np.uint16
    assert (m.astype(np.int64).sum(axis=2) == sn).all()
    assert m.tobytes() == reweight.block_multiplicities(sn, L, 6, 42).tobytes()
    assert m.tobytes() != reweight.block_multiplicities(sn, L, 6, 43).tobytes()
    assert (m[:, 2] == 1).all() and (m[:, 3] == 1).all()                # L >= sn: the series itself
    assert (m[:, 1] != 1).any()
    # blocks of 7: a drawn sample's circular run of drawn samples is at least 7 long unless the cut at sn draws shortened the last block
    one = reweight.block_multiplicities(sn, 7, 1, 5)
    assert one.shape == (1, 1, sn)
    # L = 1: every draw is a start of its own, so the counts are the histogram of the starts, in the generator's order
    rng = np.random.Generator(np.random.Philox(9))
    want = np.stack([np.bincount(rng.integers(0, 50, 50), minlength=50) for _ in range(3)])
    assert np.array_equal(reweight.block_multiplicities(50, 1, 3, 9)[:, 0], want)
    # a scalar L is one series
    assert reweight.block_multiplicities(10, 10, 2, 0).tolist() == [[[1] * 10]] * 2
    for bad in (dict(sn=0, L=1, nrep=1), dict(sn=5, L=0, nrep=1), dict(sn=5, L=1, nrep=0)):
        with pytest.raises(ValueError):
            reweight.block_multiplicities(seed=1, **bad)


def test_block_multiplicities_refuse_a_count_above_uint16(monkeypatch):
    monkeypatch.setattr(reweight, '_draw_starts', lambda rng, sn, nb: np.zeros(nb, dtype=np.int64))
    assert reweight.block_multiplicities(65535, 1, 1, 0)[0, 0, 0] == 65535
    with pytest.raises(ValueError, match='65535'):
        reweight.block_multiplicities(65536, 1, 1, 0)


def test_bootstrap_flags():
    a = reweight.parse_args([])
    assert (a.bootstrap, a.block_length, a.bootstrap_seed) == (0, 0, 256)
    a = reweight.parse_args(['-bs', '1024', '-bl', '9', '-bd', '7'])
    assert (a.bootstrap, a.block_length, a.bootstrap_seed) == (1024, 9, 7)
    ob7, ob8 = ['-ob'] + ['x'] * 7, ['-ob'] + ['x'] * 8
    assert reweight.parse_args(['-bs', '4', '-hq', 'pe', '-hx', '0.5'] + ob7).bootstrap == 4
    assert len(reweight.parse_args(['-hq', 'pe', '-hx', '0.5'] + ob8).observables) == 8       # without -bs eight names stay allowed
    assert len(reweight.parse_args(['-bs', '4', '-hq', 'pe'] + ob8).observables) == 8         # and without -hx
    for bad in (['-bs', '-1'], ['-bs', '1025'], ['-bl', '-1'], ['-bs', '4', '-hq', 'pe', '-hx', '0.5'] + ob8):
        with pytest.raises(SystemExit):
            reweight.parse_args(bad)


def test_boot_spreads_of_identical_replicates_are_zero():
    pn, tn, tg, natoms, nrep = 2, 3, 5, 32, 4
    tfine = np.linspace(0.5, 1.5, tg)
    tb = np.tile(1.0 / tfine, (pn, 1))
    tc = np.array([[2.0], [4.0]]) * tb
    rng = np.random.default_rng(3)
    one = dict(tf=rng.random(pn * tg), ess=rng.random(pn * tg) * 100, mean=rng.random((pn * tg, 2)) * 10, cov=rng.random((pn * tg, 3)),
               omean=np.stack([rng.random(pn * tg), np.tile(np.linspace(0.1, 0.9, tg), pn)], axis=1))
    ex = {key: np.stack([val] * nrep) for key, val in one.items()}
    fr = np.stack([rng.random((pn, tn))] * nrep)
    fr[2] = np.nan
    for key in ex:
        ex[key][2] = np.nan
    out = reweight.boot_spreads(fr, np.array([0, 1, 2, 0]), tfine, tb, tc, ex, natoms, 1, True)
    assert sorted(out) == ['rwcs', 'rwes', 'rwfs', 'rwgs', 'rwhs', 'rwms', 'rwos', 'rwvs']
    for key in ('rwfs', 'rwgs', 'rwhs', 'rwvs', 'rwcs', 'rwos'):
        assert (out[key] <= 1e-14).all(), key                         # the mean of equal numbers rounds: not exactly 0
    assert out['rwfs'].shape == (pn, tn) and out['rwgs'].shape == (pn, tg) and out['rwos'].shape == (pn, tg, 1)
    assert out['rwms'].shape == out['rwes'].shape == (pn, 4)
    assert (out['rwms'][:, 0] <= 1e-14).all() and (out['rwms'][:, 3] == 3).all()      # the status-2 replicate is left out
    assert (out['rwes'][:, 3] == 3).all() and np.allclose(out['rwes'][:, 1], 1.0) and np.allclose(out['rwes'][:, 2], 1.0)
    # a replicate without a crossing is left out of .rwes and counted
    ex['omean'][3, :, 1] = 0.9
    out = reweight.boot_spreads(fr, np.array([0, 1, 2, 0]), tfine, tb, tc, ex, natoms, 1, True)
    assert (out['rwes'][:, 3] == 2).all() and (out['rwms'][:, 3] == 3).all()
