"""Block-bootstrap replicates on the GPU: nm_reweight_boot_solve and nm_reweight_boot_expect through the C-ABI on sentinel-filled
outputs, against the longdouble restatement tests/reweight_boot_ref.py, never against the library itself.

Tolerances.  One application of a replicate's map may deviate by 3 tol_map(N, K, U), tol_map = (N + K + 64) u + 16 u U of
reweight_ref: the two base quantities of the perturbative form (p through logd, and q) are each within tol_map, and the
non-negative sums over K and over N terms meet (N + K) u, inside a third (the kernel header derives the tighter (K + 45 +
N/2^18) u + ...).  Where e and v carry an offset of 1e6 the doubles that hold f are ~1e6: 4 u |value| more.  A max-norm change
d of f changes logd by at most d, F by at most d and the gauged result by at most 2 d: the restatement's map applied to a
returned fr[r] moves it by at most 2 delta[r] + 2 * 3 tol_map.  The expectations use the tolerances of tests/test_reweight_gpu.py
with tol_map replaced by 3 tol_map.
Condition.  Except in the no-overlap case no replicate may end with status 2; the restatement confirms for every
one-application input that every S_r[i] = exp(f[i] - F_r(f)[i]) stays above 1e-3 (the smallest seen was 0.76)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import reweight_boot_ref as BR
import reweight_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import reweight

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -7.25e300
KT, RT, CH, TGB = 128, 16, 4096, 256    # csrc/nm_reweight_boot.h: the weights kernel's state tile, the replicate tile; the chunk, the targets per launch
ECH = 4 * CH                            # the expectation kernel's own chunk
U16P = C.POINTER(C.c_uint16)


def dp(a):
    return a.ctypes.data_as(B.c_double_p)


def boot_solve(b, c, count, e, v, f, mult, tol=0.0, max_iter=1):
    """the raw ABI on sentinel-filled outputs: (fr, iters, delta, status)"""
    L = B.load()
    mult = np.ascontiguousarray(mult, dtype=np.uint16)
    nr = mult.shape[0]
    fr, delta = np.full((nr, b.size), SENT), np.full(nr, SENT)
    iters, status = np.full(nr, -77, dtype=np.intc), np.full(nr, -77, dtype=np.intc)
    count = np.ascontiguousarray(count, dtype=np.int64)
    rc = L.nm_reweight_boot_solve(0, b.size, dp(b), dp(c), count.ctypes.data_as(B.c_int64_p), e.size, dp(e), dp(v), dp(f), nr,
                                  mult.ctypes.data_as(U16P), tol, max_iter, dp(fr), iters.ctypes.data_as(B.c_int_p), dp(delta),
                                  status.ctypes.data_as(B.c_int_p))
    assert rc == B.NM_OK, L.nm_reweight_last_error().decode()
    assert not (fr == SENT).any() and not (delta == SENT).any() and (iters != -77).all() and (status != -77).all()
    return fr, iters, delta, status


def boot_expect(b, c, count, f, e, v, mult, fr, tb, tc, obs=None):
    L = B.load()
    mult = np.ascontiguousarray(mult, dtype=np.uint16)
    fr = np.ascontiguousarray(fr, dtype=np.float64)
    nr, nt, nobs = mult.shape[0], tb.size, 0 if obs is None else obs.shape[0]
    out = dict(tf=np.full((nr, nt), SENT), ess=np.full((nr, nt), SENT), mean=np.full((nr, nt, 2), SENT), cov=np.full((nr, nt, 3), SENT),
               omean=np.full((nr, nt, nobs), SENT))
    count = np.ascontiguousarray(count, dtype=np.int64)
    rc = L.nm_reweight_boot_expect(0, b.size, dp(b), dp(c), count.ctypes.data_as(B.c_int64_p), dp(f), e.size, dp(e), dp(v), nr,
                                   mult.ctypes.data_as(U16P), dp(fr), nt, dp(tb), dp(tc), nobs, dp(obs) if nobs else None, dp(out['tf']),
                                   dp(out['ess']), dp(out['mean']), dp(out['cov']), dp(out['omean']) if nobs else None)
    assert rc == B.NM_OK, L.nm_reweight_last_error().decode()
    for key, x in out.items():
        assert not (x == SENT).any(), key
    return out


def data(k, n, seed=0, empty=()):
    """k states, n Gamma samples; the states `empty` drew no sample (the generator of tests/test_reweight_gpu.py)"""
    rng = np.random.default_rng(1000 * k + n + seed)
    b = np.sort(1.0 + 0.5 * rng.random(k))
    c = 0.5 + 0.3 * rng.random(k)
    e, v = rng.gamma(4.0, 1.0, n), rng.gamma(3.0, 1.0, n)
    pick = np.array([s for s in range(k) if s not in empty])
    count = np.bincount(pick[rng.integers(0, pick.size, n)], minlength=k).astype(np.int64)
    f0 = rng.normal(0.0, 0.5, k)
    return b, c, count, e, v, f0


def resample(n, nrep, seed):
    """ordinary bootstrap multiplicities (nrep, n)"""
    rng = np.random.default_rng(seed)
    return np.stack([np.bincount(rng.integers(0, n, n), minlength=n) for _ in range(nrep)]).astype(np.uint16)


_BASE = {}


def base_solution(key, b, c, count, e, v, f0):
    """the restatement's converged solution rounded to float64, computed once per set"""
    if key not in _BASE:
        _BASE[key] = R.solve(b, c, count, f0, e, v)[0]
    return _BASE[key]


def first_chunk_only(n):
    m = np.zeros(n, dtype=np.uint16)
    m[:CH] = n // CH
    return m


def one_sample(n):
    m = np.zeros(n, dtype=np.uint16)
    m[n // 2 + 17] = n
    return m


# ---- one application of the map
MAP_CASES = {
    'K1': dict(k=1, n=1009), 'K2': dict(k=2, n=1009), 'K5': dict(k=5, n=1009), 'two-states-without-samples': dict(k=6, n=1009, empty=(0, 3)),
    'K129-above-the-state-tile': dict(k=KT + 1, n=1009), 'N1': dict(k=5, n=1), 'N257': dict(k=5, n=257), 'N4095': dict(k=5, n=CH - 1),
    'N4096': dict(k=5, n=CH), 'N4097': dict(k=5, n=CH + 1), 'R1': dict(k=5, n=1009, nrep=1),
    'R17-above-the-replicate-tile': dict(k=5, n=1009, nrep=RT + 1),
    'N8192-K1-empty-chunk-and-one-sample': dict(k=1, n=2 * CH, special=True),
    'N8192-K5-empty-chunk-and-one-sample': dict(k=5, n=2 * CH, special=True),
    'offsets-of-a-million': dict(k=5, n=1009, shift=(-1e6, 1e6)),
}


@pytest.mark.parametrize('case', sorted(MAP_CASES))
def test_one_application_of_the_map(case):
    kw = dict(MAP_CASES[case])
    nrep, special, shift = kw.pop('nrep', 3), kw.pop('special', False), kw.pop('shift', None)
    b, c, count, e, v, f0 = data(**kw)
    if shift:
        e, v = e + shift[0], v + shift[1]
    k, n = b.size, e.size
    f = base_solution(case, b, c, count, e, v, f0)
    mult = resample(n, nrep, 77 + n)
    if special:
        mult = np.stack([first_chunk_only(n), one_sample(n), mult[0]])
        assert mult[0, CH:].sum() == 0 and (mult[1] > 0).sum() == 1 and mult[1].max() == n
    fr, iters, delta, status = boot_solve(b, c, count, e, v, f, mult)
    u_max = R.u_max(b, c, e, v)
    tol = 3 * R.tol_map(n, k, u_max) + (4 * R.UNIT * np.abs(f).max() if shift else 0.0)
    worst, smin = 0.0, np.inf
    for r in range(mult.shape[0]):
        want, big = BR.apply_map(b, c, count, f, e, v, mult[r])
        smin = min(smin, float(np.exp(f.astype(R.LD) - big).min()))
        worst = max(worst, float(np.abs(fr[r].astype(R.LD) - want).max()))
        assert abs(delta[r] - float(np.abs(want - f.astype(R.LD)).max())) <= 2 * tol
    print('%s: |dfr| = %.3g (tolerance %.3g), U = %.3g, smallest S = %.3g' % (case, worst, tol, u_max, smin))
    assert smin > 1e-3                                                  # the condition under which status 2 may not occur
    assert (iters == 1).all() and (fr[:, 0] == 0.0).all() and np.isfinite(fr).all() and np.isfinite(delta).all()
    assert ((status == 0) | (status == 1)).all() and ((status == 0) == (delta <= 0.0)).all()
    assert worst <= tol
    if k == 1:
        assert (fr == 0.0).all() and (delta == 0.0).all() and (status == 0).all()


# ---- the converged replicates
CONVERGED = {'K5-N1009': dict(k=5, n=1009, exact=True), 'K64-N8193': dict(k=64, n=8193, exact=False)}
_CONV = {}


def converged(case):
    """the set, its base solution, block-bootstrap multiplicities with replicate 4 all ones, and one call to convergence"""
    if case not in _CONV:
        kw = dict(CONVERGED[case])
        exact = kw.pop('exact')
        b, c, count, e, v, f0 = data(**kw)
        k, n = b.size, e.size
        f = base_solution('conv-' + case, b, c, count, e, v, f0)
        mult = reweight.block_multiplicities(n, 5, 9, 256)[:, 0]          # one series of n samples, blocks of 5
        mult[4] = 1
        got = boot_solve(b, c, count, e, v, f, mult, tol=1e-12, max_iter=200)
        _CONV[case] = dict(b=b, c=c, count=count, e=e, v=v, f=f, mult=mult, got=got, exact=exact, tol=3 * R.tol_map(n, k, R.u_max(b, c, e, v)))
    return _CONV[case]


@pytest.mark.parametrize('case', sorted(CONVERGED))
def test_converged_replicates_are_fixed_points_of_the_restatement(case):
    s = converged(case)
    fr, iters, delta, status = s['got']
    assert (status == 0).all() and (delta <= 1e-12).all() and (iters >= 1).all() and (iters < 200).all()
    for r in range(9):
        again = BR.apply_map(s['b'], s['c'], s['count'], fr[r], s['e'], s['v'], s['mult'][r])[0]
        res = float(np.abs(again - fr[r].astype(R.LD)).max())
        ref_iters = len(BR.solve(s['b'], s['c'], s['count'], s['f'], s['e'], s['v'], s['mult'][r], tol=1e-12, max_iter=200, exact=s['exact'])[0])
        print('%s replicate %d: %d iterations (restatement %d), delta %.3g, residual %.3g (bound %.3g), |fr - f| = %.3g' % (
            case, r, iters[r], ref_iters, delta[r], res, 2 * delta[r] + 2 * s['tol'], np.abs(fr[r] - s['f']).max()))
        assert res <= 2 * delta[r] + 2 * s['tol']
        assert abs(int(iters[r]) - ref_iters) <= 1
    assert (np.abs(fr - s['f'][None, :]).max(axis=1)[[0, 1, 2, 3, 5, 6, 7, 8]] > 1e-6).all()     # the resampled ones did move


@pytest.mark.parametrize('case', sorted(CONVERGED))
def test_the_all_ones_replicate_is_the_base_solution_and_is_frozen(case):
    s = converged(case)
    fr, iters, delta, status = s['got']
    assert np.abs(fr[4] - s['f']).max() <= 2 * delta[4] + 2 * s['tol']
    assert iters[4] < iters.max()                                         # the others went on after it had stopped
    alone = boot_solve(s['b'], s['c'], s['count'], s['e'], s['v'], s['f'], s['mult'][4:5], tol=1e-12, max_iter=200)
    assert alone[0][0].tobytes() == fr[4].tobytes() and alone[1][0] == iters[4] and alone[2][0] == delta[4] and alone[3][0] == 0


def test_max_iter_reached_returns_the_second_iterate():
    s = converged('K5-N1009')
    fr, iters, delta, status = boot_solve(s['b'], s['c'], s['count'], s['e'], s['v'], s['f'], s['mult'], tol=1e-12, max_iter=2)
    moved = [r for r in range(9) if r != 4]
    assert (status[moved] == 1).all() and (iters[moved] == 2).all() and (delta[moved] > 1e-12).all()
    for r in moved:
        its, deltas = BR.solve(s['b'], s['c'], s['count'], s['f'], s['e'], s['v'], s['mult'][r], tol=1e-12, max_iter=2)
        assert len(its) == 2
        err = float(np.abs(fr[r] - its[1]).max())
        print('replicate %d: second iterate off by %.3g (bound %.3g), delta %.3g (restatement %.3g)' % (r, err, 2 * s['tol'], delta[r], deltas[1]))
        assert err <= 2 * s['tol'] and abs(delta[r] - deltas[1]) <= 4 * s['tol']


def no_overlap_set():
    """states 0 and 1 overlap and are sampled; state 2 is unsampled and so far off that only sample 0, an outlier, weighs anything"""
    rng = np.random.default_rng(12)
    b, c = np.array([1.0, 1.1, -50.0]), np.array([0.5, 0.5, 0.5])
    count = np.array([150, 150, 0], dtype=np.int64)
    e, v = rng.gamma(4.0, 1.0, 300), 3.0 + rng.random(300)
    e[0] = 100.0
    assert e[1:].max() < 20
    f = R.solve(b, c, count, np.zeros(3), e, v)[0]
    mult = np.ones((2, 300), dtype=np.uint16)
    mult[1, 0], mult[1, 1] = 0, 2
    return b, c, count, e, v, f, mult


def test_a_replicate_that_lost_its_only_overlap():
    b, c, count, e, v, f, mult = no_overlap_set()
    fr, iters, delta, status = boot_solve(b, c, count, e, v, f, mult, tol=1e-12, max_iter=50)
    assert status[0] == 0 and np.isfinite(fr[0]).all()
    tol = 3 * R.tol_map(300, 3, R.u_max(b, c, e, v)) + 4 * R.UNIT * np.abs(f).max()
    print('no overlap: status %s, iters %s, fr[1] = %s' % (status, iters, fr[1]))
    if status[1] == 2:
        assert np.isnan(fr[1]).all()
    else:
        one = boot_solve(b, c, count, e, v, f, mult)[0]
        want = BR.apply_map(b, c, count, f, e, v, mult[1])[0]
        assert np.isfinite(fr[1]).all() and float(np.abs(one[1].astype(R.LD) - want).max()) <= tol + 4 * R.UNIT * float(np.abs(want).max())
    tb, tc = np.array([1.0, 1.05]), np.array([0.5, 0.5])
    ex = boot_expect(b, c, count, f, e, v, mult, fr, tb, tc, np.ones((1, 300)))
    for key, x in ex.items():
        assert np.isfinite(x[0]).all(), key
        if status[1] == 2:
            assert np.isnan(x[1]).all(), key


# ---- expectations, with the restatement's fr passed in
def targets(b, c, nt, rng):
    tb = np.concatenate([b, rng.uniform(b.min() * 0.95, b.max() * 1.05, nt)])[:nt]
    tc = np.concatenate([c, rng.uniform(c.min() * 0.95, c.max() * 1.05, nt)])[:nt]
    return np.ascontiguousarray(tb), np.ascontiguousarray(tc)


def observables(nobs, e, rng):
    obs = rng.normal(0.0, 2.0, (nobs, e.size))
    if nobs > 0:
        obs[0] = 3.25
    if nobs > 1:
        obs[1] = e - e.mean()
    return obs


_EXPECT = {}


def expect_set(n=1009 + 37, nrep=RT + 1):
    if n not in _EXPECT:
        b, c, count, e, v, f0 = data(5, n, seed=3)
        f = base_solution('expect-%d' % n, b, c, count, e, v, f0)
        mult = resample(e.size, nrep, 5)
        fr = np.stack([BR.apply_map(b, c, count, f, e, v, m)[0].astype(np.float64) for m in mult])
        _EXPECT[n] = dict(b=b, c=c, count=count, e=e, v=v, f=f, mult=mult, fr=fr)
    return _EXPECT[n]


def check_expectations(got, want, tol, e, v, obs, n):
    de, dv = float(np.abs(e - e.mean()).max()), float(np.abs(v - v.mean()).max())
    err = lambda key: np.abs(got[key].astype(R.LD) - want[key]).astype(np.float64)
    print('tolerance %.3g: tf %.3g, mean %.3g %.3g, cov %.3g %.3g %.3g, ess (relative) %.3g' % (
        tol, err('tf').max(), err('mean')[:, 0].max() / de, err('mean')[:, 1].max() / dv, err('cov')[:, 0].max() / de ** 2,
        err('cov')[:, 1].max() / (de * dv), err('cov')[:, 2].max() / dv ** 2, (err('ess') / want['ess'].astype(np.float64)).max()))
    assert err('tf').max() <= tol
    assert err('mean')[:, 0].max() <= tol * de and err('mean')[:, 1].max() <= tol * dv
    assert err('cov')[:, 0].max() <= tol * de * de and err('cov')[:, 1].max() <= tol * de * dv and err('cov')[:, 2].max() <= tol * dv * dv
    assert (err('ess') <= 4 * tol * want['ess'].astype(np.float64)).all()
    assert (got['ess'] >= 1).all() and (got['ess'] <= n).all()
    if obs is not None:
        assert (err('omean') <= 2 * tol * np.abs(obs).max(axis=1)[None, :]).all()
        assert np.abs(got['omean'][:, 0] - 3.25).max() <= 2 * tol * 3.25


@pytest.mark.parametrize('nt,nobs,nrep', ((1, 0, 1), (1, 8, RT + 1), (TGB - 1, 1, 1), (TGB, 8, 1), (TGB + 1, 1, 2), (TGB + 1, 0, RT + 1)))
def test_expectations(nt, nobs, nrep):
    s = expect_set()
    b, c, count, e, v, f = (s[key] for key in ('b', 'c', 'count', 'e', 'v', 'f'))
    rng = np.random.default_rng(nt * 10 + nobs)
    tb, tc = targets(b, c, nt, rng)
    obs = observables(nobs, e, rng) if nobs else None
    pick = list(range(RT + 1 - nrep, RT + 1))                              # the last replicates: the one behind the tile is always among them
    got = boot_expect(b, c, count, f, e, v, s['mult'][pick], s['fr'][pick], tb, tc, obs)
    tol = 3 * R.tol_map(e.size, 5, max(R.u_max(b, c, e, v), R.u_max(tb, tc, e, v)))
    check = sorted(set([0, nrep - 1])) if nt > 8 else range(nrep)         # the restatement costs: both ends of the batch where there are many targets
    for j in check:
        want = BR.expect(b, c, count, s['fr'][pick[j]], e, v, s['mult'][pick[j]], tb, tc, obs)
        check_expectations({key: x[j] for key, x in got.items()}, want, tol, e, v, obs, e.size)
    for x in got.values():
        assert np.isfinite(x).all()


@pytest.mark.parametrize('nt,nobs', ((5, 0), (3, 2)))
def test_expectations_over_more_than_one_chunk(nt, nobs):
    """N = one sample more than two of the expectation kernel's chunks; 5 and 3 targets are no multiple of its 4 and 2 per workgroup"""
    s = expect_set(2 * ECH + 1, 2)
    b, c, count, e, v, f = (s[key] for key in ('b', 'c', 'count', 'e', 'v', 'f'))
    rng = np.random.default_rng(nt * 10 + nobs)
    tb, tc = targets(b, c, nt, rng)
    obs = observables(nobs, e, rng) if nobs else None
    got = boot_expect(b, c, count, f, e, v, s['mult'], s['fr'], tb, tc, obs)
    tol = 3 * R.tol_map(e.size, 5, max(R.u_max(b, c, e, v), R.u_max(tb, tc, e, v)))
    for j in range(2):
        want = BR.expect(b, c, count, s['fr'][j], e, v, s['mult'][j], tb, tc, obs)
        check_expectations({key: x[j] for key, x in got.items()}, want, tol, e, v, obs, e.size)


def test_two_calls_give_identical_bits():
    b, c, count, e, v, f0 = data(9, 3 * CH + 11, seed=7)
    f = base_solution('bits', b, c, count, e, v, f0)
    mult = resample(e.size, RT + 3, 8)
    one = boot_solve(b, c, count, e, v, f, mult, tol=1e-10, max_iter=7)
    two = boot_solve(b, c, count, e, v, f, mult, tol=1e-10, max_iter=7)
    for x, y in zip(one, two):
        assert x.tobytes() == y.tobytes()
    assert (one[3] != 2).all()
    rng = np.random.default_rng(8)
    tb, tc = targets(b, c, 12, rng)
    obs = observables(3, e, rng)
    x, y = boot_expect(b, c, count, f, e, v, mult, one[0], tb, tc, obs), boot_expect(b, c, count, f, e, v, mult, one[0], tb, tc, obs)
    for key in x:
        assert x[key].tobytes() == y[key].tobytes(), key


# ---- the command line
def write_grid(tmp_path, pn=2, tn=3, sn=64, natoms=32):
    prefix = str(tmp_path / 'rw.lj.fcc.lammps')
    rng = np.random.default_rng(10)
    P, T = np.linspace(1, 2, pn, dtype=np.float32), np.linspace(1, 2, tn, dtype=np.float32)
    noise = rng.normal(size=(pn, tn, sn))
    for i in range(1, sn):                                               # a correlated series: g > 1
        noise[..., i] = 0.7 * noise[..., i - 1] + np.sqrt(1 - 0.49) * noise[..., i]
    pe = -5.0 * natoms + 1.5 * natoms * T[None, :, None] + np.sqrt(1.5 * natoms) * T[None, :, None] * noise
    vol = natoms * (1.0 + 0.1 * T[None, :, None] - 0.02 * P[:, None, None]) + rng.normal(size=(pn, tn, sn))
    np.save(prefix + '.virial.trgt.npy', P)
    np.save(prefix + '.temp.trgt.npy', T)
    np.save(prefix + '.pe.npy', pe.astype(np.float32))
    np.save(prefix + '.vol.npy', vol.astype(np.float32))
    np.save(prefix + '.natoms.npy', np.full((pn, tn, sn), natoms, dtype=np.uint16))
    np.save(prefix + '.sof.npy', rng.random((pn, tn, sn)).astype(np.float32))
    return prefix


PLAIN = ('rwf', 'rwi', 'rwt', 'rwg', 'rwh', 'rwv', 'rwc', 'rwn', 'rwo', 'rwm')
BOOT = ('rwb', 'rwbi', 'rwfs', 'rwgs', 'rwhs', 'rwvs', 'rwcs', 'rwos', 'rwms', 'rwes')


def run_stage(prefix, extra):
    for key in PLAIN + BOOT + ('rwx', 'rwp', 'rwa', 'rwe'):
        if os.path.exists(prefix + '.%s.npy' % key):
            os.remove(prefix + '.%s.npy' % key)
    rc = reweight.main(['-n', 'rw', '-e', 'LJ', '-tg', '17', '-rt', '1e-12', '-ob', 'sof', '-hq', 'pe', '-hb', '16', '-hx', '-2.75'] + extra)
    return rc, {key: np.load(prefix + '.%s.npy' % key) for key in PLAIN + BOOT + ('rwe',) if os.path.exists(prefix + '.%s.npy' % key)}


def test_command_line(tmp_path, monkeypatch):
    prefix = write_grid(tmp_path)
    monkeypatch.chdir(tmp_path)
    rc, plain = run_stage(prefix, [])
    assert rc == 0 and sorted(plain) == sorted(PLAIN + ('rwe',))          # without -bs: the files of before, and only those
    rc, again = run_stage(prefix, [])
    assert all(plain[key].tobytes() == again[key].tobytes() for key in plain)
    # blocks as long as the series: every replicate is the original, every spread is rounding
    rc, whole = run_stage(prefix, ['-bs', '8', '-bl', '64'])
    assert rc == 0 and all(plain[key].tobytes() == whole[key].tobytes() for key in plain)
    b, c = reweight.states(np.load(prefix + '.virial.trgt.npy'), np.load(prefix + '.temp.trgt.npy'), 'LJ')
    pe, vol = np.load(prefix + '.pe.npy').astype(np.float64).reshape(6, -1), np.load(prefix + '.vol.npy').astype(np.float64).reshape(6, -1)
    bound = 2 * 1e-12 + 2 * 3 * R.tol_map(6 * 64, 6, R.u_max(b, c, pe.reshape(-1), vol.reshape(-1)))
    assert (whole['rwbi'][:, 2] == 0).all() and (whole['rwb'][..., 1] == 64).all() and (whole['rwb'][..., 0] >= 1).all()
    print('-bl 64: the largest standard deviation of f is %.3g (bound %.3g)' % (whole['rwfs'].max(), bound))
    assert whole['rwfs'].max() <= bound
    for key in ('rwgs', 'rwhs', 'rwvs', 'rwcs', 'rwos'):
        assert whole[key].max() <= bound, key                             # the same replicate eight times: the rounding of a mean
    assert (whole['rwms'][:, 0] <= bound).all() and (whole['rwms'][:, 3] == 8).all()
    assert (whole['rwes'][:, 3] == (~np.isnan(plain['rwe'])) * 8).all() and not (whole['rwes'][:, 0] > bound).any()
    # the real thing
    rc, boot = run_stage(prefix, ['-bs', '8'])
    assert rc == 0 and all(plain[key].tobytes() == boot[key].tobytes() for key in plain)
    shapes = dict(rwb=(2, 3, 2), rwbi=(8, 3), rwfs=(2, 3), rwgs=(2, 17), rwhs=(2, 17), rwvs=(2, 17), rwcs=(2, 17), rwos=(2, 17, 1),
                  rwms=(2, 4), rwes=(2, 4))
    for key, shape in shapes.items():
        assert boot[key].shape == shape and boot[key].dtype == np.float64, key
    for key in ('rwb', 'rwbi', 'rwfs', 'rwgs', 'rwhs', 'rwvs', 'rwcs', 'rwos', 'rwms'):
        assert np.isfinite(boot[key]).all(), key
    assert (boot['rwb'][..., 0] > 1.5).all() and (boot['rwb'][..., 1] == np.ceil(boot['rwb'][..., 0])).all()
    assert (boot['rwbi'][:, 2] == 0).all() and (boot['rwbi'][:, 1] <= 1e-12).all() and (boot['rwbi'][:, 0] >= 1).all()
    assert boot['rwfs'][0, 0] == 0 and (boot['rwfs'].reshape(-1)[1:] > 1e-4).all() and (boot['rwhs'] > 0).all()
    assert (boot['rwms'][:, 3] == 8).all() and (boot['rwms'][:, 1] <= boot['rwms'][:, 2]).all()
    assert (boot['rwes'][:, 3] <= 8).all() and (boot['rwes'][:, 3] >= 0).all()
    for p in range(2):
        if not np.isnan(plain['rwe'][p]):
            assert boot['rwes'][p, 3] >= 1 and boot['rwes'][p, 1] <= boot['rwes'][p, 2]
    # the seed
    rc, same = run_stage(prefix, ['-bs', '8', '-bd', '256'])
    assert all(boot[key].tobytes() == same[key].tobytes() for key in boot)
    rc, other = run_stage(prefix, ['-bs', '8', '-bd', '7'])
    assert other['rwfs'].tobytes() != boot['rwfs'].tobytes() and other['rwb'].tobytes() == boot['rwb'].tobytes()


def test_replicates_that_do_not_converge_set_the_exit_status(tmp_path):
    """two applications are not enough for 1e-9, neither for the base solve nor for a resampled replicate: the files are still
    written, both messages go to stderr, exit status 1; without -ob and -hx there is no .rwos and no .rwes"""
    prefix = write_grid(tmp_path)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'neuralmelting_amd.reweight', '-n', 'rw', '-tg', '5', '-bs', '3', '-ri', '2'],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and 'bootstrap replicates did not converge' in r.stderr, r.stderr
    info = np.load(prefix + '.rwbi.npy')
    assert info.shape == (3, 3) and (info[:, 0] == 2).all() and (info[:, 2] == 1).all() and (info[:, 1] > 1e-9).all()
    assert np.load(prefix + '.rwgs.npy').shape == (2, 5) and np.load(prefix + '.rwms.npy').shape == (2, 4)
    assert not os.path.exists(prefix + '.rwes.npy') and not os.path.exists(prefix + '.rwos.npy')
