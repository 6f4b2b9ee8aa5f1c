"""Multistate reweighting on the GPU: nm_reweight_solve and nm_reweight_expect through the C-ABI against the longdouble
restatement tests/reweight_ref.py and the Gamma known answer, never against the library itself.

Tolerances.  tol_map(N, K, U) = (N + K + 64) u + 16 u U is the issue's bound for one application of the map (logd: N = 0).
Where a quantity is a ratio of two weighted sums, the bound is multiplied by the largest summand (the means: max |x - mean x|;
the second moments: the product of two such; an observable: twice that, max |obs|, as csrc/nm_reweight.h derives for a ratio).
ess = (sum w)^2 / sum w^2 carries two relative errors of the first sum and one of the second, whose exponent's rounding counts
twice: 4 tol_map relative.  Where e and v carry an offset of 1e6 the doubles that hold f, tf and logd are ~1e6 themselves: those
comparisons add a few roundings of the value compared (4 u |value|), nothing else changes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import reweight_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import reweight

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -7.25e300
KT, CH, TGB = 512, 4096, 256      # csrc/nm_reweight.h: the LDS state tile, the sample chunk, the targets per launch


def dp(a):
    return a.ctypes.data_as(B.c_double_p)


def solve(b, c, count, e, v, f0, tol=0.0, max_iter=1, logd=True):
    """the raw ABI on sentinel-filled outputs: (f, logd or None, iters, delta)"""
    L = B.load()
    f = np.array(f0, dtype=np.float64)
    ld = np.full(e.size, SENT) if logd else None
    iters, delta = C.c_int(-1), C.c_double(SENT)
    count = np.ascontiguousarray(count, dtype=np.int64)
    rc = L.nm_reweight_solve(0, b.size, dp(b), dp(c), count.ctypes.data_as(B.c_int64_p), e.size, dp(e), dp(v), tol, max_iter, dp(f),
                             dp(ld) if logd else None, C.byref(iters), C.byref(delta))
    assert rc == B.NM_OK, L.nm_reweight_last_error().decode()
    return f, ld, iters.value, delta.value


def expect(b, c, count, f, e, v, tb, tc, obs=None):
    L = B.load()
    nt, nobs = tb.size, 0 if obs is None else obs.shape[0]
    out = dict(tf=np.full(nt, SENT), ess=np.full(nt, SENT), mean=np.full((nt, 2), SENT), cov=np.full((nt, 3), SENT),
               omean=np.full((nt, nobs), SENT))
    count = np.ascontiguousarray(count, dtype=np.int64)
    rc = L.nm_reweight_expect(0, b.size, dp(b), dp(c), count.ctypes.data_as(B.c_int64_p), dp(f), e.size, dp(e), dp(v), nt, dp(tb), dp(tc),
                              nobs, dp(obs) if nobs else None, dp(out['tf']), dp(out['ess']), dp(out['mean']), dp(out['cov']),
                              dp(out['omean']) if nobs else None)
    assert rc == B.NM_OK, L.nm_reweight_last_error().decode()
    for key, x in out.items():
        assert not (x == SENT).any() and np.isfinite(x).all(), key
    return out


def data(k, n, seed=0, empty=(), same=()):
    """k states, n samples; the states `empty` drew no sample; the pair `same` is one state twice (with its own count and start:
    F(f)[i] depends on b[i] and c[i] only)"""
    rng = np.random.default_rng(1000 * k + n + seed)
    b = np.sort(1.0 + 0.5 * rng.random(k))
    c = 0.5 + 0.3 * rng.random(k)
    if same:
        b[same[1]], c[same[1]] = b[same[0]], c[same[0]]
    e, v = rng.gamma(4.0, 1.0, n), rng.gamma(3.0, 1.0, n)
    pick = np.array([s for s in range(k) if s not in empty])
    count = np.bincount(pick[rng.integers(0, pick.size, n)], minlength=k).astype(np.int64)
    f0 = rng.normal(0.0, 0.5, k)
    return b, c, count, e, v, f0


# ---- one application of the map
MAP_CASES = {
    'K1': dict(k=1, n=1009), 'K2': dict(k=2, n=1009), 'K63': dict(k=63, n=1009), 'K64': dict(k=64, n=1009), 'K65': dict(k=65, n=1009),
    'K513-above-the-tile': dict(k=KT + 1, n=1009), 'N1': dict(k=5, n=1), 'N63': dict(k=5, n=63), 'N64': dict(k=5, n=64),
    'N65': dict(k=5, n=65), 'N4095': dict(k=5, n=CH - 1), 'N4096': dict(k=5, n=CH), 'N4097': dict(k=5, n=CH + 1),
    'N100003': dict(k=5, n=100003), 'N262145-above-the-lanes': dict(k=5, n=64 * CH + 1), 'a-state-without-samples': dict(k=6, n=1009, empty=(0, 3)),
    'two-identical-states': dict(k=7, n=1009, same=(1, 5)),
}


@pytest.mark.parametrize('case', sorted(MAP_CASES))
def test_one_application_of_the_map(case):
    kw = MAP_CASES[case]
    b, c, count, e, v, f0 = data(**kw)
    assert count.sum() == e.size and all(count[s] == 0 for s in kw.get('empty', ()))
    f, logd, iters, delta = solve(b, c, count, e, v, f0)
    want_f, want_logd = R.apply_map(b, c, count, f0, e, v)
    k, n = b.size, e.size
    u_max = R.u_max(b, c, e, v)
    tol_f, tol_d = R.tol_map(n, k, u_max), R.tol_map(0, k, u_max)
    err_f = float(np.abs(f.astype(R.LD) - want_f).max())
    err_d = float(np.abs(logd.astype(R.LD) - want_logd).max())
    print('%s: |df| = %.3g (tolerance %.3g), |dlogd| = %.3g (tolerance %.3g), U = %.3g' % (case, err_f, tol_f, err_d, tol_d, u_max))
    assert iters == 1 and f[0] == 0.0
    assert np.isfinite(f).all() and np.isfinite(logd).all()
    assert err_f <= tol_f and err_d <= tol_d
    assert abs(delta - np.abs(f - f0).max()) <= 2 * tol_f
    if k == 1:
        assert f.tolist() == [0.0]
    if 'same' in kw:
        assert f[kw['same'][0]] == f[kw['same'][1]]


# ---- the converged solution on the Gamma set
@pytest.fixture(scope='module')
def gamma():
    b, c, count, e, v = R.gamma_set()
    f, _, iters, delta = solve(b, c, count, e, v, R.gamma_start(b, c, count, e, v), tol=1e-10, max_iter=5000, logd=False)
    return dict(b=b, c=c, count=count, e=e, v=v, f=f, iters=iters, delta=delta)


def test_converged_solution_is_a_fixed_point_and_the_known_answer(gamma):
    g = gamma
    print('Gamma set: %d iterations, delta %.3g' % (g['iters'], g['delta']))
    assert g['delta'] <= 1e-10 and 1 <= g['iters'] < 5000 and g['f'][0] == 0.0
    again = R.apply_map(g['b'], g['c'], g['count'], g['f'], g['e'], g['v'])[0]
    tol = 1e-10 + R.tol_map(g['e'].size, 6, R.u_max(g['b'], g['c'], g['e'], g['v']))
    res = float(np.abs(again - g['f'].astype(R.LD)).max())
    print('residual of the restatement\'s map at the returned f: %.3g (tolerance %.3g)' % (res, tol))
    assert res <= tol
    assert float(np.abs(g['f'] - R.gamma_exact_f()).max()) <= 0.05


def test_converged_moments_meet_the_known_answer(gamma):
    g = gamma
    tb, tc = R.gamma_targets()
    ex = expect(g['b'], g['c'], g['count'], g['f'], g['e'], g['v'], tb, tc)
    mean, cov = R.gamma_exact_moments(tb, tc)
    assert float(np.abs(ex['mean'] / mean - 1).max()) <= 0.05
    assert float(np.abs(ex['cov'][:, [0, 2]] / cov[:, [0, 2]] - 1).max()) <= 0.05
    assert float(np.abs(ex['cov'][:, 1] / np.sqrt(cov[:, 0] * cov[:, 2])).max()) <= 0.05
    assert (ex['ess'] <= g['e'].size).all() and (ex['ess'][:6] >= g['count'] / 6.0).all()
    # at the fixed point F(f) = f: tf at the states is f, up to a few delta
    assert np.abs(ex['tf'][:6] - g['f']).max() <= 4e-10 + R.tol_map(g['e'].size, 6, R.u_max(tb, tc, g['e'], g['v']))


# ---- expectations
def targets(b, c, nt, rng):
    """on the states first, then between and a little beyond them"""
    tb = np.concatenate([b, rng.uniform(b.min() * 0.95, b.max() * 1.05, nt)])[:nt]
    tc = np.concatenate([c, rng.uniform(c.min() * 0.95, c.max() * 1.05, nt)])[:nt]
    return np.ascontiguousarray(tb), np.ascontiguousarray(tc)


def observables(nobs, e, rng):
    """[0] a constant, [1] negative somewhere, the rest noise"""
    obs = rng.normal(0.0, 2.0, (nobs, e.size))
    if nobs > 0:
        obs[0] = 3.25
    if nobs > 1:
        obs[1] = e - e.mean()
        assert (obs[1] < 0).any() and (obs[1] > 0).any()
    return obs


def check_expectations(got, want, n, k, b, c, tb, tc, e, v, obs, extra_tf=0.0):
    tol = R.tol_map(n, k, max(R.u_max(b, c, e, v), R.u_max(tb, tc, e, v)))
    de, dv = float(np.abs(e - e.mean()).max()), float(np.abs(v - v.mean()).max())
    err = lambda key: np.abs(got[key].astype(R.LD) - want[key]).astype(np.float64)
    print('tolerance %.3g: tf %.3g, mean %.3g %.3g, cov %.3g %.3g %.3g, ess (relative) %.3g' % (
        tol, err('tf').max(), err('mean')[:, 0].max() / de, err('mean')[:, 1].max() / dv, err('cov')[:, 0].max() / de ** 2,
        err('cov')[:, 1].max() / (de * dv), err('cov')[:, 2].max() / dv ** 2, (err('ess') / want['ess'].astype(np.float64)).max()))
    assert err('tf').max() <= tol + extra_tf
    assert err('mean')[:, 0].max() <= tol * de and err('mean')[:, 1].max() <= tol * dv
    assert err('cov')[:, 0].max() <= tol * de * de and err('cov')[:, 1].max() <= tol * de * dv and err('cov')[:, 2].max() <= tol * dv * dv
    assert (err('ess') <= 4 * tol * want['ess'].astype(np.float64)).all()
    if obs is not None:
        assert (err('omean') <= 2 * tol * np.abs(obs).max(axis=1)[None, :]).all()
        # "a constant observable returns the constant": the issue names no tolerance.  sum(w * 3.25) and sum(w) round their
        # terms and their additions apart, so the ratio is the constant to the ratio's bound above, not to the last bit
        assert np.abs(got['omean'][:, 0] - 3.25).max() <= 2 * tol * 3.25


# the last: 65 chunks, so a lane of the wave that joins a target's chunks takes a second one
@pytest.mark.parametrize('nt,nobs,n', [pytest.param(nt, nobs, CH + 37, id='%d-%d' % (nt, nobs))
                                       for nt, nobs in ((1, 0), (1, 8), (TGB - 1, 1), (TGB, 8), (TGB + 1, 1), (TGB + 1, 0))]
                         + [pytest.param(TGB + 1, 1, 64 * CH + 1, id='%d-1-N262145-above-the-lanes' % (TGB + 1))])
def test_expectations(nt, nobs, n):
    b, c, count, e, v, f = data(5, n, seed=3)
    rng = np.random.default_rng(nt * 10 + nobs)
    tb, tc = targets(b, c, nt, rng)
    obs = observables(nobs, e, rng) if nobs else None
    got = expect(b, c, count, f, e, v, tb, tc, obs)
    want = R.expect(b, c, count, f, e, v, tb, tc, obs)
    check_expectations(got, want, e.size, 5, b, c, tb, tc, e, v, obs)
    assert (got['ess'] >= 1).all() and (got['ess'] <= e.size).all()


def test_offsets_of_a_million_cost_the_central_moments_nothing():
    b, c, count, e, v, f = data(5, 2003, seed=4)
    se, sv = -1e6, 1e6
    rng = np.random.default_rng(5)
    tb, tc = targets(b, c, 9, rng)
    plain = expect(b, c, count, f, e, v, tb, tc)
    # the same states with every u_k shifted by b_k se + c_k sv: f moves with it (exactly, then rounded to the double that carries it)
    fs = np.array([float(R.Fraction(float(fk)) + R.Fraction(float(bk)) * R.Fraction(se) + R.Fraction(float(ck)) * R.Fraction(sv))
                   for fk, bk, ck in zip(f, b, c)])
    es, vs = e + se, v + sv
    got = expect(b, c, count, fs, es, vs, tb, tc)
    want = R.expect(b, c, count, fs, es, vs, tb, tc)
    big = 4 * R.UNIT * max(np.abs(fs).max(), np.abs(want['tf'].astype(np.float64)).max())
    # against the restatement of the shifted problem: U is that of the centred data, as without the offsets
    tol = R.tol_map(e.size, 5, max(R.u_max(b, c, es, vs), R.u_max(tb, tc, es, vs)))
    de, dv = float(np.abs(es - es.mean()).max()), float(np.abs(vs - vs.mean()).max())
    assert abs(de - np.abs(e - e.mean()).max()) < 1e-8         # U and the spreads are those of the unshifted data
    err = lambda key: np.abs(got[key].astype(R.LD) - want[key]).astype(np.float64)
    print('shifted: tolerance %.3g, cov %.3g %.3g %.3g, ess (relative) %.3g, tf %.3g (+ %.3g)' % (
        tol, err('cov')[:, 0].max() / de ** 2, err('cov')[:, 1].max() / (de * dv), err('cov')[:, 2].max() / dv ** 2,
        (err('ess') / want['ess'].astype(np.float64)).max(), err('tf').max(), big))
    assert err('cov')[:, 0].max() <= tol * de * de and err('cov')[:, 1].max() <= tol * de * dv and err('cov')[:, 2].max() <= tol * dv * dv
    assert (err('ess') <= 4 * tol * want['ess'].astype(np.float64)).all()
    assert err('tf').max() <= tol + big
    # against the unshifted call: the means move by the shifts, tf by tb se + tc sv up to one constant (the doubles fs carry 4 u |fs|)
    assert np.abs(got['mean'][:, 0] - plain['mean'][:, 0] - se).max() <= 2 * tol * de + 4 * R.UNIT * abs(se)
    assert np.abs(got['mean'][:, 1] - plain['mean'][:, 1] - sv).max() <= 2 * tol * dv + 4 * R.UNIT * abs(sv)
    moved = got['tf'] - plain['tf'] - (tb * se + tc * sv)
    assert np.abs(moved - moved[0]).max() <= 2 * tol + 2 * big + 8 * R.UNIT * np.abs(tb * se + tc * sv).max()
    # and the iteration itself on the shifted samples
    f1, logd1, _, _ = solve(b, c, count, es, vs, fs)
    w1, wl = R.apply_map(b, c, count, fs, es, vs)
    assert np.abs(f1.astype(R.LD) - w1).max() <= tol + 4 * R.UNIT * np.abs(f1).max()
    assert np.abs(logd1.astype(R.LD) - wl).max() <= tol + 4 * R.UNIT * np.abs(logd1).max()


def test_states_without_any_overlap_give_finite_results():
    rng = np.random.default_rng(6)
    b, c = np.array([1.0, 1.5]), np.array([0.5, 0.5])
    count = np.array([300, 211], dtype=np.int64)
    e = np.concatenate([10.0 + rng.random(300), 5000.0 + rng.random(211)])
    v = 3.0 + rng.random(511)
    u = b[:, None] * e[None, :] + c[:, None] * v[None, :]
    assert np.abs(u[:, :300].max(axis=1) - u[:, 300:].min(axis=1)).min() > 2000
    f, logd, iters, delta = solve(b, c, count, e, v, np.zeros(2), tol=0.0, max_iter=3)
    assert iters == 3 and np.isfinite(f).all() and np.isfinite(logd).all() and np.isfinite(delta)
    tb, tc = np.array([1.0, 1.5, 1.25]), np.array([0.5, 0.5, 0.5])
    ex = expect(b, c, count, f, e, v, tb, tc)
    assert (ex['ess'] >= 1).all() and (ex['ess'] <= 511).all()
    want_f, want_logd = R.apply_map(b, c, count, np.zeros(2), e, v)
    f1, logd1, _, _ = solve(b, c, count, e, v, np.zeros(2))
    tol = R.tol_map(511, 2, R.u_max(b, c, e, v))
    assert np.abs(f1.astype(R.LD) - want_f).max() <= tol + 4 * R.UNIT * np.abs(f1).max()
    assert np.abs(logd1.astype(R.LD) - want_logd).max() <= tol + 4 * R.UNIT * np.abs(logd1).max()


# ---- housekeeping
def test_two_calls_give_identical_bits_and_logd_may_be_null():
    b, c, count, e, v, f0 = data(9, 3 * CH + 11, seed=7)
    one = solve(b, c, count, e, v, f0, tol=0.0, max_iter=7)
    two = solve(b, c, count, e, v, f0, tol=0.0, max_iter=7)
    assert one[2] == two[2] == 7 and one[3] == two[3]
    assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes()
    assert not (one[1] == SENT).any()
    null = solve(b, c, count, e, v, f0, tol=0.0, max_iter=7, logd=False)
    assert null[1] is None and null[0].tobytes() == one[0].tobytes()
    rng = np.random.default_rng(8)
    tb, tc = targets(b, c, 12, rng)
    obs = observables(3, e, rng)
    x, y = expect(b, c, count, one[0], e, v, tb, tc, obs), expect(b, c, count, one[0], e, v, tb, tc, obs)
    for key in x:
        assert x[key].tobytes() == y[key].tobytes(), key


def test_the_iteration_stops_at_the_first_iterate_within_the_tolerance():
    """the status is read every few iterations only: the result must still be the iterate that met the tolerance, not a later one"""
    b, c, count, e, v, f0 = data(4, 2 * CH + 5, seed=9)
    f, _, iters, delta = solve(b, c, count, e, v, f0, tol=1e-6, max_iter=500, logd=False)
    assert 1 < iters < 500 and delta <= 1e-6
    g, _, iters2, delta2 = solve(b, c, count, e, v, f0, tol=0.0, max_iter=iters, logd=False)
    assert iters2 == iters and delta2 == delta and g.tobytes() == f.tobytes()
    if iters > 2:
        _, _, _, before = solve(b, c, count, e, v, f0, tol=0.0, max_iter=iters - 1, logd=False)
        assert before > 1e-6


# ---- the command line
def write_grid(tmp_path, pn=2, tn=4, sn=200, natoms=32):
    prefix = str(tmp_path / 'rw.lj.fcc.lammps')
    rng = np.random.default_rng(10)
    P, T = np.linspace(1, 2, pn, dtype=np.float32), np.linspace(1, 2, tn, dtype=np.float32)
    pe = -5.0 * natoms + 1.5 * natoms * T[None, :, None] + np.sqrt(1.5 * natoms) * T[None, :, None] * rng.normal(size=(pn, tn, sn))
    vol = natoms * (1.0 + 0.1 * T[None, :, None] - 0.02 * P[:, None, None]) + rng.normal(size=(pn, tn, sn))
    np.save(prefix + '.virial.trgt.npy', P)
    np.save(prefix + '.temp.trgt.npy', T)
    np.save(prefix + '.pe.npy', pe.astype(np.float32))
    np.save(prefix + '.vol.npy', vol.astype(np.float32))
    np.save(prefix + '.natoms.npy', np.full((pn, tn, sn), natoms, dtype=np.uint16))
    np.save(prefix + '.sof.npy', rng.random((pn, tn, sn)).astype(np.float32))
    return prefix


def test_command_line(tmp_path, monkeypatch):
    prefix = write_grid(tmp_path)
    monkeypatch.chdir(tmp_path)
    assert reweight.main(['-n', 'rw', '-e', 'LJ', '-sk', '10', '-sd', '2', '-tg', '33', '-ob', 'sof']) == 0
    shapes = dict(rwf=(2, 4), rwi=(3,), rwt=(33,), rwg=(2, 33), rwh=(2, 33), rwv=(2, 33), rwc=(2, 33), rwn=(2, 33), rwo=(2, 33, 1), rwm=(2,))
    out = {}
    for key, shape in shapes.items():
        out[key] = np.load(prefix + '.%s.npy' % key)
        assert out[key].shape == shape and out[key].dtype == np.float64 and np.isfinite(out[key]).all(), key
    assert out['rwf'][0, 0] == 0.0
    assert out['rwi'][1] <= out['rwi'][2] == 1e-9 and 1 <= out['rwi'][0] < 20000
    assert all(t in out['rwt'] for t in out['rwm'])
    assert (out['rwn'] >= 1).all() and (out['rwn'] <= 2 * 4 * 95).all() and (out['rwc'] > 0).all()
    assert (out['rwo'] > 0).all() and (out['rwo'] < 1).all()
    assert (out['rwv'] > 1.0).all() and (out['rwv'] < 1.3).all()          # the grid's volumes per atom lie within 1.06 .. 1.18
    # one iteration cannot converge: the files are still written, a message names delta, exit status 1
    for key in shapes:
        os.remove(prefix + '.%s.npy' % key)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    r = subprocess.run([sys.executable, '-m', 'neuralmelting_amd.reweight', '-n', 'rw', '-ri', '1', '-tg', '5'], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and 'delta' in r.stderr, r.stderr
    assert np.load(prefix + '.rwi.npy')[0] == 1 and not os.path.exists(prefix + '.rwo.npy')
    assert np.load(prefix + '.rwg.npy').shape == (2, 5)
