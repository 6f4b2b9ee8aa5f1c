"""Reweighted histograms on the GPU: nm_reweight_histogram through the C-ABI against the longdouble restatement
tests/reweight_hist_ref.py, on sentinel-filled outputs.

Tolerance per bin (and for below and above): 2 tol_map(N, K, U) want + N 2^-96.  logd and tf each lie within tol_map = (N + K + 64) u
+ 16 u U of reweight_ref, and an error of the exponent's argument is the weight's relative error; N 2^-96 is the accumulator's
truncation.  U is the larger of max |b (e - e0) + c (v - v0)| over the states and over the targets, as test_reweight_gpu.py takes
it.  A sample counted in the wrong bin moves two bins by a weight of the order 1/N, which is 1e10 tolerances or more here.
The sample counts are the wave, chunk (4096) and workgroup (4 chunks) edges of csrc/nm_reweight.h, the target counts the edges
of a launch of 256 targets."""
import os

import numpy as np
import pytest

import reweight_hist_ref as H
import reweight_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import reweight

pytestmark = pytest.mark.gpu
SENT = -7.25e300
CH, HG, TGB = 4096, 4, 256        # csrc/nm_reweight.h: the sample chunk, the chunks of a workgroup, the targets per launch


def dp(a):
    return a.ctypes.data_as(B.c_double_p)


def histogram(b, c, count, f, e, v, tb, tc, x, edges, with_outside=True):
    """the raw ABI on sentinel-filled outputs: (hist (T, nq, nbins), outside (T, nq, 2) or None)"""
    L = B.load()
    x, edges = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(edges, dtype=np.float64)
    nt, nq, nbins = tb.size, x.shape[0], edges.shape[1] - 1
    assert x.shape == (nq, e.size) and edges.shape == (nq, nbins + 1)
    hist = np.full((nt, nq, nbins), SENT)
    outside = np.full((nt, nq, 2), SENT) if with_outside else None
    count = np.ascontiguousarray(count, dtype=np.int64)
    rc = L.nm_reweight_histogram(0, b.size, dp(b), dp(c), count.ctypes.data_as(B.c_int64_p), dp(f), e.size, dp(e), dp(v), nt, dp(tb), dp(tc),
                                 nq, dp(x), nbins, dp(edges), dp(hist), dp(outside) if with_outside else None)
    assert rc == B.NM_OK, L.nm_reweight_last_error().decode()
    for out in (hist, outside) if with_outside else (hist,):
        assert not (out == SENT).any() and np.isfinite(out).all() and (out >= 0).all()
    return hist, outside


def data(k, n, seed=0):
    """k states, n samples, and an f of the size a solution has"""
    rng = np.random.default_rng(1000 * k + n + seed)
    b = np.sort(1.0 + 0.5 * rng.random(k))
    c = 0.5 + 0.3 * rng.random(k)
    e, v = rng.gamma(4.0, 1.0, n), rng.gamma(3.0, 1.0, n)
    count = np.bincount(rng.integers(0, k, n), minlength=k).astype(np.int64)
    return b, c, count, e, v, rng.normal(0.0, 0.5, k)


def targets(b, c, nt, rng):
    """on the states first, then between and a little beyond them"""
    tb = np.concatenate([b, rng.uniform(b.min() * 0.95, b.max() * 1.05, nt)])[:nt]
    tc = np.concatenate([c, rng.uniform(c.min() * 0.95, c.max() * 1.05, nt)])[:nt]
    return np.ascontiguousarray(tb), np.ascontiguousarray(tc)


def span_edges(x, nbins, kind='span'):
    """'span': linspace(min, max) as the command line makes it (the largest sample lies ON the last edge); 'uneven': sorted random
    edges over the range; 'middle': the middle third of the range only.  A single value gets min - 0.5 .. min + 0.5."""
    lo, hi = float(x.min()), float(x.max())
    if lo == hi:
        lo, hi = lo - 0.5, lo + 0.5
    if kind == 'middle':
        lo, hi = lo + (hi - lo) / 3.0, hi - (hi - lo) / 3.0
    if kind == 'uneven':
        inner = np.sort(np.random.default_rng(nbins).uniform(lo, hi, nbins - 1))
        edges = np.concatenate([[lo], inner, [hi]])
        assert (np.diff(edges) > 0).all()
        return edges
    return np.linspace(lo, hi, nbins + 1)


def compare(label, b, c, count, f, e, v, tb, tc, x, edges):
    """one call against the restatement: every bin, below and above within the tolerance, and the sum rule; returns both"""
    n, k = e.size, b.size
    hist, outside = histogram(b, c, count, f, e, v, tb, tc, x, edges)
    want_h, want_o, _ = H.histogram(b, c, count, f, e, v, tb, tc, x, edges)
    u_max = max(R.u_max(b, c, e, v), R.u_max(tb, tc, e, v))
    err_h = np.abs(hist.astype(R.LD) - want_h).astype(np.float64)
    err_o = np.abs(outside.astype(R.LD) - want_o).astype(np.float64)
    tol_h, tol_o = H.tol(n, k, u_max, want_h), H.tol(n, k, u_max, want_o)
    total = hist.astype(R.LD).sum(axis=2) + outside.astype(R.LD).sum(axis=2)
    err_s = float(np.abs(total - 1).max())
    print('%s: largest deviation %.3g in a bin (%.3g of its tolerance), %.3g outside (%.3g of its tolerance); |sum - 1| %.3g (tolerance %.3g); '
          'U = %.3g' % (label, err_h.max(), (err_h / tol_h).max(), err_o.max(), (err_o / tol_o).max(), err_s, 2 * R.tol_map(n, k, u_max), u_max))
    assert (err_h <= tol_h).all() and (err_o <= tol_o).all()
    assert err_s <= 2 * R.tol_map(n, k, u_max)
    return hist, outside, want_h, want_o


@pytest.mark.parametrize('n', (1, 63, 64, 65, CH - 1, CH, CH + 1, HG * CH, HG * CH + 1, 100003))
def test_sample_counts(n):
    b, c, count, e, v, f = data(5, n, seed=1)
    rng = np.random.default_rng(n)
    tb, tc = targets(b, c, 3, rng)
    x = np.stack([e, rng.normal(0.0, 2.0, n)])
    edges = np.stack([span_edges(x[0], 64), span_edges(x[1], 64, 'middle')])
    _, _, want_h, want_o = compare('N = %d' % n, b, c, count, f, e, v, tb, tc, x, edges)
    assert (want_o[:, 0] == 0).all()                                   # the edges of the first quantity span its samples
    if n >= 63:
        assert (want_o[:, 1] > 0).all()                                # both sides of the second lie outside


@pytest.mark.parametrize('nt', (1, TGB - 1, TGB, TGB + 1))
def test_target_counts(nt):
    b, c, count, e, v, f = data(5, CH + 37, seed=2)
    tb, tc = targets(b, c, nt, np.random.default_rng(nt))
    compare('%d targets' % nt, b, c, count, f, e, v, tb, tc, e[None, :], span_edges(e, 16)[None, :])


@pytest.mark.parametrize('nq,nbins,kind', ((1, 1, 'span'), (1, 2, 'span'), (8, 1024, 'span'), (8, 1, 'span'), (3, 1023, 'span'),
                                           (2, 37, 'uneven'), (2, 37, 'middle'), (3, 213, 'uneven'), (4, 400, 'middle')))
def test_shapes_and_edges(nq, nbins, kind):
    """(8, 1024) is the limit of both (one target per workgroup, 131,328 B of LDS); (3, 213) takes two targets per workgroup,
    (4, 400) one, the small shapes four"""
    b, c, count, e, v, f = data(5, CH + 37, seed=3)
    rng = np.random.default_rng(nq * 10000 + nbins)
    tb, tc = targets(b, c, 5, rng)
    x = np.stack([e, v, e - v, rng.normal(size=e.size), rng.random(e.size), e * v, -e, rng.gamma(2.0, 1.0, e.size)][:nq])
    edges = np.stack([span_edges(xq, nbins, kind) for xq in x])
    _, _, _, want_o = compare('nq = %d, nbins = %d, %s edges' % (nq, nbins, kind), b, c, count, f, e, v, tb, tc, x, edges)
    if kind == 'middle':
        assert (want_o > 0).all()
    else:
        assert (want_o == 0).all()


def test_samples_on_the_edges():
    """every sample equals an edge, the first and the last included: a bin rule that multiplied instead of comparing would move
    whole samples"""
    b, c, count, e, v, f = data(5, CH + 37, seed=4)
    rng = np.random.default_rng(44)
    tb, tc = targets(b, c, 5, rng)
    edges = np.stack([np.linspace(0.1, 0.7, 65), span_edges(np.array([-3.0, 11.0]), 64, 'uneven')])
    x = np.stack([rng.choice(edges[0], e.size), rng.choice(edges[1], e.size)])
    x[:, :4] = edges[:, [0, 64, 0, 64]]
    assert np.isin(x[0], edges[0]).all() and np.isin(x[1], edges[1]).all()
    hist, outside, want_h, _ = compare('samples on the edges', b, c, count, f, e, v, tb, tc, x, edges)
    assert (outside == 0).all() and (want_h > 0).all()


def test_bins_equal_the_expectation_of_their_indicator():
    b, c, count, e, v, f = data(5, CH + 37, seed=5)
    tb, tc = targets(b, c, 7, np.random.default_rng(55))
    edges = span_edges(e, 8)
    hist, _ = histogram(b, c, count, f, e, v, tb, tc, e[None, :], edges[None, :])
    code = H.codes(e, edges)
    obs = np.stack([(code == j).astype(np.float64) for j in range(8)])
    assert obs.sum() == e.size
    ex = reweight.expect(b, c, count, f, e, v, tb, tc, obs)
    tol = R.tol_map(e.size, 5, max(R.u_max(b, c, e, v), R.u_max(tb, tc, e, v)))
    err = float(np.abs(hist[:, 0, :] - ex['omean']).max())
    print('bins against nm_reweight_expect of their indicators: %.3g (tolerance %.3g)' % (err, 4 * tol))
    assert err <= 4 * tol


def test_a_target_without_overlap_gives_finite_results():
    """two states far apart and a target far beyond them: one sample carries all the weight"""
    rng = np.random.default_rng(6)
    b, c = np.array([1.0, 1.5]), np.array([0.5, 0.5])
    count = np.array([300, 211], dtype=np.int64)
    e = np.concatenate([10.0 + rng.random(300), 5000.0 + rng.random(211)])
    e[17] = 0.0
    v = 3.0 + rng.random(511)
    f = np.zeros(2)
    tb, tc = np.array([200.0, 1.0, 1.5]), np.array([0.5, 0.5, 0.5])
    edges = span_edges(e, 32)
    hist, outside, _, _ = compare('no overlap', b, c, count, f, e, v, tb, tc, e[None, :], edges[None, :])
    tol = float(H.tol(511, 2, max(R.u_max(b, c, e, v), R.u_max(tb, tc, e, v)), 1.0))
    assert H.codes(e[17:18], edges)[0] == 0 and hist[0, 0, 0] >= 1.0 - tol and (outside == 0).all()


def test_two_calls_give_identical_bits_and_outside_may_be_null():
    b, c, count, e, v, f = data(9, 5 * CH + 11, seed=7)
    rng = np.random.default_rng(77)
    tb, tc = targets(b, c, 12, rng)
    x = np.stack([e, v, rng.normal(size=e.size)])
    edges = np.stack([span_edges(x[0], 100), span_edges(x[1], 100, 'middle'), span_edges(x[2], 100, 'uneven')])
    one = histogram(b, c, count, f, e, v, tb, tc, x, edges)
    two = histogram(b, c, count, f, e, v, tb, tc, x, edges)
    assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes()
    null = histogram(b, c, count, f, e, v, tb, tc, x, edges, with_outside=False)
    assert null[1] is None and null[0].tobytes() == one[0].tobytes()
    h, o = reweight.histogram(b, c, count, f, e, v, tb, tc, x, edges)  # the Python entry is the same call
    assert h.tobytes() == one[0].tobytes() and o.tobytes() == one[1].tobytes()


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


def test_command_line(tmp_path, monkeypatch, capsys):
    plain, with_hq = tmp_path / 'plain', tmp_path / 'hq'
    plain.mkdir()
    with_hq.mkdir()
    common = ['-n', 'rw', '-e', 'LJ', '-sk', '10', '-sd', '2', '-tg', '33', '-ob', 'sof']
    prefix0 = write_grid(plain)
    monkeypatch.chdir(plain)
    assert reweight.main(common) == 0
    assert not any(os.path.exists(prefix0 + '.%s.npy' % key) for key in reweight.HIST_SUFFIXES)
    prefix = write_grid(with_hq)
    monkeypatch.chdir(with_hq)
    assert reweight.main(common + ['-v', '-hq', 'sof', 'pe', 'vol', '-hb', '32', '-hx', '0.5']) == 0
    said = capsys.readouterr().out
    for key in reweight.SUFFIXES:                                       # the ten earlier files, byte for byte
        assert open(prefix0 + '.%s.npy' % key, 'rb').read() == open(prefix + '.%s.npy' % key, 'rb').read(), key
    out = {key: np.load(prefix + '.%s.npy' % key) for key in reweight.HIST_SUFFIXES}
    shapes = dict(rwx=(3, 33), rwp=(2, 33, 3, 32), rwa=(2, 33), rwe=(2,))
    for key, shape in shapes.items():
        assert out[key].shape == shape and out[key].dtype == np.float64, key
    assert np.isfinite(out['rwx']).all() and np.isfinite(out['rwp']).all() and (out['rwp'] >= 0).all()
    # the edges span the kept samples of every quantity (pe and vol per atom), so nothing lies outside and the bins sum to 1
    sof = np.load(prefix + '.sof.npy').astype(np.float64)[:, :, 10::2]
    pe = np.load(prefix + '.pe.npy').astype(np.float64)[:, :, 10::2]
    vol = np.load(prefix + '.vol.npy').astype(np.float64)[:, :, 10::2]
    for q, kept in enumerate((sof, pe / 32, vol / 32)):
        assert np.array_equal(out['rwx'][q], np.linspace(kept.min(), kept.max(), 33))
    P, T = np.load(prefix + '.virial.trgt.npy'), np.load(prefix + '.temp.trgt.npy')
    b, c = reweight.states(P, T, 'LJ')
    _, tb, tc = reweight.fine_targets(P, T, 'LJ', 33)
    tol = 2 * R.tol_map(pe.size, 8, max(R.u_max(b, c, pe, vol), R.u_max(tb.reshape(-1), tc.reshape(-1), pe, vol)))
    print('|sum of .rwp over the bins - 1| = %.3g (tolerance %.3g)' % (np.abs(out['rwp'].sum(axis=3) - 1).max(), tol))
    assert np.abs(out['rwp'].sum(axis=3) - 1).max() <= tol
    # the cut 0.5 on sof, moved to the nearest edge; the uniform sof does not depend on the state: no crossing is required of it
    j = int(np.argmin(np.abs(out['rwx'][0] - 0.5)))
    assert np.array_equal(out['rwa'], out['rwp'][:, :, 0, j:].sum(axis=2))
    want = reweight.equal_weight(np.load(prefix + '.rwt.npy'), out['rwa'])
    assert np.array_equal(out['rwe'], want, equal_nan=True)
    assert 'the cut is the edge %.9g' % out['rwx'][0, j] in said
