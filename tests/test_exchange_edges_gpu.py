"""The device's two exchange sweeps — nm_exchange_kernel (exchange_row: one wave, rows lane-strided) and the row leader's sweep inside
nm_cycles_kernel — against the plain restatement of tests/exchange_ref.py (own Philox, criterion in longdouble), where the existing tests
do not go: more rows than the wave has lanes, no pair or one pair per row, rows of up to 128 temperatures (the fused leader's scratch then
runs over the reduction area's first word, which the row barrier uses as its flag), a second and third sweep on top of a non-identity
slot-to-buffer map with an adapt in between, whole-row shards against the full grid, the exchange tape at more than one row, and the
numerical edges of u <= min(1, exp(dh)).  Every check is deterministic; the margins of the reference's decisions are asserted where the
reference is made (exchange_ref.check_margins), so a criterion that is off by rounding cannot flip one.

Measured on an MI355X: the largest |dh_dev - dh_ref| / bound is 1.5e-4 on the synthetic energies (2 x 33 and 2 x 64) and 0.072 on the chains'
own energies in the fused runs (1 x 128), where neighbouring slots differ by hundreds of energy units and the rounded reciprocals count.

What this file cannot tell apart: `<` from `<=` in the FUSED leader's decision.  The two differ only where a Philox uniform equals
min(1, exp(dh)) to the bit, and the fused launch takes no tape; exchange_row's `<=` is pinned through the tape (u = 0 against exp = 0)."""
import numpy as np
import pytest

import exchange_ref as R

pytestmark = pytest.mark.gpu

FACTOR = {0.25: 0.9375, 0.5: 1.0, 0.75: 1.0625}      # gen_mc_param (remcmc:726-745)


def _engine(npn, nt, **kw):
    """a context of 2-atom replicas: nothing here runs a block"""
    import neuralmelting_amd as nm
    P, T = R.grids(npn, nt)
    e = nm.Engine(2, P, T, seed=R.SEED, **kw)
    et, pf = e.constants()
    ref = R.constants_lj(P, T, kw.get('row0', 0), kw.get('nrows'))
    np.testing.assert_array_equal(et, ref[0])
    np.testing.assert_array_equal(pf, ref[1])
    return e


def _crit_ratio(crit, ref, what):
    """the device's float64 criteria within the restatement's bound of the longdouble ones, in its order; the largest error / bound"""
    assert len(crit) == len(ref.dh), what
    if not len(crit):
        return 0.0
    ratio = np.abs((crit.astype(np.longdouble) - ref.dh).astype(np.float64)) / ref.bound
    assert (ratio <= 1.0).all(), '%s: pair %d is off by %.3g of its bound' % (what, ratio.argmax(), ratio.max())
    return float(ratio.max())


@pytest.mark.parametrize('npn,nt', R.SHAPES)
def test_device_sweep_equals_the_restatement(npn, nt):
    """three sweeps at steps s, s + 1, s + 2 with fresh energies per slot each time: the second and third start from what the one before
    left in slot2buf; behind the first, an adapt whose step sizes must follow the buffers while ratios and counters stay with the slots"""
    ns, ppr = npn * nt, nt * (nt - 1) // 2
    rng = np.random.default_rng(1000 * npn + nt)
    e = _engine(npn, nt)
    d0 = (1.0 + np.arange(ns))[:, None] * np.array([1.0, 2.0, 3.0]) / 1024.0        # every buffer its own step sizes
    e.set_state(dxdvdt=d0)
    worst = 0.0
    for s, (step, th, ref) in enumerate(R.reference_sweeps(npn, nt)):
        what = '%dx%d sweep %d' % (npn, nt, s)
        e.set_thermo(th)                                                            # (by slot: lands in the buffer that sits there now)
        e.set_step(step)
        n = e.exchange(count=(s != 1))                                              # the middle sweep without the count's round trip
        perm = e.perm()
        assert n == (ref.swaps if s != 1 else None), what
        np.testing.assert_array_equal(perm, ref.perm, err_msg=what)
        worst = max(worst, _crit_ratio(e.exchange_crit(), ref, what))
        if s == 0:
            ratio = rng.choice(np.array([0.25, 0.5, 0.75], dtype=np.float32), size=(ns, 3))
            e.set_counters(count=1.0 + rng.random((ns, 6)), ratio=ratio)
            e.adapt()
            rows = e.thermo()
            f = np.vectorize(FACTOR.get)(ratio.astype(np.float64))
            np.testing.assert_array_equal(rows[:, 5:8], f * d0[ref.perm], err_msg='step sizes follow the buffer, the ratio the slot')
            assert (rows[:, 8:17] == 0).all()
            np.testing.assert_array_equal(rows[:, :5], th[ref.perm])                # (and the energies with the buffer)
    if ppr == 0:
        assert e.exchange() == 0 and list(e.perm()) == list(range(ns)) and e.exchange_crit().shape == (0,)
    else:
        assert not np.array_equal(e.perm(), np.arange(ns))
    assert (e.status() == 0).all()
    e.close()
    print('%dx%d: largest |dh_dev - dh_ref| / bound = %.3g' % (npn, nt, worst))


@pytest.mark.parametrize('npn,nt', [(3, 5), (65, 2)])
def test_exchange_tape_over_several_rows(npn, nt):
    """the tape is read at [local row * ppr + pair]; taking it away returns to Philox"""
    ns, npairs = npn * nt, npn * nt * (nt - 1) // 2
    et, pf = R.constants_lj(*R.grids(npn, nt))
    e = _engine(npn, nt)
    rng = np.random.default_rng(17 * npn + nt)
    tape = rng.random(npairs)
    th = R.case_thermo(npn, nt, 0)
    ref = R.sweep(npn, nt, 0, npn, R.SEED, 5, th[:, 1] + th[:, 2], th[:, 4], et, pf, tape=tape)
    R.check_margins(ref, 'tape %dx%d' % (npn, nt))
    philox = R.sweep(npn, nt, 0, npn, R.SEED, 5, th[:, 1] + th[:, 2], th[:, 4], et, pf)
    assert not np.array_equal(ref.perm, philox.perm)                                # the tape decides otherwise than Philox would
    e.set_thermo(th); e.set_step(5)
    e.set_exchange_tape(tape)
    assert e.exchange() == ref.swaps
    np.testing.assert_array_equal(e.perm(), ref.perm)
    _crit_ratio(e.exchange_crit(), ref, 'tape')
    e.set_exchange_tape(None)
    th = R.case_thermo(npn, nt, 1)
    ref2 = R.sweep(npn, nt, 0, npn, R.SEED, 6, th[:, 1] + th[:, 2], th[:, 4], et, pf, perm=ref.perm)
    R.check_margins(ref2, 'after the tape %dx%d' % (npn, nt))
    e.set_thermo(th); e.set_step(6)
    assert e.exchange() == ref2.swaps
    np.testing.assert_array_equal(e.perm(), ref2.perm)
    e.close()


def test_a_grid_without_pairs_takes_an_empty_tape():
    e = _engine(3, 1)
    e.set_exchange_tape(np.zeros(0))
    e.set_thermo(R.case_thermo(3, 1, 0))
    assert e.exchange() == 0 and list(e.perm()) == [0, 1, 2] and len(e.exchange_crit()) == 0
    e.set_exchange_tape(None)
    assert e.exchange() == 0
    assert (e.status() == 0).all()
    e.close()


def _edge_engine():
    import neuralmelting_amd as nm
    npn = len(R.EDGE_PAIRS)
    P, T = np.linspace(1.0, 8.0, npn, dtype=np.float32), np.array(R.EDGE_T, dtype=np.float32)
    return npn, nm.Engine(2, P, T, seed=R.SEED), R.constants_lj(P, T)


def test_edge_uniforms_against_exact_criteria_on_the_device():
    """exp(dh) exactly 1 against the largest uniform, 0 against u = 0 and u = 2^-53, inf against anything: through the tape; then the same
    energies on Philox, where dh >= 0 swaps and dh = -1000 does not"""
    npn, e, (et, pf) = _edge_engine()
    th = R.edge_pair_thermo()
    etot, vol = th[:, 1] + th[:, 2], th[:, 4]
    tape = np.array([u for _, _, u, _ in R.EDGE_PAIRS])
    want = [sw for _, _, _, sw in R.EDGE_PAIRS]
    ref = R.sweep(npn, 2, 0, npn, R.SEED, 0, etot, vol, et, pf, tape=tape)
    assert [ref.perm[2 * r] == 2 * r + 1 for r in range(npn)] == want               # (the reference itself: test_exchange_edges.py)
    e.set_thermo(th); e.set_step(0)
    e.set_exchange_tape(tape)
    assert e.exchange() == sum(want)
    perm = e.perm()
    for r, (name, _, _, sw) in enumerate(R.EDGE_PAIRS):
        assert (perm[2 * r] == 2 * r + 1) == sw and sorted(perm[2 * r:2 * r + 2]) == [2 * r, 2 * r + 1], name
    np.testing.assert_array_equal(e.exchange_crit(), R.EDGE_DH)                     # exact by construction
    e.set_exchange_tape(None)
    for step in (1, 2, 3):
        ref = R.sweep(npn, 2, 0, npn, R.SEED, step, etot, vol, et, pf, perm=perm)
        e.set_thermo(th); e.set_step(step)
        assert e.exchange() == ref.swaps == sum(dh >= 0 for dh in R.EDGE_DH)
        perm = e.perm()
        np.testing.assert_array_equal(perm, ref.perm)
    assert (e.status() == 0).all()
    e.close()


@pytest.mark.parametrize('kind', ['nan', 'inf'])
def test_nan_and_infinite_energies_on_the_device(kind):
    """a NaN energy never moves and leaves its row's other pairs as they are decided without it; +inf against -inf and +inf covers
    exp(-inf) = 0, exp(+inf) = inf and exp(NaN); the context stays usable"""
    nt = 5
    et, pf = R.constants_lj(*R.grids(1, nt))
    e = _engine(1, nt)
    th = R.edge_row_thermo(kind, nt)
    perm = np.arange(nt)
    for step in (0, 1, 2):
        ref = R.sweep(1, nt, 0, 1, R.SEED, step, th[:, 1] + th[:, 2], th[:, 4], et, pf, perm=perm)
        R.check_margins(ref, '%s row, step %d' % (kind, step))
        e.set_thermo(th); e.set_step(step)
        assert e.exchange() == ref.swaps
        perm = e.perm()
        np.testing.assert_array_equal(perm, ref.perm)
        crit, dh = e.exchange_crit(), ref.dh.astype(np.float64)
        np.testing.assert_array_equal(np.isnan(crit), np.isnan(dh))
        np.testing.assert_array_equal(crit[np.isinf(dh)], dh[np.isinf(dh)])
        fin = np.isfinite(dh)
        assert (np.abs(crit[fin] - dh[fin]) <= ref.bound[fin]).all()
        if kind == 'nan':
            assert perm[2] == 2 and np.isnan(crit).sum() == nt - 1 and ref.swaps > 0
        else:
            assert np.isnan(crit).any() and (crit == np.inf).any() and (crit == -np.inf).any()
    assert (e.status() == 0).all()
    th = R.edge_row_thermo('finite', nt)                                            # usable: an ordinary sweep behind them
    ref = R.sweep(1, nt, 0, 1, R.SEED, 3, th[:, 1] + th[:, 2], th[:, 4], et, pf, perm=perm)
    R.check_margins(ref, 'finite row behind the %s rows' % kind)
    e.set_thermo(th); e.set_step(3)
    assert e.exchange() == ref.swaps
    np.testing.assert_array_equal(e.perm(), ref.perm)
    _crit_ratio(e.exchange_crit(), ref, 'finite row')
    e.close()


def test_whole_row_shards_equal_the_full_grid():
    """contexts of rows 0-1 and 2-4 of a 5 x 6 grid, given their slices of the energies: the Philox counter takes the GLOBAL row, the
    criterion and tape index the local one — permutations (local buffer numbers), criteria bit for bit and counts are the full context's"""
    npn, nt = 5, 6
    ppr = nt * (nt - 1) // 2
    full = _engine(npn, nt)
    shards = [(r0, nr, _engine(npn, nt, row0=r0, nrows=nr)) for r0, nr in ((0, 2), (2, 3))]
    for s, (step, th, ref) in enumerate(R.reference_sweeps(npn, nt)):
        full.set_thermo(th); full.set_step(step)
        n = full.exchange()
        perm, crit = full.perm(), full.exchange_crit()
        assert n == ref.swaps
        np.testing.assert_array_equal(perm, ref.perm)
        total = 0
        for r0, nr, e in shards:
            e.set_thermo(R.case_thermo(npn, nt, s, r0, nr)); e.set_step(step)
            total += e.exchange()
            np.testing.assert_array_equal(e.perm(), perm[r0 * nt:(r0 + nr) * nt] - r0 * nt, err_msg='rows %d+%d sweep %d' % (r0, nr, s))
            np.testing.assert_array_equal(e.exchange_crit(), crit[r0 * ppr:(r0 + nr) * ppr])
        assert total == n
    assert not np.array_equal(shards[1][2].perm(), np.arange(3 * nt))
    for _, _, e in shards:
        e.close()
    full.close()


# ---- the row leader's sweep inside the fused launch, at wide and narrow rows ------------------------------------------------------------------

# element, pressure rows, temperatures, workgroups per replica the grid gets.  The leader's scratch — (4 nt + ppr) doubles and nt ints over the
# positions' LDS — ends at 18,432 B at nt = 64 and at 69,632 B at nt = 128 (68,580 B at 127): across the reduction area, whose first word the row
# barrier uses as its flag, inside the 82 KiB every 4^3 configuration asks for
FUSED = [('LJ', 1, 32, 8), ('LJ', 1, 33, 4), ('LJ', 1, 64, 4), ('LJ', 2, 64, 2), ('LJ', 1, 128, 2), ('LJ', 1, 127, 2), ('LJ', 64, 2, 2),
         ('LJ', 128, 1, 2), ('Al', 1, 64, 4)]
TIED_TO_THE_RESTATEMENT = {(2, 64), (1, 128)}


@pytest.mark.parametrize('el,npn,ntn,cus', FUSED)
def test_fused_cycles_at_wide_and_narrow_rows(monkeypatch, el, npn, ntn, cus):
    """test_cycles_gpu's criterion — everything bit for bit against the loop of run_block / adapt / exchange, one launch per call — on rows of 1, 2
    and 32 to 128 temperatures: 3 cycles of 2 moves from the lattice, then 2 more from where the chains stand"""
    from neuralmelting_amd import lattice
    from test_cycles_gpu import _engine as cyc_engine, _everything
    monkeypatch.setenv('NM_FUSED_CYCLES', 'all')
    pr, tr = ((1.0, 8.0), (0.25, 2.5)) if el == 'LJ' else ((1.0, 8.0), (256.0, 2560.0))
    P, T = R.grids(npn, ntn, pr, tr)
    x, v, box, d = lattice.init_states(4, P, T, 0.03125, 0.03125, el=el)
    mod, ns = 2, npn * ntn
    a = cyc_engine(4, P, T, el, x, v, box, d)
    assert a.cus_per_replica == cus
    got = []
    for step0, ncyc in ((7, 3), (10, 2)):
        a.timing_reset()
        a.set_step(step0)
        a.run_cycles(ncyc, mod)
        got.append(_everything(a))
        assert a.timing()[0] == 1                                                   # one launch
    assert a.note() == '' and a.heals == 0
    a.close()
    b = cyc_engine(4, P, T, el, x, v, box, d)
    want, before = [], None
    for step0, ncyc in ((7, 3), (10, 2)):
        for s in range(step0, step0 + ncyc):
            b.set_step(s)
            b.run_block(mod)
            b.adapt()
            if s == 11 and (npn, ntn) in TIED_TO_THE_RESTATEMENT:
                before = (b.thermo(), b.perm())                                     # what the last sweep decides on
            b.exchange(count=False)
        want.append(_everything(b))
    b.close()
    for g, w in zip(got, want):
        assert (g['status'] == 0).all()
        for key in w:
            np.testing.assert_array_equal(g[key], w[key], err_msg=key)
    if ntn > 1:
        assert not np.array_equal(want[1]['perm'], np.arange(ns))                   # the rows did exchange
    else:
        assert np.array_equal(got[1]['perm'], np.arange(ns)) and got[1]['crit'].shape == (0,)
    if before is not None:                                                          # the fused sweep tied to the independent reference
        rows, perm0 = before
        et, pf = R.constants_lj(P, T)
        ref = R.sweep(npn, ntn, 0, npn, 256, 11, rows[:, 1] + rows[:, 2], rows[:, 4], et, pf, perm=perm0)
        R.check_margins(ref, 'fused %dx%d, last sweep' % (npn, ntn))
        np.testing.assert_array_equal(got[1]['perm'], ref.perm)
        print('%dx%d fused: largest |dh_dev - dh_ref| / bound = %.3g' % (npn, ntn, _crit_ratio(got[1]['crit'], ref, 'fused')))
