"""The replica-exchange sweep at the grid's edges, on the CPU: the plain restatement (tests/exchange_ref.py: own Philox, criterion in
longdouble), the host sweep used when a pressure row spans ranks (neuralmelting_amd/exchange.py) and the oracle's decide identically — on
grids without pairs, with one pair per row, with more rows than a wave has lanes and with rows of up to 128 temperatures, over three
sweeps with the permutation carried over, from a row offset, and where exp overflows, underflows, gives exactly 1 or meets a NaN.
tests/test_exchange_edges_gpu.py holds the device kernels to the same restatement."""
import numpy as np
import pytest

import exchange_ref as R
from neuralmelting_amd import exchange as X


def test_restatement_philox_known_answers():
    # Random123 kat_vectors, philox4x32-10 (the three of test_oracle.py)
    assert R.philox4x32_10([0, 0, 0, 0], [0, 0]) == (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)
    assert R.philox4x32_10([0xffffffff] * 4, [0xffffffff] * 2) == (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)
    assert R.philox4x32_10([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == \
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)
    assert R.u01(0, 0) == 0.0 and R.u01(0xffffffff, 0xffffffff) == 1.0 - 2.0 ** -53 and R.u01(0x80000000, 0) == 0.5
    assert R.u01(0, 0x7ff) == 0.0 and R.u01(0, 0x800) == 2.0 ** -53            # the low 11 bits are dropped


def _same_nonfinite(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fin = np.isfinite(b)
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
    np.testing.assert_array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)])   # the same infinities
    return fin


def _within_bound(crit, res, what):
    """every float64 criterion within the restatement's bound of the longdouble one, pair by pair in sweep order; returns the worst ratio"""
    assert len(crit) == len(res.dh)
    if not len(crit):
        return 0.0
    err = np.abs((np.asarray(crit, dtype=np.longdouble) - res.dh).astype(np.float64))
    ratio = err / res.bound
    assert (ratio <= 1.0).all(), '%s: pair %d is off by %.3g of its bound' % (what, ratio.argmax(), ratio.max())
    return float(ratio.max())


@pytest.mark.parametrize('npn,nt', R.SHAPES)
def test_restatement_host_sweep_and_oracle_agree(oracle, npn, nt):
    """three sweeps with the permutation carried over and fresh energies per slot each time (the margins of every pair are checked when
    the reference is made: exchange_ref.reference_sweeps)"""
    et, pf = R.constants_lj(*R.grids(npn, nt))
    ns, ppr = npn * nt, nt * (nt - 1) // 2
    perm_o = perm_h = np.arange(ns)
    worst = 0.0
    for s, (step, th, ref) in enumerate(R.reference_sweeps(npn, nt)):
        etot, vol = th[:, 1] + th[:, 2], th[:, 4]
        swaps, perm_o, _, _, crit = oracle.exchange(npn, nt, 0, npn, R.SEED, step, etot, vol, et, pf, perm=perm_o)
        assert swaps == ref.swaps and list(perm_o) == list(ref.perm), 'oracle, sweep %d' % s
        worst = max(worst, _within_bound(crit, ref, 'oracle %dx%d sweep %d' % (npn, nt, s)))
        p, sw = X.sweep(npn, nt, R.SEED, step, etot, vol, et, pf)                   # (starts from the identity: composed here)
        perm_h = perm_h[p]
        assert sw == ref.swaps and list(perm_h) == list(ref.perm), 'exchange.sweep, sweep %d' % s
        assert len(ref.dh) == npn * ppr
        if ppr == 0:
            assert ref.swaps == 0 and list(ref.perm) == list(range(ns))
    if ppr:
        assert not np.array_equal(perm_o, np.arange(ns))                            # the comparison is not vacuous
    print('%dx%d: largest |dh_oracle - dh_ref| / bound = %.3g' % (npn, nt, worst))


@pytest.mark.parametrize('npn,nt,row0,nrows', [(5, 6, 2, 3), (5, 6, 0, 2), (130, 2, 64, 66), (3, 5, 2, 1), (130, 1, 100, 30)])
def test_oracle_from_a_row_offset(oracle, npn, nt, row0, nrows):
    """rows row0 .. of the grid swept on their own: the Philox counter takes the global row, everything else the local one — and the result is
    the full grid's, restricted to those rows"""
    et, pf = R.constants_lj(*R.grids(npn, nt), row0, nrows)
    perm = None
    full = R.reference_sweeps(npn, nt)
    ppr = nt * (nt - 1) // 2
    for s, (step, th, ref) in enumerate(R.reference_sweeps(npn, nt, row0, nrows)):
        swaps, perm, _, _, crit = oracle.exchange(npn, nt, row0, nrows, R.SEED, step, th[:, 1] + th[:, 2], th[:, 4], et, pf, perm=perm)
        assert swaps == ref.swaps and list(perm) == list(ref.perm)
        _within_bound(crit, ref, 'oracle rows %d+%d sweep %d' % (row0, nrows, s))
        # the restatement's shard against its own full grid: same uniforms, same criteria, same permutation up to the offset
        f = full[s][2]
        sl = slice(row0 * ppr, (row0 + nrows) * ppr)
        np.testing.assert_array_equal(ref.u, f.u[sl])
        np.testing.assert_array_equal(ref.dh, f.dh[sl])
        np.testing.assert_array_equal(ref.perm, f.perm[row0 * nt:(row0 + nrows) * nt] - row0 * nt)


def _edge_grid():
    npn = len(R.EDGE_PAIRS)
    P, T = np.linspace(1.0, 8.0, npn, dtype=np.float32), np.array(R.EDGE_T, dtype=np.float32)
    return npn, P, T


def test_edge_uniforms_against_exact_criteria(oracle):
    """u <= min(1, exp(dh)) where exp gives exactly 1, underflows to 0 and overflows: through the tape, on the restatement and the oracle"""
    npn, P, T = _edge_grid()
    et, pf = R.constants_lj(P, T)
    th = R.edge_pair_thermo()
    tape = np.array([u for _, _, u, _ in R.EDGE_PAIRS])
    want = [sw for _, _, _, sw in R.EDGE_PAIRS]
    etot, vol = th[:, 1] + th[:, 2], th[:, 4]
    ref = R.sweep(npn, 2, 0, npn, R.SEED, 0, etot, vol, et, pf, tape=tape)
    np.testing.assert_array_equal(ref.dh.astype(np.float64), R.EDGE_DH)             # exact by construction
    got = [ref.perm[2 * r] == 2 * r + 1 for r in range(npn)]
    assert got == want and ref.swaps == sum(want)
    swaps, perm, _, _, crit = oracle.exchange(npn, 2, 0, npn, R.SEED, 0, etot, vol, et, pf, tape=tape)
    assert swaps == ref.swaps and list(perm) == list(ref.perm)
    np.testing.assert_array_equal(crit, R.EDGE_DH)
    with np.errstate(over='ignore'):
        e = np.exp(np.array(R.EDGE_DH))
    assert e[0] == 1.0 and e[1] == 0.0 and np.isinf(e[3])                            # what the float64 paths meet at these criteria


def test_edge_overflow_on_energies_alone(oracle):
    """dh = 0 and dh = +800 swap under any uniform, dh = -1000 under none that Philox can give but 0: the three implementations on Philox"""
    npn, P, T = _edge_grid()
    et, pf = R.constants_lj(P, T)
    th = R.edge_pair_thermo()
    etot, vol = th[:, 1] + th[:, 2], th[:, 4]
    want = [dh >= 0 for dh in R.EDGE_DH]
    for step in range(4):
        ref = R.sweep(npn, 2, 0, npn, R.SEED, step, etot, vol, et, pf)
        assert (ref.u > 0).all()
        assert [ref.perm[2 * r] == 2 * r + 1 for r in range(npn)] == want
        swaps, perm, _, _, _ = oracle.exchange(npn, 2, 0, npn, R.SEED, step, etot, vol, et, pf)
        p, sw = X.sweep(npn, 2, R.SEED, step, etot, vol, et, pf)
        assert swaps == sw == ref.swaps and list(perm) == list(p) == list(ref.perm)


@pytest.mark.parametrize('step', [0, 1, 2])
def test_a_nan_energy_never_moves_and_changes_nothing_else(oracle, step):
    nt = 5
    P, T = R.grids(1, nt)
    et, pf = R.constants_lj(P, T)
    th = R.edge_row_thermo('nan', nt)
    etot, vol = th[:, 1] + th[:, 2], th[:, 4]
    ref = R.sweep(1, nt, 0, 1, R.SEED, step, etot, vol, et, pf)
    assert ref.perm[2] == 2 and np.isnan(ref.dh).sum() == nt - 1
    # ... as without it: the finite row, with the uniforms of that slot's pairs replaced by 2 (no swap whatever the criterion)
    tape = ref.u.copy()
    tape[[q for q, (v, w) in enumerate(R.pair_slots(nt)) if 2 in (v, w)]] = 2.0
    fin = R.edge_row_thermo('finite', nt)
    alone = R.sweep(1, nt, 0, 1, R.SEED, step, fin[:, 1] + fin[:, 2], fin[:, 4], et, pf, tape=tape)
    np.testing.assert_array_equal(ref.perm, alone.perm)
    assert ref.swaps == alone.swaps > 0
    R.check_margins(ref, 'nan row, step %d' % step)
    swaps, perm, _, _, crit = oracle.exchange(1, nt, 0, 1, R.SEED, step, etot, vol, et, pf)
    p, sw = X.sweep(1, nt, R.SEED, step, etot, vol, et, pf)
    assert swaps == sw == ref.swaps and list(perm) == list(p) == list(ref.perm)
    fin_pairs = _same_nonfinite(crit, ref.dh)
    assert (np.abs(crit[fin_pairs] - ref.dh[fin_pairs].astype(np.float64)) <= ref.bound[fin_pairs]).all()


@pytest.mark.parametrize('step', [0, 1, 2])
def test_infinite_energies(oracle, step):
    """pe = +inf against -inf and against another +inf: dh = -inf (exp 0: no swap), +inf (exp inf: swap) and NaN (no swap)"""
    nt = 5
    P, T = R.grids(1, nt)
    et, pf = R.constants_lj(P, T)
    th = R.edge_row_thermo('inf', nt)
    etot, vol = th[:, 1] + th[:, 2], th[:, 4]
    ref = R.sweep(1, nt, 0, 1, R.SEED, step, etot, vol, et, pf)
    dh = ref.dh.astype(np.float64)
    assert np.isnan(dh).any() and (dh == np.inf).any() and (dh == -np.inf).any()
    R.check_margins(ref, 'inf row, step %d' % step)
    swaps, perm, _, _, crit = oracle.exchange(1, nt, 0, 1, R.SEED, step, etot, vol, et, pf)
    p, sw = X.sweep(1, nt, R.SEED, step, etot, vol, et, pf)
    assert swaps == sw == ref.swaps and list(perm) == list(p) == list(ref.perm)
    _same_nonfinite(crit, dh)
