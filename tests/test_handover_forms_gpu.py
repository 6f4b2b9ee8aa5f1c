"""The cluster hand-over's error path in every workgroup of every 4^3 cluster row, in both forms of the kernels.  The test that accepts a
handed-over granule (nm_math.h granule_state, nm_kernels.h get_granules) tells valid from valid-and-poisoned: a workgroup whose list overflowed
publishes under the poison mark, its peers take the status over from the granule, and the whole cluster leaves the block.  Driven by fault
injection (NM_INJECT_OVERFLOW=n,q: the n-th rebuild of a block overflows in workgroup q, tests/test_properties_gpu.py).

Grid, start and MOD are those of tests/test_production_form_sizes_gpu.py (1 pressure x 2 temperatures of 256 atoms, a cold crystal and a hot
fluid, equilibrated).  For (LJ, Q = 2, 4, 8) and (Al, Q = 2, 4), every q < Q, as built and with NM_PLAIN_KERNELS=0:
  * one run_block stops every slot with the list-overflow status and nothing else (no 2 s hand-over timeout);
  * the state read back is the state before the block, bit for bit;
  * re-issued without the injection, the block equals a clean run bit for bit.
n comes from the clean run's rebuilds move by move: the latest rebuild that every slot makes, and of those one inside an HMC trajectory —
where the other workgroups learn of the overflow from position granules alone — if there is one.  From this start there is one for Al (both
slots rebuild inside trajectories) and none for LJ: its cold crystal builds its lists once, at the block's first evaluation, so the rebuild
that stops every LJ slot is that one (n = 0, the peers learn from the partial sums).  Wherever that is so the trajectory gets a second
injection, at the first rebuild that lies inside a trajectory in every slot that makes it: those slots stop as above, the others complete
the block and equal the clean run bit for bit.
And Q = 4, LJ once more through run_cycles as one fused launch.  (The hand-over's timeout branch has no GPU test: it needs a cluster that is
not co-resident and a 2 s spin.)"""
import functools

import numpy as np
import pytest

from test_production_form_sizes_gpu import MOD, _engine, _equilibrated

pytestmark = pytest.mark.gpu

CASES = [('LJ', 2), ('LJ', 4), ('LJ', 8), ('Al', 2), ('Al', 4)]
STEP0 = 12                  # the equilibrated start has made cycles 0 .. 11
ST_LIST_OVERFLOW = 1        # include/nm.h NM_ST_LIST_OVERFLOW
NTH = 12                    # thermo column: Hamiltonian moves tried


def _prepare(monkeypatch, el, cus, plain):
    start = _equilibrated(el)   # (made at the default cluster size, in front of the switches below, as in the file it comes from)
    monkeypatch.delenv('NM_INJECT_OVERFLOW', raising=False)
    monkeypatch.setenv('NM_CUS_PER_REPLICA', str(cus))
    monkeypatch.setenv('NM_FUSED_CYCLES', 'all')
    if plain:
        monkeypatch.delenv('NM_PLAIN_KERNELS', raising=False)
    else:
        monkeypatch.setenv('NM_PLAIN_KERNELS', '0')
    return start


def _fresh(el, cus, start):
    e = _engine(256, el, start)
    assert e.cus_per_replica == cus
    e.set_step(STEP0)
    return e


def _state(e):
    x, v, box, d = e.get_state()
    return dict(x=x, v=v, box=box, d=d)


def _result(e):
    e.synchronize()
    assert (e.status() == 0).all() and e.note() == '' and e.heals == 0
    return dict(_state(e), thermo=e.thermo())


@functools.lru_cache(maxsize=None)
def _injections(el, cus):
    """(n_all, n_traj, reach) from the clean block, move by move.  A block of m moves is the first m moves of the block of MOD (the draws are
    counter-based), so the rebuilds and the Hamiltonian moves of move m are the differences of the counters of the blocks of m and m - 1
    moves.  n_all: the rebuild (counted from 0, as the injection counts) that stops EVERY slot — the latest that all slots make and that lies
    inside a Hamiltonian move in all of them, else the latest that all slots make.  n_traj: n_all if that lies inside trajectories; else the
    first rebuild that lies inside a Hamiltonian move in every slot that makes it; reach: the slots that make it.
    Called with the environment of the production form."""
    start = _equilibrated(el)
    rebuilds, hmc = [np.zeros(2)], [np.zeros(2)]
    for m in range(1, MOD + 1):
        e = _fresh(el, cus, start)
        e.run_block(m)
        e.synchronize()
        assert (e.status() == 0).all()
        rebuilds.append(e.stats()[:, 1].copy())
        hmc.append(e.thermo()[:, NTH].copy())
        e.close()
    rebuilds, hmc = np.array(rebuilds), np.array(hmc)        # [m][slot], cumulative
    assert (np.diff(rebuilds, axis=0) >= 0).all() and (np.diff(hmc, axis=0) >= 0).all() and (np.diff(hmc, axis=0) <= 1).all()
    assert rebuilds[1].min() >= 1                            # a block starts with a rebuild

    def in_trajectory(n, k):
        m = int(np.searchsorted(rebuilds[:, k], n, side='right'))   # the move that makes rebuild n, 1-based
        return n >= 1 and hmc[m, k] - hmc[m - 1, k] == 1            # (rebuild 0 is the block's first evaluation)

    common = int(rebuilds[MOD].min())
    inside = [n for n in range(common) if all(in_trajectory(n, k) for k in range(2))]
    if inside:
        return inside[-1], inside[-1], (True, True)
    for n in range(common, int(rebuilds[MOD].max())):
        reach = tuple(bool(rebuilds[MOD, k] > n) for k in range(2))
        if all(in_trajectory(n, k) for k in range(2) if reach[k]):
            return common - 1, n, reach
    raise AssertionError('no rebuild inside a trajectory: rebuilds per move %s, Hamiltonian moves %s'
                         % (np.diff(rebuilds, axis=0).T.tolist(), np.diff(hmc, axis=0).T.tolist()))


def _stops(monkeypatch, e, n, q, run):
    import neuralmelting_amd as nm
    monkeypatch.setenv('NM_INJECT_OVERFLOW', '%d,%d' % (n, q))
    run(e)
    with pytest.raises(nm.NMError) as err:
        e.synchronize()
    monkeypatch.delenv('NM_INJECT_OVERFLOW')
    assert 'neighbour list overflow' in str(err.value) and 'timed out' not in str(err.value)
    return e.status()


def _stops_and_resumes(monkeypatch, el, cus, start, n, q, clean, run):
    """the issue of the block stops every slot and leaves the state alone; the re-issue equals the clean run"""
    e = _fresh(el, cus, start)
    np.testing.assert_array_equal(_stops(monkeypatch, e, n, q, run), ST_LIST_OVERFLOW)   # every slot, and no other bit
    for key, got in _state(e).items():
        np.testing.assert_array_equal(got, start['xvbd'.index(key[0])], err_msg='%s behind the stopped block, n = %d, q = %d' % (key, n, q))
    e.set_step(STEP0)
    run(e)                                                                # the caller re-issues
    again = _result(e)
    e.close()
    for key in clean:
        np.testing.assert_array_equal(again[key], clean[key], err_msg='%s of the re-issued block, n = %d, q = %d' % (key, n, q))


def _stops_the_slots_it_reaches(monkeypatch, el, cus, start, n, q, reach, clean, run, others_complete=True):
    e = _fresh(el, cus, start)
    reach = np.array(reach)
    np.testing.assert_array_equal(_stops(monkeypatch, e, n, q, run), np.where(reach, ST_LIST_OVERFLOW, 0))
    for key, got in _state(e).items():
        want = start['xvbd'.index(key[0])]
        np.testing.assert_array_equal(got[reach], want[reach], err_msg='%s behind the stopped block, n = %d, q = %d' % (key, n, q))
        if others_complete and key != 'd':
            np.testing.assert_array_equal(got[~reach], clean[key][~reach], err_msg='%s of the slots that completed, n = %d, q = %d' % (key, n, q))
    e.close()


@pytest.mark.parametrize('el,cus', CASES)
def test_an_overflow_in_any_workgroup_stops_the_cluster_and_the_block_can_be_reissued(monkeypatch, el, cus):
    _prepare(monkeypatch, el, cus, True)
    n_all, n_traj, reach = _injections(el, cus)
    run = lambda e: e.run_block(MOD)
    hit = set()
    for plain in (True, False):
        start = _prepare(monkeypatch, el, cus, plain)
        e = _fresh(el, cus, start)
        run(e)
        clean = _result(e)
        assert e.stats()[:, 1].min() > n_all                              # every slot makes that rebuild
        e.close()
        for q in range(cus):
            _stops_and_resumes(monkeypatch, el, cus, start, n_all, q, clean, run)
            if n_traj != n_all:
                _stops_the_slots_it_reaches(monkeypatch, el, cus, start, n_traj, q, reach, clean, run)
            hit.add((plain, q))
    print('%s Q=%d: rebuild %d stops every slot, rebuild %d lies inside a trajectory (slots %s)' % (el, cus, n_all, n_traj, reach))
    assert any(reach) and hit == {(plain, q) for plain in (True, False) for q in range(cus)}


def test_the_same_inside_a_fused_launch(monkeypatch):
    el, cus = 'LJ', 4
    start = _prepare(monkeypatch, el, cus, True)
    n_all, n_traj, reach = _injections(el, cus)
    run = lambda e: e.run_cycles(2, MOD)                                  # one launch (NM_FUSED_CYCLES=all); its first block stops
    e = _fresh(el, cus, start)
    run(e)
    clean = _result(e)
    e.close()
    hit = set()
    for q in range(cus):
        _stops_and_resumes(monkeypatch, el, cus, start, n_all, q, clean, run)
        if n_traj != n_all:   # (what a slot that completed its block does behind a stopped one is tests/test_cycles_gpu.py's matter)
            _stops_the_slots_it_reaches(monkeypatch, el, cus, start, n_traj, q, reach, clean, run, others_complete=False)
        hit.add(q)
    assert any(reach) and hit == set(range(cus))
