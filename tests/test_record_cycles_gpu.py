"""nm_run_cycles_recorded: recorded cycles of the main loop (remcmc:977-995 with write_outputs) as one call.  The bar: the chains and every record
equal, bit for bit, the single path — nm_run_block + nm_snapshot + nm_adapt + nm_exchange per cycle — on the fused launch and on the loop of single
launches, for every instantiation of the recording kernel; the records share the snapshot queue in cycle order; a healed launch records again; a record
of a block that did not complete is never handed out, and neither is a snapshot, which is a record of one cycle."""
import time

import numpy as np
import pytest

from helpers import grids
from test_cycles_gpu import _everything

pytestmark = pytest.mark.gpu


def _engine(sz, P, T, el, state):
    import neuralmelting_amd as nm
    e = nm.Engine(4 * sz ** 3, P, T, element=el)
    e.set_state(*state)
    return e


def _single_rec(e, step0, ncyc, mod):
    """the single path of recorded cycles: block, snapshot, adapt, exchange"""
    out = []
    for s in range(step0, step0 + ncyc):
        e.set_step(s)
        e.run_block(mod)
        e.snapshot()
        e.adapt()
        e.exchange(count=False)
        out.append(e.snapshot_fetch())
    return out


def _recorded(e, step0, ncyc, mod):
    e.set_step(step0)
    e.run_cycles_recorded(ncyc, mod)
    assert e.snapshot_pending == ncyc
    out = [e.snapshot_fetch() for _ in range(ncyc)]
    assert e.snapshot_pending == 0
    return out


def _same(got, want):
    assert len(got) == len(want)
    for c, (g, w) in enumerate(zip(got, want)):
        for name, a, b in zip(('rows', 'x', 'box'), g, w):
            np.testing.assert_array_equal(a, b, err_msg='cycle %d %s' % (c, name))


def _same_state(g, w):
    assert (g['status'] == 0).all()
    for key in w:
        np.testing.assert_array_equal(g[key], w[key], err_msg=key)


def _states(sz, P, T, el='LJ'):
    from neuralmelting_amd import lattice
    return lattice.init_states(sz, P, T, 0.03125, 0.03125, el=el)


@pytest.mark.parametrize('fused_env', [None, '0'])
@pytest.mark.parametrize('cus', [4, 2])
def test_recorded_cycles_equal_the_single_path(monkeypatch, cus, fused_env):
    P, T = grids(8, 8)
    st = _states(4, P, T)
    monkeypatch.setenv('NM_CUS_PER_REPLICA', str(cus))
    if fused_env is not None:
        monkeypatch.setenv('NM_FUSED_CYCLES', fused_env)
    ncyc, mod = 6, 8
    a = _engine(4, P, T, 'LJ', st)
    assert a.cus_per_replica == cus
    a.timing_reset()
    got = _recorded(a, 5, ncyc, mod)
    g = _everything(a)
    assert a.timing()[0] == (ncyc if fused_env == '0' else 1)
    assert a.heals == 0
    a.close()
    b = _engine(4, P, T, 'LJ', st)
    want = _single_rec(b, 5, ncyc, mod)
    w = _everything(b)
    b.close()
    _same(got, want)
    _same_state(g, w)
    assert not np.array_equal(w['perm'], np.arange(64))     # the rows did exchange
    assert (want[-1][0][:, [8, 10, 12]].sum(1) == mod).all()  # the records are taken in front of gen_mc_params: the block's trials, not zeros


# every other instantiation of nm_cycles_kernel<C, true>: Sutton-Chen at 4 and 2 workgroups, LJ 4^3 at 8, the 6^3 cluster of eight
REC_CASES = [('Al', 4, 8, 8, 4), ('Al', 4, 16, 8, 2), ('LJ', 4, 4, 8, 8), ('LJ', 6, 4, 8, 8)]


@pytest.mark.parametrize('el,sz,npn,ntn,cus', REC_CASES)
def test_every_recording_instantiation_equals_the_single_path(monkeypatch, el, sz, npn, ntn, cus):
    monkeypatch.setenv('NM_FUSED_CYCLES', 'all')
    pr, tr = ((1.0, 8.0), (0.25, 2.5)) if el == 'LJ' else ((1.0, 8.0), (256.0, 2560.0))
    P, T = grids(npn, ntn, pr, tr)
    st = _states(sz, P, T, el)
    ncyc, mod = (4, 12) if sz == 4 else (3, 6)
    a = _engine(sz, P, T, el, st)
    assert a.cus_per_replica == cus
    a.timing_reset()
    got = _recorded(a, 7, ncyc, mod)
    g = _everything(a)
    assert a.timing()[0] == 1
    a.close()
    b = _engine(sz, P, T, el, st)
    want = _single_rec(b, 7, ncyc, mod)
    w = _everything(b)
    b.close()
    _same(got, want)
    _same_state(g, w)


def test_capacity_long_calls_and_the_two_ring_limit():
    import neuralmelting_amd as nm
    from neuralmelting_amd import _lib as B
    P, T = grids(8, 8)
    st = _states(4, P, T)
    a = _engine(4, P, T, 'LJ', st)
    assert a.record_capacity == 64                           # 64 x 64 slots x (768 + 19) doubles: 26 MB, inside the budget
    a.set_step(0)
    with pytest.raises(nm.NMError) as ei:
        a.run_cycles_recorded(70, 1)
    assert ei.value.code == B.NM_ERR_ARG and a.snapshot_pending == 0
    for bad in (0, -1):
        with pytest.raises(nm.NMError) as ei:
            a.run_cycles_recorded(bad, 1)
        assert ei.value.code == B.NM_ERR_ARG
    a.timing_reset()
    got = _recorded(a, 0, 64, 1)                            # a whole ring: one launch of 64 cycles
    assert a.timing()[0] == 1
    # two calls pending: a third is refused and queues nothing
    a.set_step(64)
    a.run_cycles_recorded(2, 1)
    a.set_step(66)
    a.run_cycles_recorded(3, 1)
    assert a.snapshot_pending == 5
    a.set_step(69)
    with pytest.raises(nm.NMError) as ei:
        a.run_cycles_recorded(1, 1)
    assert ei.value.code == B.NM_ERR_STATE and a.snapshot_pending == 5
    got += [a.snapshot_fetch() for _ in range(2)]
    assert a.snapshot_pending == 3
    a.run_cycles_recorded(1, 1)                              # one ring is free again
    assert a.snapshot_pending == 4
    got += [a.snapshot_fetch() for _ in range(4)]
    assert a.snapshot_pending == 0
    with pytest.raises(nm.NMError) as ei:
        a.snapshot_fetch()
    assert ei.value.code == B.NM_ERR_STATE
    g = _everything(a)
    a.close()
    b = _engine(4, P, T, 'LJ', st)
    want = _single_rec(b, 0, 70, 1)
    w = _everything(b)
    b.close()
    _same(got, want)
    _same_state(g, w)


def test_records_and_snapshots_share_one_queue_in_cycle_order():
    P, T = grids(8, 8)
    st = _states(4, P, T)
    mod = 8
    a = _engine(4, P, T, 'LJ', st)

    def single(s):
        a.set_step(s)
        a.run_block(mod)
        a.snapshot()
        a.adapt()
        a.exchange(count=False)
    single(0)
    a.set_step(1)
    a.run_cycles_recorded(2, mod)
    single(3)
    a.set_step(4)
    a.run_cycles_recorded(2, mod)
    assert a.snapshot_pending == 6                           # two snapshots and two calls' records, nothing fetched yet
    got = [a.snapshot_fetch() for _ in range(6)]
    g = _everything(a)
    a.close()
    b = _engine(4, P, T, 'LJ', st)
    want = _single_rec(b, 0, 6, mod)
    w = _everything(b)
    b.close()
    _same(got, want)
    _same_state(g, w)


def test_a_recorded_launch_that_is_not_resident_records_again_when_reissued(monkeypatch):
    """the census of the recorded fused launch fails (NM_INJECT_CENSUS): nothing ran and no record is tagged; the fetch settles the queue, which
    re-issues the launch at 2 workgroups per replica into the same ring — records and chains are those of a context at 2 from the start"""
    P, T = grids(8, 8)
    st = _states(4, P, T)
    ncyc, mod = 4, 12
    monkeypatch.setenv('NM_INJECT_CENSUS', '0')
    a = _engine(4, P, T, 'LJ', st)
    assert a.cus_per_replica == 4
    got = _recorded(a, 3, ncyc, mod)
    monkeypatch.delenv('NM_INJECT_CENSUS')
    assert a.cus_per_replica == 2 and a.heals == 1
    g = _everything(a)
    a.close()
    monkeypatch.setenv('NM_CUS_PER_REPLICA', '2')
    b = _engine(4, P, T, 'LJ', st)
    want = _single_rec(b, 3, ncyc, mod)
    w = _everything(b)
    b.close()
    _same(got, want)
    _same_state(g, w)


def test_a_snapshot_behind_a_block_that_did_not_complete_is_taken_again_or_reported(monkeypatch):
    """a snapshot is a record: behind a block whose census fails (NM_INJECT_CENSUS), with the next cycle queued before the fetch as the driver does,
    the fetch settles the queue, which re-issues both cycles at 2 workgroups per replica — snapshots and chains are those of a context at 2 from the
    start; behind a block that stops on an injected list overflow, the fetch is NM_ERR_STATE with the reason, never the state from before the block"""
    import neuralmelting_amd as nm
    from neuralmelting_amd import _lib as B
    P, T = grids(8, 8)
    st = _states(4, P, T)
    ncyc, mod = 4, 12
    monkeypatch.setenv('NM_INJECT_CENSUS', '0')
    a = _engine(4, P, T, 'LJ', st)
    assert a.cus_per_replica == 4
    got = []
    for s in range(3, 3 + ncyc):
        a.set_step(s)
        a.run_block(mod)
        a.snapshot()
        a.adapt()
        a.exchange(count=False)
        if s > 3:
            got.append(a.snapshot_fetch())                   # the cycle before this one
    got.append(a.snapshot_fetch())
    monkeypatch.delenv('NM_INJECT_CENSUS')
    assert a.cus_per_replica == 2 and a.heals == 1 and a.snapshot_pending == 0
    g = _everything(a)
    a.close()
    monkeypatch.setenv('NM_CUS_PER_REPLICA', '2')
    b = _engine(4, P, T, 'LJ', st)
    want = _single_rec(b, 3, ncyc, mod)
    w = _everything(b)
    b.close()
    _same(got, want)
    _same_state(g, w)
    monkeypatch.delenv('NM_CUS_PER_REPLICA')

    e = _engine(4, P, T, 'LJ', st)
    e.run_block(8)
    e.synchronize()
    monkeypatch.setenv('NM_INJECT_OVERFLOW', '3,1')
    e.set_step(1)
    e.run_block(48)
    e.snapshot()
    e.adapt()
    e.exchange(count=False)
    monkeypatch.delenv('NM_INJECT_OVERFLOW')
    with pytest.raises(nm.NMError) as ei:
        e.snapshot_fetch()
    assert ei.value.code == B.NM_ERR_STATE and 'neighbour list overflow' in str(ei.value)
    assert e.snapshot_pending == 0
    e.close()


def test_a_record_of_a_block_that_did_not_complete_is_never_handed_out(monkeypatch):
    """an injected list overflow inside the recorded fused launch: the records of the cycles that completed are those of a clean run, the first fetch
    of a cycle that did not complete is NM_ERR_STATE with the reason, the call's other records are dropped, and the grid drains at once"""
    import neuralmelting_amd as nm
    from neuralmelting_amd import _lib as B
    P, T = grids(8, 8)
    st = _states(4, P, T)
    b = _engine(4, P, T, 'LJ', st)
    b.run_block(8)
    want = _single_rec(b, 1, 6, 48)
    b.close()
    e = _engine(4, P, T, 'LJ', st)
    e.run_block(8)
    e.synchronize()
    monkeypatch.setenv('NM_INJECT_OVERFLOW', '3,1')
    e.set_step(1)
    t0 = time.perf_counter()
    e.run_cycles_recorded(6, 48)
    got, err = [], None
    for _ in range(6):
        try:
            got.append(e.snapshot_fetch())
        except nm.NMError as x:
            err = x
            break
    assert time.perf_counter() - t0 < 1.0                    # six cycles are ~35 ms; a timeout would be 2 s
    monkeypatch.delenv('NM_INJECT_OVERFLOW')
    assert err is not None and err.code == B.NM_ERR_STATE and 'neighbour list overflow' in str(err)
    assert e.snapshot_pending == 0
    _same(got, want[:len(got)])
    e.close()


def test_driver_recorded_run_writes_the_same_files_fused_or_not(tmp_path, monkeypatch):
    """-sc 0 of 12 cycles on the 8 x 8 grid, restart dump every 5: cycles 0-3 and 5-8 go to the engine as run_cycles_recorded (one launch each on
    this grid), the dump cycles, cycle 10 and the last the single way; every file equals the one of a run whose engine makes single launches"""
    import os
    from neuralmelting_amd import remcmc
    from test_driver import check_outputs, run_driver
    argv = '-bm -e LJ -ss 4 -pn 8 -tn 8 -sn 12 -sm 8 -sc 0 -rd 5 -n q'.split()
    calls = []

    def counting(run):
        eng = remcmc.Run.make_engine(run)
        inner = eng.run_cycles_recorded

        def rec(n, mod):
            calls.append(n)
            inner(n, mod)
        eng.run_cycles_recorded = rec
        return eng
    a = tmp_path / 'a'; b = tmp_path / 'b'
    a.mkdir(); b.mkdir()
    ra = run_driver(a, argv, counting)
    monkeypatch.setenv('NM_FUSED_CYCLES', '0')
    run_driver(b, argv)
    monkeypatch.delenv('NM_FUSED_CYCLES')
    assert calls == [4, 4]
    check_outputs(a, ra, nrec=12)
    names = sorted(os.listdir(b))
    assert names == sorted(os.listdir(a)) and any(n.endswith('.thrm') for n in names)
    for f in names:
        assert open(os.path.join(a, f), 'rb').read() == open(os.path.join(b, f), 'rb').read(), f
