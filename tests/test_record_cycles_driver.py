"""Recorded cycles as one call (nm_run_cycles_recorded), host side: the driver sends the cycles that record but neither dump nor end the run to the
engine as one run_cycles_recorded call of at most record_capacity cycles, fetches their records from the snapshot queue in cycle order, and leaves
the same files as a driver whose engine has no such call.  The engine here is the oracle stand-in (no GPU)."""
import ctypes as C
import os

import numpy as np

from helpers import OracleEngine
from test_abi import declared_symbols

NEW = ('nm_run_cycles_recorded', 'nm_record_capacity', 'nm_snapshot_pending')


def _recording(cap, calls):
    class Recording(OracleEngine):
        """run_cycles_recorded as the single path would run it: per cycle block, snapshot, adapt, exchange"""
        record_capacity = cap

        def run_cycles(self, ncycles, mod):
            calls.append(('run_cycles', self.step, ncycles))
            OracleEngine.run_cycles(self, ncycles, mod)

        def snapshot(self):
            """nm_snapshot's limit counts its own pending snapshots only, not records of recorded calls"""
            if not hasattr(self, '_snaps'):
                self._snaps = []
            assert sum(1 for s in self._snaps if s[3] is None) < 2, 'two snapshots are pending'
            lp = self.loop
            self._snaps.append((lp.rows().copy(), lp.x.copy(), lp.box.copy(), None))

        def snapshot_fetch(self, positions=True):
            rows, x, box, _ = self._snaps.pop(0)
            return rows, (x if positions else None), box

        def run_cycles_recorded(self, ncycles, mod):
            assert 1 <= ncycles <= self.record_capacity
            calls.append(('run_cycles_recorded', self.step, ncycles))
            assert len({s[3] for s in getattr(self, '_snaps', ()) if s[3] is not None}) < 2, 'records of two calls are pending'
            if not hasattr(self, '_snaps'):
                self._snaps = []
            lp = self.loop
            for k in range(ncycles):
                lp.run_block(mod, self.step + k)
                self._snaps.append((lp.rows().copy(), lp.x.copy(), lp.box.copy(), len(calls)))
                lp.adapt()
                lp.exchange(self.step + k)
    return Recording


class Plain(OracleEngine):
    run_cycles = property()     # hasattr() is False: the driver takes the cycle-by-cycle path


def _same_files(a, b):
    names = sorted(os.listdir(b))
    assert names == sorted(os.listdir(a)) and any(n.endswith('.thrm') for n in names)
    for f in names:
        fa, fb = os.path.join(a, f), os.path.join(b, f)
        if f.endswith('.npy'):
            xa, xb = np.load(fa, allow_pickle=True), np.load(fb, allow_pickle=True)
            if xa.dtype == object:
                assert all(np.array_equal(np.asarray(u), np.asarray(w)) for ra_, rb_ in zip(xa, xb) for u, w in zip(ra_, rb_)), f
            else:
                assert np.array_equal(xa, xb), f
        else:
            assert open(fa, 'rb').read() == open(fb, 'rb').read(), f


def test_recorded_cycles_go_to_the_engine_as_one_call(tmp_path, oracle):
    """-sc 2 of 8 cycles, restart dump every 5: cycles 0-1 are quiet (run_cycles), 2-3 and 5-6 record without a dump (run_cycles_recorded each),
    cycle 4 dumps and cycle 7 is the last: those go the single way — and every file equals the one of a driver whose engine has neither call"""
    from test_driver import check_outputs, run_driver
    argv = '-bm -e LJ -ss 4 -pn 2 -tn 2 -sn 8 -sm 3 -sc 2 -rd 5 -n r'.split()
    calls = []
    a = tmp_path / 'a'; b = tmp_path / 'b'
    a.mkdir(); b.mkdir()
    ra = run_driver(a, argv, lambda r: _recording(64, calls)(oracle, r))
    run_driver(b, argv, lambda r: Plain(oracle, r))
    assert calls == [('run_cycles', 0, 2), ('run_cycles_recorded', 2, 2), ('run_cycles_recorded', 5, 2)]
    check_outputs(a, ra, nrec=6)
    _same_files(a, b)


def test_a_record_capacity_of_one_means_single_cycles(tmp_path, oracle):
    from test_driver import run_driver
    argv = '-bm -e LJ -ss 4 -pn 2 -tn 2 -sn 8 -sm 3 -sc 2 -rd 5 -n r'.split()
    calls = []
    a = tmp_path / 'a'; b = tmp_path / 'b'
    a.mkdir(); b.mkdir()
    run_driver(a, argv, lambda r: _recording(1, calls)(oracle, r))
    run_driver(b, argv, lambda r: Plain(oracle, r))
    assert calls == [('run_cycles', 0, 2)]
    _same_files(a, b)


def test_a_capacity_smaller_than_the_stretch_splits_it_into_calls(tmp_path, oracle):
    """-sc 0 of 12 cycles, dump every 100: cycles 0-10 record without a dump, cut into calls of at most 3; the calls' records are fetched while
    the next call is queued, and the files are those of the single path"""
    from test_driver import run_driver
    argv = '-bm -e LJ -ss 4 -pn 2 -tn 2 -sn 12 -sm 2 -sc 0 -rd 100 -n r'.split()
    calls = []
    a = tmp_path / 'a'; b = tmp_path / 'b'
    a.mkdir(); b.mkdir()
    run_driver(a, argv, lambda r: _recording(3, calls)(oracle, r))
    run_driver(b, argv, lambda r: Plain(oracle, r))
    assert calls == [('run_cycles_recorded', 0, 3), ('run_cycles_recorded', 3, 3), ('run_cycles_recorded', 6, 3), ('run_cycles_recorded', 9, 2)]
    _same_files(a, b)


def test_the_recorded_call_is_declared_exported_and_bound():
    from neuralmelting_amd import _lib
    L = C.CDLL(_lib.LIB_PATH)
    syms = declared_symbols()
    for s in NEW:
        assert s in syms, s
        assert hasattr(L, s), s
        assert s in _lib.SYMBOLS, s
    from neuralmelting_amd.engine import Engine
    assert hasattr(Engine, 'run_cycles_recorded') and hasattr(Engine, 'record_capacity') and hasattr(Engine, 'snapshot_pending')


def test_calls_shrink_towards_the_end_of_the_run(tmp_path, oracle):
    """a call holds at most half of the cycles left (but 2): the last call's records are written behind the GPU's last cycle, so that tail stays short"""
    from test_driver import run_driver
    argv = '-bm -e LJ -ss 4 -pn 2 -tn 2 -sn 40 -sm 1 -sc 0 -rd 1000 -n r'.split()
    calls = []
    a = tmp_path / 'a'; b = tmp_path / 'b'
    a.mkdir(); b.mkdir()
    run_driver(a, argv, lambda r: _recording(64, calls)(oracle, r))
    run_driver(b, argv, lambda r: Plain(oracle, r))
    assert calls == [('run_cycles_recorded', 0, 20), ('run_cycles_recorded', 20, 10), ('run_cycles_recorded', 30, 5),
                     ('run_cycles_recorded', 35, 3)]
    _same_files(a, b)
