"""The production form of the 4^3 kernels (nm_kernels.h nm_block_body PLAIN) has its atom count at compile time: it runs full cells only,
256 atoms, and nm_api.hip's plain_call sends every other atom count of the size class to the general form.  Two things are
pinned here on one stage sequence — run_block(16), run_cycles(3, 16) as one launch, run_cycles_recorded(3, 16):
(a) full cells, every 4^3 row of the table, from the lattice and from an equilibrated start: the build as it is and NM_PLAIN_KERNELS=0 agree
    BIT FOR BIT in states, step sizes, thermo rows, the permutation, the records and stats columns 0-3 (tests/test_plain_kernels_gpu.py pins the
    two forms on other sequences; this one adds the recorded cycles behind a block from the lattice and the block from the equilibrated start);
(b) atom counts below NMAX at kind 0 — 108 and 255 — complete the same sequence with status 0, equal NM_PLAIN_KERNELS=0 bit for bit (the
    switch changes nothing: they run the general form whatever it says), and their first block agrees with the oracle's to the tolerances
    tests/test_parity_gpu.py uses for the rows of these sizes (energies 1e-6 relative, counters exact, x 1e-8, v 1e-7)."""
import functools

import numpy as np
import pytest

from helpers import OracleLoop, grids

pytestmark = pytest.mark.gpu

# (element, workgroups per replica): every 4^3 row of nm_rows.hip's table
FULL_CASES = [('LJ', 1), ('LJ', 2), ('LJ', 4), ('LJ', 8), ('Al', 1), ('Al', 2), ('Al', 4)]
STATS_COLS = [0, 1, 2, 3]   # evaluations, list rebuilds, energy evaluations, interacting pairs
MOD = 16
RTOL = 1e-6                 # tests/test_parity_gpu.py: RTOL, and x 1e-8 / v 1e-7 absolute (_block_parity, _short_trajectories_parity)


def _grid(el='LJ'):
    """1 pressure x 2 temperatures: a cold crystal and a hot fluid (tests/test_trajectory_start_gpu.py)"""
    return grids(1, 2, (1.0, 8.0), (0.25, 2.5) if el == 'LJ' else (256.0, 2560.0))


@functools.lru_cache(maxsize=None)
def _lattice(el):
    from neuralmelting_amd import lattice
    state = lattice.init_states(4, *_grid(el), 0.03125, 0.03125, el=el)
    for a in state:
        a.setflags(write=False)
    return state


def _engine(natoms, el, state, **kw):
    import neuralmelting_amd as nm
    P, T = _grid(el)
    e = nm.Engine(natoms, P, T, element=el, **kw)
    e.set_state(*state)
    return e


@functools.lru_cache(maxsize=None)
def _equilibrated(el):
    """the lattice after 12 cycles of 16 moves, the step sizes as adapt left them.  Computed once per element, shared and never changed."""
    e = _engine(256, el, _lattice(el))
    e.set_step(0)
    e.run_cycles(12, MOD)
    e.synchronize()
    state = e.get_state()
    assert (e.status() == 0).all()
    e.close()
    for a in state:
        a.setflags(write=False)
    return state


def _everything(e):
    e.synchronize()
    x, v, box, d = e.get_state()
    assert (e.status() == 0).all()
    return dict(x=x, v=v, box=box, d=d, thermo=e.thermo(), perm=e.perm(), stats=e.stats()[:, STATS_COLS])


def _stages(natoms, el, cus, state, step0):
    """run_block(16), run_cycles(3, 16), run_cycles_recorded(3, 16) with its records"""
    e = _engine(natoms, el, state)
    assert e.cus_per_replica == cus
    out = []
    e.set_step(step0)
    e.run_block(MOD)
    out.append(_everything(e))
    e.adapt()
    e.exchange(count=False)
    e.set_step(step0 + 1)
    e.run_cycles(3, MOD)
    out.append(_everything(e))
    e.set_step(step0 + 4)
    e.run_cycles_recorded(3, MOD)
    recs = [e.snapshot_fetch() for _ in range(3)]
    out.append(_everything(e))
    out.append(dict(rows=np.array([r[0] for r in recs]), x=np.array([r[1] for r in recs]), box=np.array([r[2] for r in recs])))
    assert e.note() == '' and e.heals == 0
    e.close()
    return out


def _both_forms(monkeypatch, natoms, el, cus, state, step0):
    """the stages as built and with the general form forced, compared bit for bit; returns the former"""
    monkeypatch.setenv('NM_CUS_PER_REPLICA', str(cus))
    monkeypatch.setenv('NM_FUSED_CYCLES', 'all')
    monkeypatch.delenv('NM_PLAIN_KERNELS', raising=False)
    built = _stages(natoms, el, cus, state, step0)
    monkeypatch.setenv('NM_PLAIN_KERNELS', '0')
    general = _stages(natoms, el, cus, state, step0)
    assert len(built) == len(general)
    for n, (g, w) in enumerate(zip(built, general)):
        assert sorted(g) == sorted(w)
        for key in w:
            np.testing.assert_array_equal(g[key], w[key], err_msg='%s of stage %d' % (key, n))
    return built


@pytest.mark.parametrize('start', ['lattice', 'equilibrated'])
@pytest.mark.parametrize('el,cus', FULL_CASES)
def test_full_cells_both_forms(monkeypatch, el, cus, start):
    state, step0 = (_lattice(el), 0) if start == 'lattice' else (_equilibrated(el), 12)
    built = _both_forms(monkeypatch, 256, el, cus, state, step0)
    assert built[0]['stats'][:, 0].min() > 0 and built[2]['stats'][:, 0].min() > built[1]['stats'][:, 0].min()   # (the counters count)
    if start == 'equilibrated':  # not vacuous: lists were rebuilt, trajectories were accepted and rejected
        assert built[2]['stats'][:, 1].sum() > built[0]['stats'][:, 1].sum() >= 1
        nth, nah = built[3]['rows'][:, :, 12].sum(), built[3]['rows'][:, :, 13].sum()
        assert 0 < nah < nth, (nth, nah)


@functools.lru_cache(maxsize=None)
def _partial(natoms):
    """108: the 3 x 3 x 3 cells at the origin of the 4^3 lattice states, in the 4^3 box (the box of a 3^3 lattice, 4.63, is below twice the
    cutoff: ST_BOX_TOO_SMALL); 255: the 4^3 lattice less its last atom"""
    x, v, box, d = _lattice('LJ')
    ns = len(box)
    if natoms == 255:
        keep = np.arange(255)
    else:
        site = np.rint(8.0 * x[0].reshape(-1, 3) / box[0]).astype(int) % 8   # half-cell index of the (slightly displaced, wrapped) lattice site
        keep = np.flatnonzero((site < 6).all(axis=1))                       # cells 0 .. 2 of 4 along every axis
    assert len(keep) == natoms
    state = (np.stack([x[k].reshape(-1, 3)[keep].reshape(-1) for k in range(ns)]), np.stack([v[k].reshape(-1, 3)[keep].reshape(-1) for k in range(ns)]),
             box.copy(), d.copy())
    for a in state:
        a.setflags(write=False)
    return state


_ORACLE = {}


def _oracle_block(oracle, natoms):
    """the oracle's first block of the partial state: rows, x, v.  Computed once per atom count, shared by the three cluster sizes."""
    if natoms not in _ORACLE:
        P, T = _grid()
        loop = OracleLoop(oracle, 4, P, T, states=tuple(a.copy() for a in _partial(natoms)))
        loop.run_block(MOD, 0)
        _ORACLE[natoms] = (loop.rows(), loop.x.copy(), loop.v.copy())
    return _ORACLE[natoms]


@pytest.mark.parametrize('natoms', [108, 255])
@pytest.mark.parametrize('cus', [1, 2, 4])
def test_fewer_atoms_than_the_row_holds(oracle, monkeypatch, natoms, cus):
    state = _partial(natoms)
    built = _both_forms(monkeypatch, natoms, 'LJ', cus, state, 0)
    rows_o, x_o, v_o = _oracle_block(oracle, natoms)
    rows, ro = built[0]['thermo'], rows_o
    print('natoms %d Q=%d: max relative deviation of the five thermo columns %.3g, max |dx| %.3g, max |dv| %.3g'
          % (natoms, cus, np.abs(rows[:, :5] / ro[:, :5] - 1.0).max(), np.abs(built[0]['x'] - x_o).max(), np.abs(built[0]['v'] - v_o).max()))
    np.testing.assert_allclose(rows[:, :8], ro[:, :8], rtol=RTOL)
    np.testing.assert_array_equal(rows[:, 8:], ro[:, 8:])
    np.testing.assert_allclose(built[0]['x'], x_o, rtol=0, atol=1e-8)
    np.testing.assert_allclose(built[0]['v'], v_o, rtol=0, atol=1e-7)
