"""The 4^3 cluster kernels start a trajectory without a hand-over wherever every workgroup can make the first kick and drift of ALL atoms itself
(nm_kernels.h advance_and_share modes 4 and 5): the peers' forces come from the board that the energy evaluation in front of
the trajectory published with its partial sums, or, after a rejection, from the saved forces in LDS.  Where neither holds them the first step's
positions are handed over as before, and NM_START_HANDOVER=1 makes every trajectory start that way.  Both starts evaluate the same expression on
the same bits, so the bar is: the two agree BIT FOR BIT — states, step sizes, thermo rows, the permutation, work statistics, records — for every
source of the forces, and stats column 10 shows that each source was in fact used."""
import functools

import numpy as np
import pytest

from helpers import grids

pytestmark = pytest.mark.gpu

# (element, workgroups per replica): every 4^3 cluster row of nm_rows.hip's table
CASES = [('LJ', 2), ('LJ', 4), ('LJ', 8), ('Al', 2), ('Al', 4)]
STATS_COLS = [0, 1, 2, 3]   # evaluations, list rebuilds, energy evaluations, interacting pairs
MOD = 16
# move mixes (ppos, pvol) and trajectory lengths.  0/0: every move a trajectory, so the board after an acceptance and LDS after a rejection;
# 0.4/0.4: trajectories behind accepted and rejected position and volume moves, which reaches the fallback; one step: the start is followed at
# once by the closing evaluation
VARIANTS = {'default': dict(), 'hmc_only': dict(ppos=0.0, pvol=0.0), 'mixed': dict(ppos=0.4, pvol=0.4), 'one_step': dict(nstps=1),
            'two_steps': dict(nstps=2)}


def _grid(el):
    """1 pressure x 2 temperatures of 256 atoms: a cold crystal and a hot fluid"""
    return grids(1, 2, (1.0, 8.0), (0.25, 2.5) if el == 'LJ' else (256.0, 2560.0))


@functools.lru_cache(maxsize=None)
def _lattice(el):
    from neuralmelting_amd import lattice
    P, T = _grid(el)
    state = lattice.init_states(4, P, T, 0.03125, 0.03125, el=el)
    for a in state:
        a.setflags(write=False)
    return state


def _engine(el, state, **kw):
    import neuralmelting_amd as nm
    P, T = _grid(el)
    e = nm.Engine(256, P, T, element=el, **kw)
    e.set_state(*state)
    return e


@functools.lru_cache(maxsize=None)
def _equilibrated(el):
    """the lattice after 12 cycles of 16 moves, the step sizes as adapt left them: trajectories are rejected now and then and the hot replica's
    atoms outrun the skin in mid-trajectory.  Computed once per element, shared by all cases and never changed."""
    e = _engine(el, _lattice(el))
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


def _run(el, cus, state, step0, kw):
    """run_block(16), run_cycles(3, 16) as one launch, run_cycles_recorded(3, 16) with its records; then the counters of the whole run"""
    e = _engine(el, state, **kw)
    assert e.cus_per_replica == cus
    out = []
    e.set_step(step0)
    e.run_block(MOD)
    out.append(_everything(e))
    first = out[0]['thermo'][:, 12:14].sum(axis=0)      # HMC trials and acceptances of the first block (.thrm columns 12, 13)
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
    st = e.stats()
    e.close()
    rec = out[3]['rows'][:, :, 12:14].sum(axis=(0, 1))  # ... and of the three recorded cycles (each record carries its own cycle's counters)
    counters = dict(blocks=st[:, 6].sum(), trajectories=st[:, 7].sum(), no_hop=st[:, 10].sum(), nth=first[0] + rec[0], nah=first[1] + rec[1])
    return out, counters


def _both_starts(monkeypatch, el, cus, state, step0, kw):
    monkeypatch.setenv('NM_CUS_PER_REPLICA', str(cus))
    monkeypatch.setenv('NM_FUSED_CYCLES', 'all')
    monkeypatch.delenv('NM_START_HANDOVER', raising=False)
    built, cb = _run(el, cus, state, step0, kw)
    monkeypatch.setenv('NM_START_HANDOVER', '1')
    handed, ch = _run(el, cus, state, step0, kw)
    print('%s Q=%d %s: as built %s; with the hand-over %s' % (el, cus, kw, cb, ch))
    assert len(built) == len(handed)
    for n, (g, w) in enumerate(zip(built, handed)):
        assert sorted(g) == sorted(w)
        for key in w:
            np.testing.assert_array_equal(g[key], w[key], err_msg='%s of stage %d' % (key, n))
    return cb, ch


@pytest.mark.parametrize('variant', sorted(VARIANTS))
@pytest.mark.parametrize('el,cus', CASES)
def test_from_the_lattice(monkeypatch, el, cus, variant):
    """from the lattice: the first trajectories of a cold start, whose step sizes are the initial ones"""
    cb, ch = _both_starts(monkeypatch, el, cus, _lattice(el), 0, VARIANTS[variant])
    assert ch['no_hop'] == 0 and cb['trajectories'] == ch['trajectories'] > 0


@pytest.mark.parametrize('variant', sorted(VARIANTS))
@pytest.mark.parametrize('el,cus', CASES)
def test_from_the_equilibrated_start(monkeypatch, el, cus, variant):
    """from the equilibrated start: rejected trajectories and rebuilds in mid-trajectory occur.  Not vacuous: the switch takes every start
    through the hand-over and the build as it is takes some without; with trajectories only, every start but possibly a block's first goes
    without (the board after an acceptance, LDS after a rejection); with many position and volume moves some starts fall back to the
    hand-over (a rejected position or volume move behind an accepted move: neither the board nor LDS holds the peers' forces); and
    trajectories are both accepted and rejected."""
    kw = VARIANTS[variant]
    cb, ch = _both_starts(monkeypatch, el, cus, _equilibrated(el), 12, kw)
    assert ch['no_hop'] == 0
    assert cb['no_hop'] > 0
    assert cb['trajectories'] == ch['trajectories'] and cb['no_hop'] <= cb['trajectories']
    if variant == 'hmc_only':
        assert cb['trajectories'] == 2 * 7 * MOD        # two replicas, seven blocks
        assert cb['no_hop'] >= cb['trajectories'] - cb['blocks']
    if variant == 'mixed':
        assert cb['no_hop'] < cb['trajectories']
    assert 0 < cb['nah'] < cb['nth'], (cb['nth'], cb['nah'])
