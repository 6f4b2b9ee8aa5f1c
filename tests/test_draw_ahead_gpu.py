"""The production form of the 4^3 kernels draws the random numbers of the next move — its roll, and the gaussians of a trajectory's velocities,
the displacement uniforms of a position move or the uniform of a volume move — and the acceptance uniform of the move that is ending under
the exchange that completes an energy evaluation, between the publication of the partial sums and the poll for the peers' (nm_kernels.h
draw_ahead).  Every draw is a function of (move, step, seed, slot, atom) alone, so where it is made cannot matter:
NM_DRAW_AHEAD=0 makes the same function draw them behind that exchange, on the serial path, and the bar is that the two agree BIT FOR BIT —
states, step sizes, thermo rows, the permutation, work statistics, records — for every 4^3 cluster row, every pair of successive move kinds
and every launch form.
Stats column 11 counts the moves whose draws were made ahead: none with the switch off, every move of the run with it on."""
import functools

import numpy as np
import pytest

from helpers import grids

pytestmark = pytest.mark.gpu

# (element, workgroups per replica): LJ and Al on every cluster row they have, Cu for the n = 9 kernels
CASES = [('LJ', 2), ('LJ', 4), ('LJ', 8), ('Al', 2), ('Al', 4), ('Cu', 4)]
STATS_COLS = [0, 1, 2, 3, 10]   # evaluations, list rebuilds, energy evaluations, interacting pairs; trajectories started without a hand-over
MOD = 16
# move mixes: the default; trajectory after trajectory; 0.4/0.4: every pair of successive move kinds, bulk after bulk and volume after volume
# included; a one-step trajectory (the start is followed at once by the closing evaluation); blocks of ONE move (nothing but move 0 is drawn)
VARIANTS = {'default': dict(), 'hmc_only': dict(ppos=0.0, pvol=0.0), 'mixed': dict(ppos=0.4, pvol=0.4), 'one_step': dict(nstps=1),
            'mod_1': dict(mod=1)}


def _grid(el):
    """1 pressure x 2 temperatures of 256 atoms: a cold crystal and a hot fluid"""
    return grids(1, 2, (1.0, 8.0), (0.25, 2.5) if el == 'LJ' else (256.0, 2560.0))


def _engine(el, state, **kw):
    import neuralmelting_amd as nm
    P, T = _grid(el)
    e = nm.Engine(256, P, T, element=el, **kw)
    e.set_state(*state)
    return e


@functools.lru_cache(maxsize=None)
def _equilibrated(el):
    """the lattice after 12 cycles of 16 moves, the step sizes as adapt left them: moves of all three kinds are accepted and rejected.  Computed
    once per element, shared by all cases and never changed."""
    from neuralmelting_amd import lattice
    P, T = _grid(el)
    e = _engine(el, lattice.init_states(4, P, T, 0.03125, 0.03125, el=el))
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


def _run(el, cus, kw, trace=False):
    """run_block(mod), run_cycles(3, mod) as one launch, run_cycles_recorded(3, mod) with its records; then the counters of the whole run.
    trace: the block is run with a per-move trace, which takes it through the general form."""
    kw = dict(kw)
    mod = kw.pop('mod', MOD)
    e = _engine(el, _equilibrated(el), **kw)
    assert e.cus_per_replica == cus
    out = []
    e.set_step(12)
    if trace:
        e.set_trace(True)
    e.run_block(mod)
    out.append(_everything(e))
    if trace:
        e.set_trace(False)
    e.adapt()
    e.exchange(count=False)
    e.set_step(13)
    e.run_cycles(3, mod)
    out.append(_everything(e))
    e.set_step(16)
    e.run_cycles_recorded(3, mod)
    recs = [e.snapshot_fetch() for _ in range(3)]
    out.append(_everything(e))
    out.append(dict(rows=np.array([r[0] for r in recs]), x=np.array([r[1] for r in recs]), box=np.array([r[2] for r in recs])))
    assert e.note() == '' and e.heals == 0
    st = e.stats()
    e.close()
    return out, st


def _assert_same(a, b):
    assert len(a) == len(b)
    for n, (g, w) in enumerate(zip(a, b)):
        assert sorted(g) == sorted(w)
        for key in w:
            np.testing.assert_array_equal(g[key], w[key], err_msg='%s of stage %d' % (key, n))


@pytest.mark.parametrize('variant', sorted(VARIANTS))
@pytest.mark.parametrize('el,cus', CASES)
def test_drawn_ahead_equals_drawn_behind_the_exchange(monkeypatch, el, cus, variant):
    kw = VARIANTS[variant]
    mod = kw.get('mod', MOD)
    monkeypatch.setenv('NM_CUS_PER_REPLICA', str(cus))
    monkeypatch.setenv('NM_FUSED_CYCLES', 'all')
    monkeypatch.setenv('NM_DRAW_AHEAD', '0')
    off, st_off = _run(el, cus, kw)
    monkeypatch.delenv('NM_DRAW_AHEAD')
    on, st_on = _run(el, cus, kw)
    print('%s Q=%d %s: blocks %s, moves drawn ahead %s (off: %s), trajectories %s' % (el, cus, kw, st_on[:, 6], st_on[:, 11], st_off[:, 11],
                                                                                   st_on[:, 7]))
    _assert_same(on, off)
    assert (st_off[:, 11] == 0).all()
    assert (st_on[:, 6] == 7).all() and (st_on[:, 11] == 7 * mod).all()      # seven blocks per slot, every move of them
    # not vacuous: the mixes run the kinds of moves they are meant to (.thrm columns 8, 10, 12: position, volume and HMC trials)
    trials = on[0]['thermo'][:, [8, 10, 12]].sum(axis=0) + on[3]['rows'][:, :, [8, 10, 12]].sum(axis=(0, 1))
    if variant == 'hmc_only':
        assert trials[0] == 0 and trials[1] == 0 and trials[2] == 2 * 4 * mod
    if variant == 'mixed':
        assert (trials > 0).all()


def test_general_form_equals_the_production_form_drawn_ahead(monkeypatch):
    """a block with a trace runs the general form, which draws where it always did: equal to the production form's block, and no move of it
    counts as drawn ahead"""
    monkeypatch.setenv('NM_CUS_PER_REPLICA', '4')
    monkeypatch.setenv('NM_FUSED_CYCLES', 'all')
    monkeypatch.delenv('NM_DRAW_AHEAD', raising=False)
    kw = VARIANTS['mixed']
    general, st_g = _run('LJ', 4, kw, trace=True)
    production, st_p = _run('LJ', 4, kw)
    _assert_same(general, production)
    assert (st_p[:, 11] == 7 * MOD).all() and (st_g[:, 11] == 6 * MOD).all()    # (the six fused cycles behind the traced block are production form)
