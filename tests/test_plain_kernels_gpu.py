"""The 4^3 kernels are built in two forms (nm_kernels.h nm_block_body PLAIN): the production form without the RNG tape, the per-move trace,
the plain NVE run, nm_eval's force output and the iterative position move, and the general form that carries them all.  nm_api.hip picks
the production form exactly when a call asks for none of those; NM_PLAIN_KERNELS=0 forces the general form.  For a given number of
workgroups per replica the kernels are bitwise reproducible, so the bar is: the two forms agree BIT FOR BIT — states,
thermo rows, counters, work statistics, records — and a call that needs the general form gets it whatever the switch says."""
import functools

import numpy as np
import pytest

from helpers import grids

pytestmark = pytest.mark.gpu

# (element, workgroups per replica): every 4^3 row of nm_rows.hip's table
CASES = [('LJ', 1), ('LJ', 2), ('LJ', 4), ('LJ', 8), ('Al', 1), ('Al', 2), ('Al', 4)]
STATS_COLS = [0, 1, 2, 3]   # evaluations, list rebuilds, energy evaluations, interacting pairs
MOD = 16


def _grid(el):
    """1 pressure x 2 temperatures of 256 atoms: a cold crystal and a hot fluid"""
    return grids(1, 2, (1.0, 8.0), (0.25, 2.5) if el == 'LJ' else (256.0, 2560.0))


def _lattice(el):
    from neuralmelting_amd import lattice
    P, T = _grid(el)
    return lattice.init_states(4, P, T, 0.03125, 0.03125, el=el)


def _engine(el, state, **kw):
    import neuralmelting_amd as nm
    P, T = _grid(el)
    e = nm.Engine(256, P, T, element=el, **kw)
    e.set_state(*state)
    return e


def _everything(e):
    e.synchronize()
    x, v, box, d = e.get_state()
    assert (e.status() == 0).all()
    return dict(x=x, v=v, box=box, d=d, thermo=e.thermo(), perm=e.perm(), stats=e.stats()[:, STATS_COLS])


def _both_forms(monkeypatch, run):
    """run() once as built and once with the general form forced"""
    monkeypatch.delenv('NM_PLAIN_KERNELS', raising=False)
    built = run()
    monkeypatch.setenv('NM_PLAIN_KERNELS', '0')
    general = run()
    return built, general


def _assert_same(built, general):
    assert len(built) == len(general)
    for n, (g, w) in enumerate(zip(built, general)):
        assert sorted(g) == sorted(w)
        for key in w:
            np.testing.assert_array_equal(g[key], w[key], err_msg='%s of stage %d' % (key, n))


@pytest.mark.parametrize('el,cus', CASES)
def test_block_and_cycles_from_the_lattice(monkeypatch, el, cus):
    """run_block(16), then run_cycles(2, 16) (NM_FUSED_CYCLES=all: as one launch at every Q > 1, so that every fused instantiation runs)"""
    monkeypatch.setenv('NM_CUS_PER_REPLICA', str(cus))
    monkeypatch.setenv('NM_FUSED_CYCLES', 'all')
    state = _lattice(el)

    def run():
        e = _engine(el, state)
        assert e.cus_per_replica == cus
        out = []
        e.set_step(0)
        e.run_block(MOD)
        out.append(_everything(e))
        e.adapt()
        e.exchange(count=False)
        e.timing_reset()
        e.set_step(1)
        e.run_cycles(2, MOD)
        out.append(_everything(e))
        assert e.timing()[0] == (1 if cus > 1 else 2)
        assert e.note() == '' and e.heals == 0
        e.close()
        return out

    _assert_same(*_both_forms(monkeypatch, run))


@functools.lru_cache(maxsize=None)
def _equilibrated(el):
    """the lattice after 12 cycles of 16 moves, the step sizes as adapt left them: the trajectories are then long enough to be rejected now and
    then, and the hot replica's atoms outrun the skin.  Computed once per element (workgroups per replica and form as the library picks them:
    a start is a start), shared by the cases below and never changed."""
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


@pytest.mark.parametrize('el,cus', CASES)
def test_cycles_with_rebuilds_and_rejections(monkeypatch, el, cus):
    """3 cycles from the equilibrated start as one launch, then 3 recorded ones (the recording instantiation; their records carry each cycle's
    counters, which nm_run_cycles zeroes behind every cycle): rebuilds, rejected trajectories and the return to the saved list all occur"""
    state = _equilibrated(el)
    monkeypatch.setenv('NM_CUS_PER_REPLICA', str(cus))
    monkeypatch.setenv('NM_FUSED_CYCLES', 'all')

    def run():
        e = _engine(el, state)
        assert e.cus_per_replica == cus
        out = []
        e.set_step(12)
        e.run_cycles(3, MOD)
        out.append(_everything(e))
        e.set_step(15)
        e.run_cycles_recorded(3, MOD)
        recs = [e.snapshot_fetch() for _ in range(3)]
        out.append(_everything(e))
        out.append(dict(rows=np.array([r[0] for r in recs]), x=np.array([r[1] for r in recs]), box=np.array([r[2] for r in recs])))
        assert e.note() == '' and e.heals == 0
        e.close()
        return out

    built, general = _both_forms(monkeypatch, run)
    _assert_same(built, general)
    # not vacuous: lists were rebuilt, and trajectories were both accepted and rejected (.thrm columns 12, 13: HMC trials and acceptances)
    assert built[0]['stats'][:, 1].sum() >= 1 and built[1]['stats'][:, 1].sum() > built[0]['stats'][:, 1].sum()
    nth, nah = built[2]['rows'][:, :, 12].sum(), built[2]['rows'][:, :, 13].sum()
    assert 0 < nah < nth, (nth, nah)


def _tapes(nslots):
    rng = np.random.default_rng(5)
    return [rng.random(8 * MOD) for _ in range(nslots)]


def _run_tape(e):
    e.set_rng_tape(_tapes(e.nslots))
    e.run_block(MOD)
    return [_everything(e)]


def _run_trace(e):
    e.set_trace(True)
    e.run_block(MOD)
    tr = e.trace(MOD)
    assert (tr[:, :, 3] != 0.0).all()        # every move left its row (column 3: the energy behind it)
    return [dict(_everything(e), trace=tr)]


def _run_md(e):
    e.run_md(24)
    return [_everything(e)]


def _run_eval(e):
    U, W, f = e.eval(forces=True)
    assert np.abs(f).max() > 0.0
    return [dict(U=U, W=W, f=f)]


@pytest.mark.parametrize('kw,run', [pytest.param({}, _run_tape, id='tape'), pytest.param({}, _run_trace, id='trace'),
                                    pytest.param(dict(bulk=False, ppos=0.5), _run_trace, id='iterative'),
                                    pytest.param({}, _run_md, id='md'), pytest.param({}, _run_eval, id='eval')])
@pytest.mark.parametrize('el,cus', [('LJ', 4), ('Al', 2)])
def test_calls_the_production_form_leaves_out_get_the_general_form(monkeypatch, el, cus, kw, run):
    """an RNG tape, a trace, iterative position moves, nm_run_md and nm_eval's forces: forcing the general form changes nothing, because these calls
    run it anyway (the production form would ignore the tape, leave the trace and the forces unwritten and draw bulk moves).  What each of them
    computes is pinned by the parity tests; here only the dispatch is."""
    monkeypatch.setenv('NM_CUS_PER_REPLICA', str(cus))
    state = _lattice(el)

    def both():
        e = _engine(el, state, **kw)
        assert e.cus_per_replica == cus
        e.set_step(3)
        out = run(e)
        e.close()
        return out

    _assert_same(*_both_forms(monkeypatch, both))
