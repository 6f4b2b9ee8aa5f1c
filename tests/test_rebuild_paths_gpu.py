"""The rebuild of the LDS Verlet lists (nm_kernels.h Replica::rebuild, its LIST_LDS branch) writes list bytes, row lengths and reference
positions that no result shows directly, but every later pair sum is taken in the order of a row, the validity check runs against the
reference positions, and a rejected trajectory that rebuilt returns to the saved list: whatever the rebuild writes differently shows in the
bits of the chain.  So the bar for a change to it is the chain itself: tests/golden/rebuild_parent.npz holds, for every path the rebuild
takes, the bytes of x, v, box, the step sizes, the thermo rows and the rebuild counts after three blocks of 16 moves (run_block twice, then
one fused cycle), as the commit BEFORE the rebuild was reworked computed them, and the test asserts byte equality.

The starts are lattice states.  Every launch builds its lists first (an LDS list does not outlive its launch), so one rebuild per block and
replica says nothing; the cases marked * rebuild during their moves as well, and the test asserts that they do:
  lj-q1 .. lj-q8    256 atoms at 1, 2, 4, 8 workgroups per replica at the reference's time step: 2 to 16 threads per row, one and several
                    rounds of 32 candidates per thread, rows of the own atoms only and of all atoms; the launch's own rebuild only
  n108-*, n32-* *   108 and 32 atoms (3^3 and 2^3 cells of the 4^3 lattice in its box) at 1 and 2 workgroups: the general form, atom counts
                    that are no multiple of 32 x the threads per row, groups without a row
  al-q4 *           the Sutton-Chen rows (256-entry rows)
  dense-q4          P = 8 at T = 0.1 and 0.25: every row is longer than 64 entries, i.e. spans two 64-entry chunks (stats column 8)
  rejected-q* *     the same four at twice the time step: trajectories that rebuilt are rejected (in some block a slot rebuilds more
                    often than the once its launch begins with, and accepts no trajectory), so the saved list, its row lengths and
                    reference positions come back
Recording is not part of the suite: `python tests/test_rebuild_paths_gpu.py OUT.npz` writes the fixture from the library in use."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MOD = 16
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'rebuild_parent.npz')
LJ_T, AL_T = (0.25, 2.5), (256.0, 2560.0)
# name: (atoms, element, workgroups per replica, pressures, temperatures, factor on the lattice state's time step)
CASES = {
    'lj-q1': (256, 'LJ', 1, (1.0, 8.0), LJ_T, 1.0),
    'lj-q2': (256, 'LJ', 2, (1.0, 8.0), LJ_T, 1.0),
    'lj-q4': (256, 'LJ', 4, (1.0, 8.0), LJ_T, 1.0),
    'lj-q8': (256, 'LJ', 8, (1.0, 8.0), LJ_T, 1.0),
    'n108-q1': (108, 'LJ', 1, (1.0, 8.0), LJ_T, 1.0),
    'n108-q2': (108, 'LJ', 2, (1.0, 8.0), LJ_T, 1.0),
    'n32-q1': (32, 'LJ', 1, (1.0, 8.0), LJ_T, 1.0),
    'n32-q2': (32, 'LJ', 2, (1.0, 8.0), LJ_T, 1.0),
    'al-q4': (256, 'Al', 4, (1.0, 8.0), AL_T, 1.0),
    'dense-q4': (256, 'LJ', 4, (8.0, 8.0), (0.1, 0.25), 1.0),
    'rejected-q1': (256, 'LJ', 1, (1.0, 8.0), LJ_T, 2.0),
    'rejected-q2': (256, 'LJ', 2, (1.0, 8.0), LJ_T, 2.0),
    'rejected-q4': (256, 'LJ', 4, (1.0, 8.0), LJ_T, 2.0),
    'rejected-q8': (256, 'LJ', 8, (1.0, 8.0), LJ_T, 2.0),
}
MOVING = ('n108', 'n32', 'al', 'rejected')   # cases whose moves rebuild
KEYS = ('x', 'v', 'box', 'd', 'thermo', 'rebuilds')


def _grid(pr, tr):
    return np.linspace(pr[0], pr[1], 1, dtype=np.float32), np.linspace(tr[0], tr[1], 2, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def _start(natoms, el, pr, tr, mult):
    """the 4^3 lattice state of the grid (1 pressure x 2 temperatures), cut down to the 3^3 or 2^3 cells at the origin for 108 and 32 atoms
    (in the 4^3 box: the box of fewer cells is below twice the cutoff), the time step times mult"""
    from neuralmelting_amd import lattice
    x, v, box, d = lattice.init_states(4, *_grid(pr, tr), 0.03125, 0.03125, el=el)
    if natoms != 256:
        ncell = {108: 3, 32: 2}[natoms]
        site = np.rint(8.0 * x[0].reshape(-1, 3) / box[0]).astype(int) % 8   # half-cell index of the (slightly displaced, wrapped) lattice site
        keep = np.flatnonzero((site < 2 * ncell).all(axis=1))
        assert len(keep) == natoms
        x = np.stack([xs.reshape(-1, 3)[keep].reshape(-1) for xs in x])
        v = np.zeros_like(x)
    d = d.copy()
    d[:, 2] *= mult
    state = (x, v, box, d)
    for a in state:
        a.setflags(write=False)
    return state


def _run(name, mult=None):
    """three blocks of 16 moves: run_block twice, then one fused cycle (the block kernel and the cycles kernel each hold a rebuild; a fused
    cycle zeroes the thermo row's counters behind it, so the first two blocks are the ones whose trials and acceptances show)"""
    import neuralmelting_amd as nm
    natoms, el, cus, pr, tr, m = CASES[name]
    os.environ['NM_CUS_PER_REPLICA'] = str(cus)
    os.environ['NM_FUSED_CYCLES'] = 'all'
    e = nm.Engine(natoms, *_grid(pr, tr), element=el)
    try:
        assert e.cus_per_replica == cus
        e.set_state(*_start(natoms, el, pr, tr, m if mult is None else mult))
        thermo, stats = [], []

        def keep():
            e.synchronize()
            assert (e.status() == 0).all(), e.status()
            thermo.append(e.thermo())
            stats.append(e.stats())
        for s in (0, 1):
            e.set_step(s)
            e.run_block(MOD)
            keep()
            e.adapt()
            e.exchange(count=False)
        e.set_step(2)
        e.run_cycles(1, MOD)
        keep()
        x, v, box, d = e.get_state()
        assert e.note() == '' and e.heals == 0
    finally:
        e.close()
    stats = np.array(stats)
    return dict(x=x, v=v, box=box, d=d, thermo=np.array(thermo), rebuilds=stats[:, :, 1].copy(), longest=stats[:, :, 8].copy())


@pytest.fixture
def _environment(monkeypatch):
    """(_run sets the two switches through os.environ: monkeypatch puts them back)"""
    monkeypatch.setenv('NM_CUS_PER_REPLICA', '0')
    monkeypatch.setenv('NM_FUSED_CYCLES', 'all')
    monkeypatch.delenv('NM_PLAIN_KERNELS', raising=False)


@functools.lru_cache(maxsize=None)
def _golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize('name', list(CASES))
def test_chain_bytes_are_the_parents(_environment, name):
    got, want = _run(name), _golden()
    reb = want[name + '.rebuilds']
    # rebuilds of each block, summed over the replicas (the counter runs on from block to block; a fused cycle zeroes nothing of it)
    per_block = np.diff(np.concatenate([np.zeros((1,) + reb.shape[1:]), reb]), axis=0).sum(axis=1)
    if name.startswith(MOVING):   # not only the one rebuild per replica that every launch begins with
        assert (per_block > reb.shape[1]).all(), reb
    for key in KEYS:
        w = want['%s.%s' % (name, key)]
        assert got[key].dtype == w.dtype and got[key].shape == w.shape, key
        assert got[key].tobytes() == w.tobytes(), '%s of %s differs in %d elements' % (key, name, (got[key] != w).sum())
    if name == 'dense-q4':
        assert got['longest'].min() > 64, got['longest']           # two 64-entry chunks in every slot's longest row
    if name.startswith('rejected'):
        th = got['thermo']                                         # .thrm columns 12, 13: HMC trials and acceptances of the block
        rebuilt = np.diff(np.concatenate([np.zeros((1,) + reb.shape[1:]), reb]), axis=0) > 1
        refused_all = (th[:, :, 12] > 0) & (th[:, :, 13] == 0)
        assert (rebuilt & refused_all).any(), (th[:, :, 12], th[:, :, 13], reb)


if __name__ == '__main__':   # record the fixture (and, with factors given, show what other time steps would do)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    os.environ.setdefault('NM_TESTING', '1')   # (as conftest.py sets it for the suite)
    out, factors = sys.argv[1], [float(a) for a in sys.argv[2:]]
    rec = {}
    for name in CASES:
        for mult in [None] + factors:
            try:
                r = _run(name, mult)
            except Exception as ex:                                # a status word or a note: said and left out; any other error ends the recording
                if not isinstance(ex, AssertionError) and 'left the supported regime' not in str(ex):
                    raise
                print('%-12s x%-4s FAILED: %r' % (name, mult, ex), flush=True)
                continue
            print('%-12s x%-4s rebuilds %s longest %s trials %s accepted %s' % (name, mult or CASES[name][5], r['rebuilds'].tolist(), r['longest'][-1].tolist(),
                                                                             r['thermo'][:, :, 12].tolist(), r['thermo'][:, :, 13].tolist()), flush=True)
            for key in KEYS:
                rec['%s.%s' % (name, key) if mult is None else '%s@%g.%s' % (name, mult, key)] = r[key]
    np.savez_compressed(out, **rec)
