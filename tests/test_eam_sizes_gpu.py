"""element Al (Sutton-Chen EAM) at 5^3 to 8^3 cells: the 16-bit-list EAM kernels (CfgMidSC, CfgMidSCQ4, CfgLargeSC, rows of the
configuration table NM_CFG_ROWS in nm_rows.hip) against the exact all-pairs reference and the oracle.

- nm_eval at every instantiation and workgroups-per-replica setting on the edge states of tests/exact_ref.py (status, pair counts,
  U and W to 1e-11, forces within the derived bound, the box below 2 rc refused);
- blocks of bulk, volume and HMC moves move by move against OracleLoop(el='Al'), two blocks with adapt between them;
- iterative position moves (the reference's default without -bm) at 500, 864 and 2048 atoms, both revert modes;
- nm_run_cycles and nm_run_cycles_recorded against single cycles, bit for bit;
- the perfect crystal: U/N and pressure do not depend on the number of cells;
- the driver at -e Al -ss 5."""
import functools
import os

import numpy as np
import pytest

import exact_ref as X
from helpers import OracleLoop, grids
from neuralmelting_amd import lattice

pytestmark = pytest.mark.gpu

AL_N = (257, 499, 500, 863, 864, 865, 1372, 2047, 2048)


def qs(n):
    """workgroups per replica with a row in the configuration table (nm_rows.hip NM_CFG_ROWS): the names are the Cfg typedefs"""
    if n <= 864:
        return {1: 'CfgMidSC', 2: 'CfgMidSC', 4: 'CfgMidSCQ4'}
    return {1: 'CfgLargeSC', 2: 'CfgLargeSC', 4: 'CfgLargeSC'}


CASES = [pytest.param(n, q, id='Al-%d-%s-q%d' % (n, cfg, q)) for n in AL_N for q, cfg in qs(n).items()]


@functools.lru_cache(maxsize=None)
def reference(n):
    L = X.box_for('Al', n, 0.055)
    out = []
    for name, x, LL in X.edge_states('Al', n, L, seed=3) + X.box_edge_states('Al', n, seed=3):
        U, W, f, npairs, _ = X.exact('Al', x, LL)
        out.append(dict(name=name, x=x, L=LL, U=float(U), W=float(W), f=f, npairs=npairs, b=X.force_bound('Al', x, LL)))
    return out


@pytest.mark.parametrize('n,q', CASES)
def test_eam_eval_edges(monkeypatch, n, q):
    import neuralmelting_amd as nm
    from neuralmelting_amd.engine import NMError
    monkeypatch.setenv('NM_CUS_PER_REPLICA', str(q))
    sts = reference(n)
    P, T = grids(1, len(sts), pr=(1.0, 8.0), tr=(300.0, 900.0))
    e = nm.Engine(n, P, T, element='Al')
    try:
        assert e.cus_per_replica == q, (qs(n)[q], e.cus_per_replica, e.note())
        d = np.tile([0.03125, 0.03125, 0.00390625], (len(sts), 1))
        e.set_state(np.stack([s['x'].reshape(-1) for s in sts]), np.zeros((len(sts), 3 * n)), [s['L'] for s in sts], d)
        e.stats(reset=True)
        U, W, f = e.eval()
        assert (e.status() == 0).all()
        st = e.stats()
        for k, s in enumerate(sts):
            tag = (qs(n)[q], q, s['name'], s['L'])
            assert st[k, 3] == s['npairs'], tag
            assert abs(U[k] - s['U']) <= 1e-11 * abs(s['U']), (tag, U[k], s['U'])
            assert abs(W[k] - s['W']) <= 1e-11 * abs(s['W']), (tag, W[k], s['W'])
            err = np.abs(f[k].reshape(-1, 3) - s['f'])
            assert np.all(err <= s['b']), (tag, float(err.max()))
        s = sts[0]
        e.set_state(s['x'].reshape(1, -1), None, [2 * X.SC_RC * (1 - 1e-9)], None, k0=0, nk=1)
        with pytest.raises(NMError, match=r'box edge < 2\*rc'):
            e.eval()
        e.set_state(s['x'].reshape(1, -1), None, [s['L']], None, k0=0, nk=1)
        U2, _, _ = e.eval(forces=False)
        assert U2[0] == U[0]
    finally:
        e.close()


def _engine(loop, n, P, T, **kw):
    import neuralmelting_amd as nm
    e = nm.Engine(n, P, T, element='Al', **kw)
    e.set_state(loop.x, loop.v, loop.box, loop.d)
    return e


# block parity: 5^3 and 6^3 at every Q, 8^3 at one and two workgroups per replica
BLOCK_CASES = [(5, 1), (5, 2), (5, 4), (6, 1), (6, 2), (6, 4), (8, 1), (8, 2)]


@pytest.mark.parametrize('sz,cus', BLOCK_CASES)
def test_eam_block_parity_large_cells(oracle, monkeypatch, sz, cus):
    """bulk, volume and HMC moves, move by move against the oracle, over two blocks with adapt between them (tolerances of
    tests/test_eam.py: branches, decisions and counters exact, criteria and energies 1e-6)"""
    monkeypatch.setenv('NM_CUS_PER_REPLICA', str(cus))
    mod = 6
    n = 4 * sz ** 3
    P, T = grids(1, 2, pr=(1.0, 8.0), tr=(300.0, 900.0))
    kw = dict(ppos=0.3, pvol=0.3)
    loop = OracleLoop(oracle, sz, P, T, el='Al', **kw)
    e = _engine(loop, n, P, T, **kw)
    assert e.cus_per_replica == cus
    e.set_trace(True)
    for step in range(2):
        e.set_step(step)
        e.run_block(mod)
        rows = e.thermo()
        tr = e.trace(mod)
        for k in range(loop.ns):
            s = oracle.Sim(n, units=1, mass=lattice.MASS['Al'], pot=1)
            s.set_rng(256, k, step)
            out = s.run_block(loop.x[k], loop.v[k], loop.box[k], loop.d[k], mod=mod, nstps=8, bulk=True, ppos=0.3, pvol=0.3,
                              lat=4.046, t=loop.tq[k], et=loop.et[k], pf=loop.pf[k], trace=True)
            np.testing.assert_array_equal(tr[k, :, :2], out['trace'][:, :2])
            np.testing.assert_allclose(tr[k, :, 2], out['trace'][:, 2], rtol=1e-6, atol=1e-6)
            np.testing.assert_allclose(rows[k, :5], out['thermo'], rtol=1e-6)
            np.testing.assert_array_equal(rows[k, 8:14], out['counters'])
            loop.x[k], loop.v[k], loop.box[k] = out['x'], out['v'], out['box']
            loop.d[k] = oracle.adapt(out['ratios'], loop.d[k])
        e.adapt()
    x, _, box, _ = e.get_state()
    np.testing.assert_allclose(box, loop.box, rtol=1e-12)
    np.testing.assert_allclose(x, loop.x, rtol=0, atol=1e-8)
    e.close()


# iterative position moves: (cells, workgroups per replica, revert modes).  500 atoms is below the workgroup's 512 threads (each thread owns at most
# one atom); 864 atoms (NJ = 2 atoms per thread) and 2048 (NJ = 4) are what Replica::delta_single_sc_strided's ownership of several atoms is for
ITER_CASES = [(5, 1, r) for r in (False, True)] + [(5, 4, False)] + [(6, q, r) for q in (1, 4) for r in (False, True)] + [(8, 1, False)]


@pytest.mark.parametrize('sz,cus,revert', ITER_CASES)
def test_eam_iterative_moves_parity(oracle, monkeypatch, sz, cus, revert):
    """iter_position_mc (the reference's default without -bm) at 5^3, 6^3 and 8^3: atom j on thread j mod 512, which keeps the density
    change of every atom it owns until the trial's decision (Replica::delta_single_sc_strided).  Every decision as the oracle's, which
    re-evaluates the whole system for every trial; reference mode (a rejected trial is not undone) and the corrected one"""
    monkeypatch.setenv('NM_CUS_PER_REPLICA', str(cus))
    n = 4 * sz ** 3
    mod = 2
    P, T = grids(1, 2, pr=(1.0, 8.0), tr=(300.0, 900.0))
    kw = dict(ppos=0.8, pvol=0.1, bulk=False, iter_revert=revert)
    loop = OracleLoop(oracle, sz, P, T, el='Al', **kw)
    e = _engine(loop, n, P, T, **kw)
    assert e.cus_per_replica == cus
    e.set_trace(True)
    e.run_block(mod)
    rows = e.thermo()
    tr = e.trace(mod)
    loop.run_block(mod, 0)
    ro = loop.rows()
    assert (tr[:, :, 0] == 3.0).sum() >= 2                             # iterative moves did take place
    assert (ro[:, 8] >= n).all()                                       # in every replica: n trials each
    np.testing.assert_array_equal(rows[:, 8:14], ro[:, 8:14])          # every one of the n decisions per move
    np.testing.assert_allclose(rows[:, :5], ro[:, :5], rtol=1e-6)
    x, _, _, _ = e.get_state()
    np.testing.assert_allclose(x, loop.x, rtol=0, atol=1e-8)
    e.close()


def test_eam_run_cycles_match_single_cycles():
    """at 5^3: nm_run_cycles (the loop of single launches here) and nm_run_cycles_recorded (the copy kernel behind each block) give the
    records and the state of the single path (block, snapshot, adapt, exchange per cycle), bit for bit"""
    import neuralmelting_amd as nm
    P, T = grids(2, 2, pr=(1.0, 8.0), tr=(300.0, 900.0))
    x, v, box, d = lattice.init_states(5, P, T, 0.03125, 0.03125, el='Al')
    mod, ncyc = 4, 3

    def fresh():
        e = nm.Engine(500, P, T, element='Al')
        e.set_state(x, v, box, d)
        e.set_step(0)
        return e

    a = fresh()
    single = []
    for s in range(ncyc):
        a.set_step(s)
        a.run_block(mod)
        a.snapshot()
        a.adapt()
        a.exchange(count=False)
        single.append(a.snapshot_fetch())
    sa = a.get_state()
    a.close()
    b = fresh()
    b.run_cycles(ncyc, mod)
    for u, w in zip(sa, b.get_state()):
        np.testing.assert_array_equal(u, w)
    b.close()
    r = fresh()
    r.run_cycles_recorded(ncyc, mod)
    for c in range(ncyc):
        rows, xr, br = r.snapshot_fetch()
        np.testing.assert_array_equal(rows, single[c][0])
        np.testing.assert_array_equal(xr, single[c][1])
        np.testing.assert_array_equal(br, single[c][2])
        assert xr.shape[1] == 1500
    for u, w in zip(sa, r.get_state()):
        np.testing.assert_array_equal(u, w)
    r.close()


def test_eam_perfect_crystal_is_size_independent():
    """rc < L / 2 at every size: each atom of a perfect crystal sees the same neighbours, so U/N and the pressure cannot depend on
    the number of cells (4^3: CfgSmallSC, 5^3: CfgMidSC, 8^3: CfgLargeSC)"""
    import neuralmelting_amd as nm
    a = lattice.lattice_constant('Al')
    out = []
    for sz in (4, 5, 8):
        n = 4 * sz ** 3
        P, T = grids(1, 1, pr=(1.0, 1.0), tr=(300.0, 300.0))
        x = (lattice.fcc_fractional(sz) * sz * a).reshape(1, -1)
        e = nm.Engine(n, P, T, element='Al')
        e.set_state(x, np.zeros_like(x), [sz * a], np.array([[0.03125, 0.03125, 0.00390625]]))
        U, W, f = e.eval()
        assert np.abs(f).max() < 1e-9
        out.append((U[0] / n, W[0] / (sz * a) ** 3))
        e.close()
    for u, w in out[1:]:
        assert abs(u - out[0][0]) <= 1e-10 * abs(out[0][0]), out
        assert abs(w - out[0][1]) <= 1e-10 * abs(out[0][1]), out


def test_driver_al_5_cells(tmp_path):
    """remcmc -e Al -ss 5 (the reference run.sh's cell size): a 2x2 grid for a few cycles writes 500-atom frames, and its restart dump
    reloads through -r"""
    from neuralmelting_amd import remcmc
    run = remcmc.Run('-bm -n al5 -e Al -ss 5 -pn 2 -tn 2 -pr 1 8 -tr 300 900 -sn 3 -sm 4 -sc 0 -rd 2'.split(), cwd=str(tmp_path))
    run.main()
    traj = [f for f in os.listdir(tmp_path) if f.startswith('al5') and f.endswith('.traj')]
    assert traj, os.listdir(tmp_path)
    first = open(tmp_path / traj[0]).readline().split()   # a frame opens with 'natoms box' (remcmc:248-256)
    assert int(first[0]) == 500, first
    run2 = remcmc.Run('-r -rn al5 -rs 2 -bm -n al5b -e Al -ss 5 -pn 2 -tn 2 -pr 1 8 -tr 300 900 -sn 2 -sm 4 -rd 2'.split(), cwd=str(tmp_path))
    run2.main()
    assert [f for f in os.listdir(tmp_path) if f.startswith('al5b') and f.endswith('.thrm')]
