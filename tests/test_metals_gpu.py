"""Elements Cu and Ni on the n = 9 Sutton-Chen kernels (the Cfg POT 2 twins of Al's configurations, nm_rows.hip), without an oracle:

- nm_eval at every instantiation and workgroups-per-replica setting against the exact all-pairs reference (tests/metals_ref.py) on
  Al's edge states scaled to the element (status, pair counts, U and W to 1e-11, forces within the derived bound, the box below 2 rc
  refused);
- the Cu-Ni scaling identity: equal n, m, c and reduced cutoff make a Ni state that is a Cu state scaled by a_Ni / a_Cu give
  eps_Ni / eps_Cu times U and W;
- iterative position moves (corrected mode): the criterion of the last trial times kT is the exact energy difference it decided on;
- the same chain however the work is launched (fused cycles against single launches; Q = 1, 2, 4);
- metal-unit physics: dH of HMC second order in dt, the perfect crystal size-independent and force-free, the NPT pressure in bar;
- the driver, parse and distr end to end at -e Cu, and -e Ni once."""
import functools
import os

import numpy as np
import pytest

import metals_ref as M
from helpers import grids
from neuralmelting_amd import lattice

pytestmark = pytest.mark.gpu

NS = (2, 100, 255, 256, 257, 500, 864, 865, 2048)
BOLTZ = 8.617343e-5          # LAMMPS update.cpp, units metal
NKTV2P = 1.6021765e6


def qs(n):
    """workgroups per replica with an n = 9 row in the configuration table (nm_rows.hip NM_CFG_ROWS): the names are the Cfg typedefs"""
    if n <= 256:
        return {1: 'CfgSmallSC9', 2: 'CfgSmallSC9Q2', 4: 'CfgSmallSC9Q4'}
    if n <= 864:
        return {1: 'CfgMidSC9', 2: 'CfgMidSC9', 4: 'CfgMidSC9Q4'}
    return {1: 'CfgLargeSC9', 2: 'CfgLargeSC9', 4: 'CfgLargeSC9'}


CASES = [pytest.param(el, n, q, id='%s-%d-%s-q%d' % (el, n, cfg, q)) for el in M.ELS for n in NS for q, cfg in qs(n).items()]


@functools.lru_cache(maxsize=None)
def reference(el, n):
    out = []
    for name, x, L in M.edge_states(el, n, seed=3):
        U, W, f, npairs = M.exact(el, x, L)
        out.append(dict(name=name, x=x, L=L, U=float(U), W=float(W), f=f, npairs=npairs, b=M.force_bound(el, x, L)))
    return out


def _d(ns):
    return np.tile([0.03125, 0.03125, 0.00390625], (ns, 1))


@pytest.mark.parametrize('el,n,q', CASES)
def test_metal_eval_edges(monkeypatch, el, n, q):
    import neuralmelting_amd as nm
    from neuralmelting_amd.engine import NMError
    monkeypatch.setenv('NM_CUS_PER_REPLICA', str(q))
    sts = reference(el, n)
    assert {'fluid', 'gas'} <= {s['name'] for s in sts}
    P, T = grids(1, len(sts), pr=(1.0, 8.0), tr=(300.0, 900.0))
    e = nm.Engine(n, P, T, element=el)
    try:
        assert e.cus_per_replica == q, (qs(n)[q], e.cus_per_replica, e.note())
        e.set_state(np.stack([s['x'].reshape(-1) for s in sts]), np.zeros((len(sts), 3 * n)), [s['L'] for s in sts], _d(len(sts)))
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
        e.set_state(s['x'].reshape(1, -1), None, [2 * M.rc(el) * (1 - 1e-9)], None, k0=0, nk=1)
        with pytest.raises(NMError, match=r'box edge < 2\*rc'):
            e.eval()
        e.set_state(s['x'].reshape(1, -1), None, [s['L']], None, k0=0, nk=1)
        U2, _, _ = e.eval(forces=False)
        assert U2[0] == U[0]
    finally:
        e.close()


@pytest.mark.parametrize('sz', [4, 8])
def test_cu_ni_scaling_identity(sz):
    """U_Ni = k U_Cu, W_Ni = k W_Cu, f_Ni = k f_Cu / s with k = eps_Ni / eps_Cu, s = a_Ni / a_Cu, on displaced crystals and a
    compressed and an expanded one"""
    import neuralmelting_amd as nm
    n = 4 * sz ** 3
    P, T = grids(2, 4, pr=(1.0, 4e4), tr=(300.0, 1500.0))
    x, v, box, d = lattice.init_states(sz, P, T, 0.06, 0.03125, el='Cu')
    s = lattice.SC['Ni'][1] / lattice.SC['Cu'][1]
    k = lattice.SC['Ni'][0] / lattice.SC['Cu'][0]
    out = {}
    for el, xx, bb in (('Cu', x, box), ('Ni', x * s, box * s)):
        e = nm.Engine(n, P, T, element=el)
        try:
            e.set_state(xx, np.zeros_like(xx), bb, d)
            out[el] = e.eval()
            assert (e.status() == 0).all()
        finally:
            e.close()
    (uc, wc, fc), (un, wn, fn) = out['Cu'], out['Ni']
    np.testing.assert_allclose(un, k * uc, rtol=1e-12, atol=0)
    np.testing.assert_allclose(wn, k * wc, rtol=1e-12, atol=0)
    fr = np.abs(fn - k * fc / s).max(1) / np.abs(fn).max(1)
    print('Cu-Ni identity %d atoms: U %.2e W %.2e f %.2e (relative)' % (n, np.abs(un / (k * uc) - 1).max(), np.abs(wn / (k * wc) - 1).max(), fr.max()))
    assert (fr < 1e-12).all(), fr


@pytest.mark.parametrize('el,sz,q', [('Cu', 4, 1), ('Cu', 4, 4), ('Ni', 5, 1), ('Cu', 6, 2), ('Ni', 8, 4), ('Cu', 8, 1)])
def test_iterative_move_criterion_is_the_exact_energy_difference(monkeypatch, el, sz, q):
    """one iterative position move per block (ppos = 1, corrected mode): where the move's last trial (atom N-1) was accepted, its criterion
    de (trace column 2, PH_ITER_END) times kT is U(final) - U(final with atom N-1 back at its move-start position), exactly.  That pins
    delta_single_sc / delta_single_sc_strided with the n = 9 term and the density bookkeeping through the N-1 trials before it
    (256 atoms: one thread per atom; 500 and more: the strided path)."""
    import neuralmelting_amd as nm
    monkeypatch.setenv('NM_CUS_PER_REPLICA', str(q))
    n = 4 * sz ** 3
    P, T = grids(2, 4, pr=(1.0, 8.0), tr=(600.0, 1500.0))
    x, v, box, d = lattice.init_states(sz, P, T, 0.03125, 0.03125, el=el)
    e = nm.Engine(n, P, T, element=el, bulk=False, ppos=1.0, pvol=0.0, iter_revert=True)
    try:
        assert e.cus_per_replica == q
        e.set_state(x, v, box, d)
        et, _ = e.constants()
        e.set_trace(True)
        e.run_block(1)
        tr = e.trace(1)
        xf, _, bf, _ = e.get_state(velocities=False)
        assert (e.status() == 0).all()
    finally:
        e.close()
    assert (tr[:, 0, 0] == 3.0).all()
    checked = 0
    for k in range(len(x)):
        L = bf[k]
        a = xf[k].reshape(-1, 3)
        d0 = a[-1] - x[k].reshape(-1, 3)[-1]
        d0 -= L * np.rint(d0 / L)
        if np.abs(d0).max() < 1e-12:
            continue                                            # rejected: the atom is back where it started
        b = a.copy()
        b[-1] = x[k].reshape(-1, 3)[-1]
        u1, u0 = M.energy(el, a, L), M.energy(el, b, L)
        du = float(u1 - u0)
        assert abs(du - tr[k, 0, 2] * et[k]) <= 1e-12 * abs(float(u1)) + 1e-12, (k, du, tr[k, 0, 2] * et[k])
        assert abs(tr[k, 0, 3] - float(u1)) <= 1e-11 * abs(float(u1))   # and the closing evaluation's U
        checked += 1
    print('%s-%d q%d: %d of %d slots with the last trial accepted' % (el, n, q, checked, len(x)))
    assert checked >= 2


@pytest.mark.parametrize('q', [2, 4])
def test_fused_cycles_equal_single_cycles(monkeypatch, q):
    """at 4^3 (the fused nm_cycles_kernel at Q = 2 and 4): nm_run_cycles and nm_run_cycles_recorded give the state, thermo and
    counters of the single path (block, snapshot, adapt, exchange per cycle), bit for bit"""
    import neuralmelting_amd as nm
    monkeypatch.setenv('NM_CUS_PER_REPLICA', str(q))
    P, T = grids(2, 4, pr=(1.0, 8.0), tr=(300.0, 1500.0))
    x, v, box, d = lattice.init_states(4, P, T, 0.03125, 0.03125, el='Cu')
    mod, ncyc = 4, 3

    def fresh():
        e = nm.Engine(256, P, T, element='Cu')
        assert e.cus_per_replica == q
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
    for u, w in zip(sa, r.get_state()):
        np.testing.assert_array_equal(u, w)
    r.close()


@pytest.mark.parametrize('el,sz', [('Cu', 4), ('Ni', 5)])
def test_same_chain_at_every_q(monkeypatch, el, sz):
    """a block of the production move mix at Q = 1, 2 and 4: identical counters, energies within 1e-9 (the sums' order differs)"""
    import neuralmelting_amd as nm
    n = 4 * sz ** 3
    P, T = grids(2, 4, pr=(1.0, 8.0), tr=(300.0, 1500.0))
    x, v, box, d = lattice.init_states(sz, P, T, 0.03125, 0.03125, el=el)
    rows = []
    for q in (1, 2, 4):
        monkeypatch.setenv('NM_CUS_PER_REPLICA', str(q))
        e = nm.Engine(n, P, T, element=el)
        try:
            assert e.cus_per_replica == q
            e.set_state(x, v, box, d)
            e.run_block(8)
            rows.append(e.thermo())
            assert (e.status() == 0).all()
        finally:
            e.close()
    for r in rows[1:]:
        np.testing.assert_array_equal(r[:, 8:14], rows[0][:, 8:14])
        np.testing.assert_allclose(r[:, 1], rows[0][:, 1], rtol=1e-9)
        np.testing.assert_allclose(r[:, 4], rows[0][:, 4], rtol=1e-9)


@pytest.mark.parametrize('el', M.ELS)
def test_hmc_energy_error_is_second_order_in_dt(el):
    """tests/test_physics_metal_gpu.py's construction for the element: over a trajectory of fixed length (4 x 0.004, 8 x 0.002,
    16 x 0.001 ps) dH falls 4x per halving of dt.  Cold crystals with the lattice put so that rc lies midway between the 6th and 7th
    fcc shells (no pair crosses the unshifted cutoff)."""
    import neuralmelting_amd as nm
    sz = 4
    n = 4 * sz ** 3
    P = np.linspace(1.0, 8.0, 8, dtype=np.float32)
    T = np.linspace(10.0, 50.0, 8, dtype=np.float32)
    a = M.rc(el) / (0.5 * (np.sqrt(3.0) + np.sqrt(3.5)))
    box = np.full(64, sz * a)
    rng = np.random.default_rng(17)
    x = (lattice.fcc_fractional(sz)[None] * box[0] + 0.04 * M.scale(el) * (rng.random((64, n, 3)) - 0.5)).reshape(64, -1)
    v = np.zeros_like(x)
    d = np.tile([0.004, 0.004, 0.00390625], (64, 1))
    dh = []
    for nstps, dt in ((4, 0.004), (8, 0.002), (16, 0.001)):
        e = nm.Engine(n, P, T, element=el, ppos=0.0, pvol=0.0, nstps=nstps)
        try:
            dd = d.copy(); dd[:, 2] = dt
            e.set_state(x, v, box, dd)
            e.set_trace(True)
            e.run_block(1)
            tr = e.trace(1)
        finally:
            e.close()
        assert (tr[:, 0, 0] == 2.0).all()
        dh.append(tr[:, 0, 2])
    dh = np.array(dh)
    r1, r2 = dh[0] / dh[1], dh[1] / dh[2]
    print('HMC dt ratios %s-%d: median %.4f %.4f, |dH| at 0.001 ps: %.3g ... %.3g'
          % (el, n, np.median(r1), np.median(r2), np.abs(dh[2]).min(), np.abs(dh[2]).max()))
    assert (np.abs(dh[2]) > 1e-9).all()
    assert 3.8 < np.median(r1) < 4.2 and 3.9 < np.median(r2) < 4.1, (np.median(r1), np.median(r2))
    assert np.mean((r2 > 3.5) & (r2 < 4.5)) > 0.9, np.sort(r2)


@pytest.mark.parametrize('el', M.ELS)
def test_perfect_crystal_is_size_independent(el):
    """4^3 (CfgSmallSC9), 5^3 (CfgMidSC9), 8^3 (CfgLargeSC9): U/N and the pressure of the perfect crystal do not depend on the cells,
    the forces vanish, and U/N is the truncated lattice sum of tests/test_metals_cpu.py"""
    import neuralmelting_amd as nm
    a = lattice.lattice_constant(el)
    out = []
    for sz in (4, 5, 8):
        n = 4 * sz ** 3
        P, T = grids(1, 1, pr=(1.0, 1.0), tr=(300.0, 300.0))
        x = (lattice.fcc_fractional(sz) * sz * a).reshape(1, -1)
        e = nm.Engine(n, P, T, element=el)
        try:
            e.set_state(x, np.zeros_like(x), [sz * a], np.array([[0.03125, 0.03125, 0.00390625]]))
            U, W, f = e.eval()
        finally:
            e.close()
        assert np.abs(f).max() < 1e-9
        out.append((U[0] / n, W[0] / (sz * a) ** 3))
    for u, w in out[1:]:
        assert abs(u - out[0][0]) <= 1e-10 * abs(out[0][0]), out
        assert abs(w - out[0][1]) <= 1e-10 * abs(out[0][1]), out
    u4, _ = lattice.sc_static(lattice.fcc_fractional(4), 4 * a, el)
    assert abs(out[0][0] - u4 / 256) <= 1e-11 * abs(u4 / 256)


def test_npt_pressure_in_bar_equals_imposed_pressure_cu():
    """tests/test_physics_metal_gpu.py::test_npt_pressure_in_bar_equals_imposed_pressure_al for Cu: 5 to 40 kbar, 300 to 900 K, the
    estimator N kT / V - dU/dV with the impulsive term of the unshifted cutoff (central difference of nm_eval on the scaled copies
    minus W / 3V) must have the slot's imposed pressure as its mean at all 64 state points"""
    import neuralmelting_amd as nm
    n, eps = 256, 2e-3
    P = np.linspace(5e3, 4e4, 8, dtype=np.float32)
    T = np.linspace(300.0, 900.0, 8, dtype=np.float32)
    x, v, box, d = lattice.init_states(4, P, T, 0.01, 0.004, el='Cu')
    d[:, 0] = 0.004
    e = nm.Engine(n, P, T, element='Cu')
    ev = nm.Engine(n, P, T, element='Cu')
    mod, burn, cycles = 64, 24, 96
    samples, imp, wdiff = [], [], []
    try:
        e.set_state(x, v, box, d)
        for step in range(burn + cycles):
            e.set_step(step)
            e.run_block(mod)
            if step >= burn:
                r = e.thermo()
                samples.append(r)
                xs, _, bs, _ = e.get_state(velocities=False)
                ev.set_state(xs, None, bs, None)
                _, W0, _ = ev.eval(forces=False)
                U = []
                for s in (1.0 + eps, 1.0 - eps):
                    f = np.cbrt(s)
                    ev.set_state(xs * f, None, bs * f, None)
                    U.append(ev.eval(forces=False)[0])
                    assert (ev.status() == 0).all()
                vol = bs ** 3
                imp.append((-(U[0] - U[1]) / (2.0 * eps * vol) - W0 / (3.0 * vol)) * NKTV2P)
                kin = (n - 1.0) * BOLTZ * r[:, 0]
                wdiff.append(np.abs(r[:, 3] - (kin + W0 / 3.0) / vol * NKTV2P) / ((kin + np.abs(W0) / 3.0) / vol * NKTV2P))
            e.adapt()
            e.exchange(count=False)
        assert (e.status() == 0).all()
    finally:
        e.close()
        ev.close()
    assert np.max(wdiff) < 1e-9, np.max(wdiff)
    r = np.array(samples)
    imp = np.array(imp)
    tkin, press, vol = r[:, :, 0], r[:, :, 3], r[:, :, 4]
    Tj = np.tile([float('%f' % t) for t in T], 8)[None, :]
    Pi = np.repeat(P.astype(np.float64), 8)
    pest = press + (n * BOLTZ * Tj - (n - 1.0) * BOLTZ * tkin) / vol * NKTV2P + imp
    nb = 8
    bm = pest.reshape(nb, cycles // nb, 64).mean(1)
    se = bm.std(0, ddof=1) / np.sqrt(nb)
    se = np.maximum(se, np.median(se))
    diff = bm.mean(0) - Pi
    z = diff / se
    print('NPT Cu: |z| max %.2f, mean z %.3f, mean diff %.1f bar, median se %.1f bar, mean impulsive term %.1f bar'
          % (np.abs(z).max(), z.mean(), diff.mean(), np.median(se), imp.mean()))
    assert (np.abs(z) < 5.0).all(), np.sort(np.abs(z))[-4:]
    assert abs(z.mean()) < 0.5, z.mean()
    assert abs(diff.mean()) < 4.0 * np.median(se) / 8.0, diff.mean()


def _run(argv, cwd):
    from neuralmelting_amd import remcmc
    run = remcmc.Run(argv, cwd=str(cwd))
    run.main()
    return run


def test_driver_parse_distr_cu(tmp_path, monkeypatch):
    """remcmc -e Cu -ss 4 -pn 2 -tn 2 with recorded cycles and a restart dump, its restart, then parse -e Cu and distr -e Cu: the
    files carry the .cu.fcc. prefix, every value is finite, the volume per atom is near a^3 / 4"""
    from neuralmelting_amd import distr, parse
    monkeypatch.chdir(tmp_path)
    run = _run('-bm -n cu1 -e Cu -ss 4 -pn 2 -tn 2 -pr 1 8 -tr 300 900 -sn 3 -sm 8 -rd 2'.split(), tmp_path)
    assert run.PREF == str(tmp_path) + '/cu1.cu.fcc.lammps'
    assert os.path.exists(run.PREF + '.thrm') and os.path.exists(run.PREF + '.traj')
    parse.main(['-n', 'cu1', '-e', 'Cu'])
    distr.main(['-n', 'cu1', '-e', 'Cu', '-sb', '32', '-cb', '8'])
    a = lattice.SC['Cu'][1]
    pe, vol = np.load(run.PREF + '.pe.npy'), np.load(run.PREF + '.vol.npy')
    assert pe.shape == (2, 2, 3) and np.isfinite(pe).all() and (pe < -3.0 * 256).all() and (pe > -4.0 * 256).all()   # ~ -3.4 eV/atom
    assert np.isfinite(vol).all() and (np.abs(vol / 256 / (a ** 3 / 4) - 1) < 0.05).all(), vol / 256
    pos = np.load(run.PREF + '.pos.npy')
    assert pos.shape == (2, 2, 3, 256, 3) and np.isfinite(pos).all()
    rdf = np.load(run.PREF + '.rdf.npy')
    assert rdf.shape == (2, 2, 3, 32) and np.isfinite(rdf).all()
    assert np.isfinite(np.load(run.PREF + '.cdf.npy')).all()
    run2 = _run('-r -rn cu1 -rs 2 -bm -n cu2 -e Cu -ss 4 -pn 2 -tn 2 -pr 1 8 -tr 300 900 -sn 2 -sm 8'.split(), tmp_path)
    t = np.loadtxt(run2.PREF + '.thrm')
    assert run2.PREF.endswith('/cu2.cu.fcc.lammps') and t.ndim == 2 and t.shape[1] == 17 and np.isfinite(t).all()


def test_driver_ni_5_cells(tmp_path):
    run = _run('-bm -n ni5 -e Ni -ss 5 -pn 2 -tn 2 -pr 1 8 -tr 300 900 -sn 2 -sm 4'.split(), tmp_path)
    t = np.loadtxt(run.PREF + '.thrm')
    assert run.PREF.endswith('/ni5.ni.fcc.lammps') and t.ndim == 2 and t.shape[1] == 17 and np.isfinite(t).all()
    assert (t[:, 1] < -4.0 * 500).all() and (np.abs(t[:, 4] / 500 / (lattice.SC['Ni'][1] ** 3 / 4) - 1) < 0.05).all()
    first = open(run.PREF + '.traj').readline().split()
    assert int(first[0]) == 500
