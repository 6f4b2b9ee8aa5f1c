"""Oracle-free pins of the metal-unit arithmetic of element Al (LAMMPS `units metal`), measured on the HIP path through the C-ABI.

In lj units kB, mvv2e, ftm2v and nktv2p all equal 1, so the tests of test_physics_gpu.py cannot tell a swapped, inverted or
misplaced conversion factor, or a mass applied in the wrong place.  The oracle takes the same four literals as nm_create, so one
consistent mistake in both passes every parity test.  The constants below are LAMMPS's (update.cpp, `units metal`), written here
and not imported from the package:
  velocity create / zero linear / zero angular, thermo temp, ke, press in bar (boltz, mvv2e, nktv2p, mass)
      test_velocity_create_semantics_metal (N = 256, 500, 2048; 2048 keeps the image flags in the global spill) and the LJ
      counterpart at N = 2048
  fix nve half-kick 0.5 dt ftm2v / m, the mass of the draw = the mass of the kick
      test_hmc_energy_error_is_second_order_in_dt_al
  the reference's pf (bar through 1e-30 1e5 / 1.60218e-19), thermo_press's nktv2p and the eV energies of the volume criterion
      test_npt_pressure_in_bar_equals_imposed_pressure_al
"""
import numpy as np
import pytest

import exact_ref as X
from neuralmelting_amd import lattice
from test_physics_gpu import lammps_velocity_create

pytestmark = pytest.mark.gpu

# LAMMPS update.cpp, units metal
BOLTZ = 8.617343e-5          # eV / K
MVV2E = 1.0364269e-4         # (g/mol) (A/ps)^2 -> eV
FTM2V = 1.0 / 1.0364269e-4   # (eV/A) / (g/mol) -> A/ps^2 (pinned by the dt^2 test)
NKTV2P = 1.6021765e6         # eV/A^3 -> bar
MASS_AL = 29.982             # remcmc:886
UNITS = {'Al': dict(mass=MASS_AL, kB=BOLTZ, mvv2e=MVV2E, nktv2p=NKTV2P), 'LJ': dict(mass=1.0, kB=1.0, mvv2e=1.0, nktv2p=1.0)}


@pytest.mark.parametrize('el,sz', [('Al', 4), ('Al', 5), ('Al', 8), ('LJ', 8)],
                         ids=['Al-256', 'Al-500', 'Al-2048', 'LJ-2048'])
def test_velocity_create_semantics_metal(el, sz):
    """test_physics_gpu.py::test_velocity_create_semantics_with_image_flags in metal units, and at N = 2048 (for LJ too), where
    velocity_create keeps the image flags in the per-workgroup global spill (the !SAVE_LDS branch).  One bulk position move
    (accepted: tape uniform 0) carries atoms across the box faces; the HMC move that follows draws velocities and integrates with
    timestep 0.  The returned velocities must (i) carry no linear momentum, (ii) no angular momentum about the centre of mass of the
    unwrapped coordinates, (iii) equal LAMMPS's documented sequence restated in numpy with mass 29.982 and the metal kB, mvv2e,
    (iv) sit just below T; the temp, ke and virial columns must be what thermo_temp, thermo_ke and thermo_press (in bar) make of
    the returned x, v with the constants above and W of the exact all-pairs reference."""
    import neuralmelting_amd as nm
    c = UNITS[el]
    m, kB, mvv2e, nktv2p = c['mass'], c['kB'], c['mvv2e'], c['nktv2p']
    n = 4 * sz ** 3
    P = np.linspace(1.0, 8.0, 2, dtype=np.float32)
    T = np.linspace(300.0, 900.0, 2, dtype=np.float32) if el == 'Al' else np.linspace(0.5, 2.0, 2, dtype=np.float32)
    x, v, box, d = lattice.init_states(sz, P, T, 0.03125, 0.03125, el=el)
    box = np.round(box, 6)                                      # init_lammps hands the box over as '%f' (remcmc:466)
    x = np.mod(x.reshape(4, n, 3), box[:, None, None]).reshape(4, -1)
    d[:, 2] = 0.0                                               # timestep 0.000000
    tag_a, tag_b = 12345, 54321
    tape = [0.0, tag_a / 65536.0, 0.0, 0.99, tag_b / 65536.0, 0.5]   # roll, randint, accept | roll, randint, accept
    e = nm.Engine(n, P, T, element=el, seed=77)
    try:
        e.set_state(x, v, box, d)
        e.set_rng_tape([tape] * 4)
        e.set_trace(True)
        e.set_step(9)
        e.run_block(2)
        tr = e.trace(2)
        rows = e.thermo()
        xo, vo, bo, _ = e.get_state()
    finally:
        e.close()
    np.testing.assert_array_equal(tr[:, :, 0], [[0.0, 2.0]] * 4)   # bulk PMC, then HMC
    np.testing.assert_array_equal(tr[:, :, 1], 1.0)                 # both accepted
    np.testing.assert_array_equal(bo, box)
    crossed = 0
    for k in range(4):
        L = box[k]
        t = float('%f' % T[k % 2])
        xi, xw, vv = x[k].reshape(n, 3), xo[k].reshape(n, 3), vo[k].reshape(n, 3)
        dxy = xw - xi
        dxy -= L * np.rint(dxy / L)
        xu = xi + dxy                                           # unwrapped = wrapped + image * L
        crossed += int((np.abs(xu - xw) > 0.5 * L).any(1).sum())
        vscale = np.sqrt(kB * t / (m * mvv2e))                  # A/ps in metal units: 2.9 at 300 K
        assert np.abs(vv.sum(0)).max() < 1e-13 * np.abs(vv).sum()                      # (i)
        xc = xu - xu.mean(0)
        lscale = m * (np.linalg.norm(xc, axis=1) * np.linalg.norm(vv, axis=1)).sum()
        Lu = m * np.cross(xc, vv).sum(0)
        Lw = m * np.cross(xw - xw.mean(0), vv).sum(0)
        assert np.abs(Lu).max() < 1e-12 * lscale, (Lu, lscale)                           # (ii)
        assert np.abs(Lw).max() > 1e-6 * lscale, (Lw, lscale)
        ref = lammps_velocity_create(xu, t, 77, k, tag_b, 9, mass=m, kB=kB, mvv2e=mvv2e)
        np.testing.assert_allclose(vv, ref, rtol=0, atol=1e-11 * vscale)                # (iii)
        smv2 = m * (vv * vv).sum()
        tk = smv2 * mvv2e / ((3 * n - 3) * kB)                  # compute temp
        ke = 0.5 * mvv2e * smv2                                 # compute ke
        assert t * (1.0 - 24.0 / (3 * n - 3)) < tk < t          # (iv) rotation removed, nothing rescaled
        np.testing.assert_allclose(rows[k, 0], tk, rtol=1e-12)
        np.testing.assert_allclose(rows[k, 2], ke, rtol=1e-12)
        U, W, _, _, _ = X.exact(el, xw, L)
        U, W = float(U), float(W)
        # thermo_press = (dof kB T_kin + W) / 3V * nktv2p: the two terms nearly cancel in a crystal near zero pressure, so the
        # tolerance is relative to their size
        kin, vol = (3 * n - 3) * kB * tk, L ** 3
        press = (kin + W) / (3.0 * vol) * nktv2p
        assert abs(rows[k, 3] - press) <= 1e-10 * (abs(kin) + abs(W)) / (3.0 * vol) * nktv2p, (rows[k, 3], press)
        np.testing.assert_allclose(rows[k, 1], U, rtol=1e-11)
        np.testing.assert_allclose(rows[k, 4], vol, rtol=1e-15)
    assert crossed >= 8                                         # the image flags really were in play


@pytest.mark.parametrize('sz', [4, 5], ids=['Al-256', 'Al-500'])
def test_hmc_energy_error_is_second_order_in_dt_al(sz):
    """fix nve in metal units: dtf = 0.5 dt ftm2v / m for the kick, x += dt v for the drift, velocities drawn with mass m and
    kinetic energy 0.5 mvv2e m v^2.  Over a trajectory of FIXED length (0.016 ps as 4 x 0.004, 8 x 0.002, 16 x 0.001) the error
    dH of velocity Verlet falls 4x per halving of dt only if ftm2v mvv2e = 1 and the kick divides by the mass the draw used: with
    ftm2v = mvv2e the atoms barely accelerate and dH does not converge at all.
    Cold crystals (T = 10-50 K) at a = 7.5 / (0.5 (sqrt 3 + sqrt 3.5)) = 4.163 A, which puts rc = 7.5 A midway between the 6th
    and 7th fcc shells (7.21 and 7.79 A): the unshifted Sutton-Chen energy jumps whenever a pair crosses rc, and no pair does here."""
    import neuralmelting_amd as nm
    n = 4 * sz ** 3
    P = np.linspace(1.0, 8.0, 8, dtype=np.float32)
    T = np.linspace(10.0, 50.0, 8, dtype=np.float32)
    a = X.SC_RC / (0.5 * (np.sqrt(3.0) + np.sqrt(3.5)))
    box = np.full(64, sz * a)
    rng = np.random.default_rng(17)
    x = (lattice.fcc_fractional(sz)[None] * box[0] + 0.04 * (rng.random((64, n, 3)) - 0.5)).reshape(64, -1)
    v = np.zeros_like(x)
    d = np.tile([0.004, 0.004, 0.00390625], (64, 1))
    dh = []
    for nstps, dt in ((4, 0.004), (8, 0.002), (16, 0.001)):
        e = nm.Engine(n, P, T, element='Al', ppos=0.0, pvol=0.0, nstps=nstps)
        try:
            dd = d.copy(); dd[:, 2] = dt
            e.set_state(x, v, box, dd)
            e.set_trace(True)
            e.run_block(1)
            tr = e.trace(1)
        finally:
            e.close()
        assert (tr[:, 0, 0] == 2.0).all()                       # the move was an HMC trajectory
        dh.append(tr[:, 0, 2])
    dh = np.array(dh)
    assert (np.abs(dh[2]) > 1e-9).all()                         # far above round-off
    r1, r2 = dh[0] / dh[1], dh[1] / dh[2]
    print('HMC dt ratios Al-%d: median %.4f %.4f, |dH| at 0.001 ps: %.3g ... %.3g'
          % (n, np.median(r1), np.median(r2), np.abs(dh[2]).min(), np.abs(dh[2]).max()))
    # measured on the MI355X: medians 4.0050 and 4.0012 at both sizes, |dH| 1e-3 ... 4e-3 at 0.001 ps
    assert 3.8 < np.median(r1) < 4.2 and 3.9 < np.median(r2) < 4.1, (np.median(r1), np.median(r2))
    assert np.mean((r2 > 3.5) & (r2 < 4.5)) > 0.9, np.sort(r2)
    for dt, lo, hi in ((0.0005, 0.98, 1.0), (0.04, 0.0, 0.5)):     # measured: acceptance 1.0000 and 0.0000
        e = nm.Engine(n, P, T, element='Al', ppos=0.0, pvol=0.0, nstps=8)
        try:
            dd = d.copy(); dd[:, 2] = dt
            e.set_state(x, v, box, dd)
            e.run_block(32)
            r = e.thermo()
        finally:
            e.close()
        assert (r[:, 12] == 32).all()
        acc = r[:, 13].sum() / r[:, 12].sum()
        print('HMC acceptance Al-%d at dt %g ps: %.4f' % (n, dt, acc))
        assert lo <= acc <= hi, (dt, acc)


def test_npt_pressure_in_bar_equals_imposed_pressure_al():
    """P = < N kT / V - dU/dV > in the ensemble volume_mc samples (test_physics_gpu.py::test_npt_virial_pressure_equals_imposed_pressure),
    here in bar at GPa-scale imposed pressures (5 to 40 kbar, 300 to 900 K, solid), where the criterion's pf = P 1e-30 1e5 /
    (1.60218e-19 kT), thermo_press's nktv2p and the eV energies must agree.  Sutton-Chen here is unshifted, and the 7th fcc shell
    lies across rc = 7.5 A at these densities, so -dU/dV has an impulsive part besides W / 3V.  It is not modelled: for every
    sample, U is evaluated (nm_eval) on the configuration scaled to V (1 +- eps), and the central difference minus the smooth
    part W / 3V of the same evaluation estimates it.  Adding it and the kinetic difference N kB T - (N-1) kB T_kin to the
    reported thermo_press gives an estimator whose mean must be the slot's pressure at all 64 state points.  Production move mix,
    adaptation and exchange on.  The chains are seeded (Philox keyed by seed, slot and step), so the values measured on the
    MI355X and quoted below recur on every run: standard error of a slot's mean 404 bar (median), impulsive term -5.26 kbar on
    average, as large as the imposed pressures themselves."""
    import neuralmelting_amd as nm
    n, eps = 256, 2e-3
    P = np.linspace(5e3, 4e4, 8, dtype=np.float32)
    T = np.linspace(300.0, 900.0, 8, dtype=np.float32)
    x, v, box, d = lattice.init_states(4, P, T, 0.01, 0.004, el='Al')
    d[:, 0] = 0.004
    e = nm.Engine(n, P, T, element='Al')
    ev = nm.Engine(n, P, T, element='Al')                       # evaluates the scaled copies; the chains are not touched
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
                # the reported pressure is thermo_press of these coordinates with the W that nm_eval finds for them
                kin = (n - 1.0) * BOLTZ * r[:, 0]
                wdiff.append(np.abs(r[:, 3] - (kin + W0 / 3.0) / vol * NKTV2P) / ((kin + np.abs(W0) / 3.0) / vol * NKTV2P))
            e.adapt()
            e.exchange(count=False)
        assert (e.status() == 0).all()
    finally:
        e.close()
        ev.close()
    assert np.max(wdiff) < 1e-9, np.max(wdiff)
    r = np.array(samples)                                       # [cycle][slot][17]
    imp = np.array(imp)
    tkin, press, vol = r[:, :, 0], r[:, :, 3], r[:, :, 4]
    Tj = np.tile([float('%f' % t) for t in T], 8)[None, :]
    Pi = np.repeat(P.astype(np.float64), 8)
    pvir = press + (n * BOLTZ * Tj - (n - 1.0) * BOLTZ * tkin) / vol * NKTV2P
    pest = pvir + imp
    nb = 8

    def zscores(a):
        bm = a.reshape(nb, cycles // nb, 64).mean(1)
        se = bm.std(0, ddof=1) / np.sqrt(nb)
        se = np.maximum(se, np.median(se))                      # as in the LJ test: no slot is trusted beyond the typical one
        return (bm.mean(0) - Pi) / se, bm.mean(0) - Pi, se
    z, diff, se = zscores(pest)
    z0, diff0, se0 = zscores(pvir)
    print('NPT Al: |z| max %.2f, mean z %.3f, mean diff %.1f bar, median se %.1f bar; without the impulsive term: mean z %.2f, '
          'mean diff %.1f bar; mean impulsive term %.1f bar' % (np.abs(z).max(), z.mean(), diff.mean(), np.median(se), z0.mean(),
                                                               diff0.mean(), imp.mean()))
    tr = (tkin / Tj).mean()
    tr_se = (tkin / Tj).std(ddof=1) / np.sqrt(tkin.size)
    print('NPT Al: <T_kin/T> %.5f +- %.5f (want %.5f)' % (tr, tr_se, (3.0 * n - 6.0) / (3.0 * n - 3.0)))
    assert (np.abs(z) < 5.0).all(), np.sort(np.abs(z))[-4:]    # measured: max 2.59 over the 64 slots
    assert abs(z.mean()) < 0.5, z.mean()                        # measured: -0.04
    assert abs(diff.mean()) < 4.0 * np.median(se) / 8.0, diff.mean()   # measured: -4.4 bar against a bound of 202 bar
    # without the impulsive term the same data are off by +5.3 kbar (mean z 11.1): the unshifted cutoff's jump is resolved, and
    # a pressure reported off by a factor cannot pass
    assert z0.mean() > 5.0 and diff0.mean() > 2000.0, (z0.mean(), diff0.mean())
    # kinetic temperature in K from thermo_temp (boltz, mvv2e): <T_kin/T> = (3N-6)/(3N-3) = 0.99608 (measured 0.99558 +- 0.00036)
    assert tr_se < 5e-4 and abs(tr - (3.0 * n - 6.0) / (3.0 * n - 3.0)) < 4.0 * tr_se, (tr, tr_se)
