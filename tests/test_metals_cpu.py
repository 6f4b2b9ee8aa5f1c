"""Elements Cu and Ni (Sutton-Chen EAM, n = 9) without a GPU: the published parameters reproduce the crystal they were fitted to, the
engine's tables carry them, the C-ABI's box relaxation and initial states equal the Python front end's, and elements without a potential
are refused by name.

Sutton & Chen, Phil. Mag. Lett. 61 (1990) 139: for the fcc crystal of lattice constant a, c = n S_n / (m sqrt(S_m)) (the equilibrium
condition; S_k = sum over the neighbours of (a/r)^k), and the cohesive energies Cu 3.50 eV, Ni 4.44 eV (Al 3.34 eV, the control)."""
import ctypes as C

import numpy as np
import pytest

import metals_ref as M
from neuralmelting_amd import _lib as B
from neuralmelting_amd import lattice

_LD = np.longdouble
COHESIVE = {'Al': 3.34, 'Cu': 3.50, 'Ni': 4.44}
CODES = {'LJ': 0, 'Al': 1, 'Ni': 2, 'Cu': 3}


def fcc_sums(rmax, ks):
    """sum over the fcc lattice (cube edge 1) of |R|^-k for 0 < |R| < rmax, long double"""
    m = int(np.ceil(rmax)) + 1
    g = np.arange(-2 * m, 2 * m + 1)
    i, j, k = np.meshgrid(g, g, g, indexing='ij')
    sel = (i + j + k) % 2 == 0                                  # half-integer points with an even sum: the fcc sites
    r2 = (i[sel] ** 2 + j[sel] ** 2 + k[sel] ** 2).astype(_LD) / 4
    r2 = r2[(r2 > 0) & (r2 < _LD(rmax) * _LD(rmax))]
    return {p: (r2 ** (-_LD(p) / 2)).sum() for p in ks}


def tail(rmax, k):
    """the continuum beyond rmax: 4 pi rho rmax^(3-k) / (k-3), rho = 4 sites per cube"""
    return 4 * np.pi * 4 * _LD(rmax) ** (3 - k) / (k - 3)


@pytest.mark.parametrize('el', ['Al', 'Cu', 'Ni'])
def test_parameters_are_the_published_ones(el):
    eps, a, c, n, rc = lattice.SC[el]
    rmax = 12.0                                                 # lattice constants (>= 10 a), then the analytic tail
    s = fcc_sums(rmax, (n, 6))
    sn, s6 = s[n] + tail(rmax, n), s[6] + tail(rmax, 6)
    # E(a0)/atom = eps [ x^n S_n / 2 - c x^3 sqrt(S_6) ], x = a / a0 (S at a0 = a); dE/da0 = 0 gives x^(n-3) = 6 c sqrt(S_6) / (n S_n)
    x = (6 * c * np.sqrt(s6) / (n * sn)) ** (_LD(1) / (n - 3))
    e0 = eps * (0.5 * x ** n * sn - c * x ** 3 * np.sqrt(s6))
    c_eq = n * sn / (6 * np.sqrt(s6))
    st = fcc_sums(rc / a, (n, 6))                               # what the engine sums: the same crystal truncated at rc
    et = eps * (0.5 * st[n] - c * np.sqrt(st[6]))
    print('%s: a0/a %.6f  E %.4f eV  c_eq %.4f (c = %g)  truncated at rc %.4f eV' % (el, x ** -1, e0, c_eq, c, et))
    assert abs(1 / x - 1) < 1e-3
    assert abs(-e0 / COHESIVE[el] - 1) < 5e-3
    assert abs(c_eq / c - 1) < 1e-4
    assert abs(et / e0 - 1) < 0.03
    # the engine's own lattice sum (lattice.sc_static, the box relaxation's) of the 4^3 crystal at a is that truncated sum
    u, _ = lattice.sc_static(lattice.fcc_fractional(4), 4 * a, el)
    assert abs(u / 256 - float(et)) < 1e-10 * abs(float(et))


def test_tables():
    """one table for both front ends: the reference's lattice constants and masses (remcmc:880-889), Al's cutoff in units of a"""
    assert lattice.LAT['Cu'] == ('fcc', 3.615) and lattice.LAT['Ni'] == ('fcc', 3.524)
    assert lattice.MASS['Cu'] == 63.546 and lattice.MASS['Ni'] == 58.693
    assert lattice.SC['Cu'][:4] == (1.2382e-2, 3.61, 39.432, 9) and lattice.SC['Ni'][:4] == (1.5707e-2, 3.52, 39.432, 9)
    assert abs(M.rc('Cu') - 6.6852) < 1e-4 and abs(M.rc('Ni') - 6.5185) < 1e-4
    assert abs(M.skin('Cu') - 0.53481) < 1e-5 and abs(M.skin('Ni') - 0.52148) < 1e-5
    assert (lattice.SC_EPS, lattice.SC_A, lattice.SC_C, lattice.SC_RC) == (0.033147, 4.05, 16.399, 7.5)   # Al's, unchanged
    from neuralmelting_amd.engine import Engine
    assert Engine.ELEMENTS == CODES
    assert (B.NM_EL_LJ, B.NM_EL_AL, B.NM_EL_NI, B.NM_EL_CU) == (0, 1, 2, 3)


def abi_state(el, sz, P, nt, seed, gslot, dx):
    L = B.load()
    x = np.empty(12 * sz ** 3)
    box = C.c_double(0.0)
    P = np.ascontiguousarray(P, dtype=np.float32)
    rc = L.nm_lattice_state(CODES[el], sz, len(P), nt, P.ctypes.data_as(B.c_float_p), seed, gslot, dx, 0, x.ctypes.data_as(B.c_double_p),
                            C.byref(box))
    assert rc == 0
    return x, box.value


@pytest.mark.parametrize('el,sz', [('Cu', 4), ('Cu', 6), ('Ni', 4), ('Ni', 6)])
def test_relax_box_and_lattice_state_equal_the_python_front_end(el, sz):
    """at 1 to 40 kbar: nm_lattice_state (nm_lattice.h) against lattice.init_states / relax_box (SciPy), as tests/test_lattice_abi.py for Al"""
    P = np.float32([1.0, 1e4, 4e4])
    T = np.linspace(300.0, 900.0, 4, dtype=np.float32)
    x, v, box, d = lattice.init_states(sz, P, T, 0.03125, 0.03125, el=el, seed=256)
    assert np.all(d[:, 2] == 0.00390625)
    for g in (0, 5, 11):
        xa, ba = abi_state(el, sz, P, 4, 256, g, 0.03125)
        assert abs(ba - box[g]) <= 1e-11 * box[g]
        dd = xa - x[g]
        dd -= ba * np.rint(dd / ba)
        assert np.abs(dd).max() < 1e-9
    # the relaxed box really is at the row's pressure, and above the minimum-image limit 2 rc
    for i, p in enumerate(P):
        b = box[4 * i] * 4.0 / sz
        w = lattice.sc_static(lattice.fcc_fractional(4), b, el)[1]
        assert abs(w / (3.0 * b ** 3) * lattice.NKTV2P_METAL - p) < 1e-6 * 4e4
        assert box[4 * i] > 2 * M.rc(el)
    # near zero pressure the edge is the truncated potential's lattice constant, within 0.3 % of a
    assert abs(box[0] / (sz * lattice.SC[el][1]) - 1) < 3e-3


def test_elements_without_a_potential_are_refused():
    """Ti (code 4: bcc, no Sutton-Chen set) and any other code: NM_ERR_UNSUPPORTED from nm_create, naming the supported elements (the
    check comes before any device is touched); Ni and Cu are not refused (on a machine without a GPU they fail later, at the device)"""
    L = B.load()
    P, T = np.float32([1.0]), np.float32([300.0])
    for el, ok in ((4, False), (5, False), (-1, False), (2, True), (3, True)):
        cfg = B.NMConfig()
        cfg.size = C.sizeof(B.NMConfig)
        cfg.element, cfg.natoms, cfg.np, cfg.nt, cfg.row0, cfg.nrows, cfg.nstps = el, 256, 1, 1, 0, 1, 8
        cfg.bulk, cfg.seed, cfg.ppos, cfg.pvol = 1, 256, 0.125, 0.125
        cfg.P, cfg.T = P.ctypes.data_as(B.c_float_p), T.ctypes.data_as(B.c_float_p)
        h = C.c_void_p()
        rc = L.nm_create(C.byref(cfg), C.byref(h))
        if ok:
            assert rc != B.NM_ERR_UNSUPPORTED, L.nm_last_error(None)
            if rc == B.NM_OK:
                L.nm_destroy(h)
        else:
            assert rc == B.NM_ERR_UNSUPPORTED
            msg = L.nm_last_error(None).decode()
            assert 'LJ' in msg and 'Al' in msg and 'Ni' in msg and 'Cu' in msg, msg
    x = np.empty(768)
    box = C.c_double(0.0)
    assert L.nm_lattice_state(4, 4, 1, 1, P.ctypes.data_as(B.c_float_p), 1, 0, 0.03, 0, x.ctypes.data_as(B.c_double_p), C.byref(box)) == B.NM_ERR_ARG
    with pytest.raises(NotImplementedError, match='metal-unit elements are Al, Ni, Cu'):
        lattice.relax_box(4, 1.0, 'Ti')


def test_driver_refuses_ti_by_name(tmp_path):
    from neuralmelting_amd import remcmc
    with pytest.raises(NotImplementedError, match='element Ti is not supported: this engine runs LJ, Al, Ni, Cu'):
        remcmc.Run('-e Ti -ss 4 -pn 2 -tn 2'.split(), cwd=str(tmp_path))


def test_the_gpu_matrix_covers_every_n9_row():
    """tests/test_metals_gpu.py names a configuration for every (kind, workgroups per replica) of Cu and Ni: the row of nm_rows.hip's
    configuration table (NM_CFG_ROWS) for each.  Those rows are Al's with the n = 9 twins, fused where Al's are."""
    import test_metals_gpu as G
    from helpers import cfg_rows
    rows = cfg_rows()
    tested = {(2, 0 if n <= 256 else 1 if n <= 864 else 2, q): G.qs(n)[q] for el, n, q in (c.values for c in G.CASES)}
    assert tested == {k: name for k, (name, _) in rows.items() if k[0] == 2}
    al_twins = {k[1:]: (name.replace('SC', 'SC9'), fused) for k, (name, fused) in rows.items() if k[0] == 1}
    assert {k[1:]: v for k, v in rows.items() if k[0] == 2} == al_twins
