"""The pair entropy of the distr stage without a GPU: the restatement tests/entropy_ref.py against closed forms, the entropy functional of
the rdf (distr.entropy_functional, -ef), nm_distr_entropy's declaration, binding and refusals (which need no device), and the command
line of -le / -ef with the kernel replaced by the restatement."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import entropy_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import distr, reweight

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENT = -7.25e300
ISENT = -77777777
NAMES = ('s', 'sbar', 'nnb', 'smean', 'sbarmean', 'nlow')
INTS = ('nnb', 'nlow')


def call(pos, box, r_m=1.0, sigma=0.1, nbins=16, r_avg=1.0, s_cut=0.0, device=0, ns=None, natoms=None, null=()):
    """the raw ABI on sentinel-filled outputs, NULL for the names in `null`; returns (rc, message, dict of the six arrays)"""
    L = B.load()
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    box = np.ascontiguousarray(box, dtype=np.float32).reshape(-1)
    m, n = pos.shape[0], pos.shape[1]
    out = dict(s=np.full((m, n), SENT), sbar=np.full((m, n), SENT), nnb=np.full((m, n), ISENT, dtype=np.int32), smean=np.full(m, SENT),
               sbarmean=np.full(m, SENT), nlow=np.full(m, ISENT, dtype=np.int32))
    ptr = {k: (None if k in null else out[k].ctypes.data_as(B.c_int32_p if k in INTS else B.c_double_p)) for k in NAMES}
    rc = L.nm_distr_entropy(device, m if ns is None else ns, n if natoms is None else natoms,
                            None if 'pos' in null else pos.ctypes.data_as(B.c_float_p), None if 'box' in null else box.ctypes.data_as(B.c_float_p),
                            float(r_m), float(sigma), int(nbins), float(r_avg), float(s_cut), *[ptr[k] for k in NAMES])
    return rc, (L.nm_distr_last_error().decode() if rc else ''), out


def fcc_integer(cells):
    """fcc with a0 = 2 on integer coordinates: exact in float32; box 2 * cells"""
    base = np.array([[0, 0, 0], [0, 1, 1], [1, 0, 1], [1, 1, 0]])
    g = np.arange(cells) * 2
    pos = (np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 1, 3) + base).reshape(-1, 3)
    return pos.astype(np.float32), np.float32(2 * cells)


def close(a, b, ulps=64):
    """a and b long double, equal to `ulps` roundings of the long double format relative to 1 + |b|"""
    return (np.abs(np.asarray(a, dtype=R.LD) - np.asarray(b, dtype=R.LD)) <= ulps * np.finfo(R.LD).eps * (1 + np.abs(b))).all()


# ---- the restatement against closed forms
@pytest.mark.parametrize('nbins', (1, 2, 7, 64, 1024))
def test_atom_without_entries(nbins):
    """one atom, and an atom whose nearest neighbour lies beyond r_m: -2 pi rho (r_m^3 / 3 + r_m D^2 / 6), to the rounding of the
    float64 grid points k * D (2^-53 each, squared: four of them at most, in units of the long double's 2^-63)"""
    grid_rounding = 4 * 2 ** 10
    one = R.entropy(np.full((1, 1, 3), 0.5), [3.0], 1.5, 0.1, nbins, 1.5)
    assert one['nnb'][0, 0] == 0 and one['navg'][0, 0] == 0
    assert close(one['s'][0, 0], R.no_entries(1, 3.0, 1.5, nbins), grid_rounding)
    assert close(one['sbar'][0, 0], one['s'][0, 0]) and close(one['smean'][0], one['s'][0, 0])
    pos = np.array([[[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 2.0, 2.0]]])
    far = R.entropy(pos, [4.0], 1.9, 0.05, nbins, 2.0)
    assert not far['nnb'].any() and far['navg'].any()
    assert close(far['s'], R.no_entries(3, 4.0, 1.9, nbins), grid_rounding)
    assert (far['s'] < 0).all() and far['e_s'].max() < 1e-12


def test_perfect_fcc_has_one_value():
    p, box = fcc_integer(3)
    out = R.entropy(p[None], [box], 3.0, 0.15, 48, 1.7)
    assert (out['nnb'] == out['nnb'][0, 0]).all() and (out['navg'] == 12).all()
    assert close(out['s'], out['s'][0, 0]) and close(out['sbar'], out['s'][0, 0]) and close(out['sbarmean'], out['s'][0, 0])
    assert out['s'][0, 0] < -1.0


def test_scaling_all_lengths_changes_nothing():
    rng = np.random.default_rng(11)
    box = np.array([4.0, 4.5], dtype=np.float32)
    pos = (rng.random((2, 40, 3)) * box[:, None, None]).astype(np.float32)
    one = R.entropy(pos, box, 1.75, 0.125, 40, 1.25, s_cut=-2.0)
    two = R.entropy(2 * pos, 2 * box, 3.5, 0.25, 40, 2.5, s_cut=-2.0)
    np.testing.assert_array_equal(one['nnb'], two['nnb'])
    np.testing.assert_array_equal(one['navg'], two['navg'])
    np.testing.assert_array_equal(one['nlow'], two['nlow'])
    assert 0 < one['nlow'].sum() < 80
    for k in ('s', 'sbar', 'smean', 'sbarmean'):
        assert close(one[k], two[k], 4096), k


def test_bound_stays_far_below_the_values():
    rng = np.random.default_rng(12)
    box = np.float32((200 / 0.9) ** (1 / 3))
    pos = (rng.random((1, 200, 3)) * box).astype(np.float32)
    out = R.entropy(pos, [box], 0.5 * float(box), 0.1, 256, 1.5)
    assert out['nnb'].max() > 64
    assert (out['e_s'] < 1e-9 * (1 + np.abs(out['s']).astype(np.float64))).all()
    for k in ('e_sbar', 'e_smean', 'e_sbarmean'):
        assert (out[k] >= out['e_s'].max()).all() and (out[k] < 1e-10).all()


# ---- the entropy functional of the rdf
def test_entropy_functional_of_a_synthetic_rdf():
    r = np.linspace(1e-16, 0.5, 6) * 4.0
    g = np.array([[0.0, 0.0, 2.5, 1.0, 0.5, 1.0], [0.0, 1.0, 1.0, 1.0, 1.0, 1.0]], dtype=np.float32)
    nrho = np.array([0.8, 1.1], dtype=np.float32)
    ef, s2 = distr.entropy_functional(g, r, nrho)
    assert ef.dtype == np.float64 and ef.shape == (2, 6) and s2.dtype == np.float64 and s2.shape == (2,)
    want = np.array([[r[0] ** 2, r[1] ** 2, (2.5 * np.log(2.5) - 1.5) * r[2] ** 2, 0.0, (0.5 * np.log(0.5) + 0.5) * r[4] ** 2, 0.0],
                     [r[0] ** 2, 0.0, 0.0, 0.0, 0.0, 0.0]])
    np.testing.assert_allclose(ef, want, rtol=1e-15, atol=0)
    assert (ef[:, 3] == 0.0).all() and ef[0, 1] == r[1] * r[1]              # g = 1 gives 0, g = 0 gives r^2, exactly
    np.testing.assert_allclose(s2, -2 * np.pi * nrho.astype(np.float64) * want.sum(axis=1) * (r[1] - r[0]), rtol=1e-15)
    assert s2[0] < s2[1] < 0 and abs(s2[1]) < 1e-30


# ---- the ABI
def test_symbol_is_declared_exported_and_bound():
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'nm_distr.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+nm_distr_entropy\s*\(', txt)
    assert 'nm_distr_entropy' in B.DISTR_SYMBOLS
    assert hasattr(C.CDLL(B.LIB_PATH), 'nm_distr_entropy')
    f = B.load().nm_distr_entropy
    assert f.restype is C.c_int
    assert f.argtypes == [C.c_int, C.c_int, C.c_int, B.c_float_p, B.c_float_p, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double,
                          B.c_double_p, B.c_double_p, B.c_int32_p, B.c_double_p, B.c_double_p, B.c_int32_p]


NAN, INF = float('nan'), float('inf')
REFUSED = {
    'ns-1': dict(ns=-1), 'natoms0': dict(natoms=0), 'natoms4096': dict(natoms=4096), 'nbins0': dict(nbins=0), 'nbins1025': dict(nbins=1025),
    'sigma0': dict(sigma=0.0), 'sigma-negative': dict(sigma=-0.1), 'sigma-nan': dict(sigma=NAN), 'sigma-inf': dict(sigma=INF),
    'r_m0': dict(r_m=0.0), 'r_m-negative': dict(r_m=-1.0), 'r_m-nan': dict(r_m=NAN), 'r_m-inf': dict(r_m=INF),
    'r_m-beyond-half-the-smaller-box': dict(box=[3.0, 2.7], r_m=1.4), 'r_avg-beyond-half-the-smaller-box': dict(box=[3.0, 2.7], r_avg=1.4),
    'r_avg0': dict(r_avg=0.0), 'r_avg-negative': dict(r_avg=-0.5), 'r_avg-nan': dict(r_avg=NAN), 'r_avg-inf': dict(r_avg=INF),
    's_cut-nan': dict(s_cut=NAN), 'box-zero': dict(box=[3.0, 0.0]), 'box-negative': dict(box=[-3.0, 3.0]), 'box-nan': dict(box=[3.0, NAN]),
    'box-inf': dict(box=[INF, 3.0]), 'null-pos': dict(null=('pos',)), 'null-box': dict(null=('box',)), 'all-outputs-null': dict(null=NAMES),
    'device-1': dict(device=-1),
}


@pytest.mark.parametrize('case', sorted(REFUSED))
def test_refusals_precede_the_device_check(case):
    kw = dict(REFUSED[case])
    rng = np.random.default_rng(5)
    box = np.array(kw.pop('box', [3.0, 3.0]), dtype=np.float32)
    pos = (rng.random((2, 8, 3)) * 2.9).astype(np.float32)
    rc, msg, out = call(pos, box, **kw)
    assert rc == B.NM_ERR_ARG
    assert msg.startswith('nm_distr_entropy:')
    for k in NAMES:
        assert (out[k] == (ISENT if k in INTS else SENT)).all(), k


def test_valid_call_without_a_device_is_a_hip_error():
    """as nm_distr_bondorder: NM_ERR_HIP where that entry finds no device, also for an empty batch, and NM_OK where it finds one"""
    rng = np.random.default_rng(6)
    pos = (rng.random((2, 8, 3)) * 3.0).astype(np.float32)
    box = np.full(2, 3.0, dtype=np.float32)
    L = B.load()
    ls = np.array([6], dtype=np.int32)
    nnb = np.zeros((2, 8), dtype=np.int32)
    for ns in (2, 0):
        sibling = L.nm_distr_bondorder(0, ns, 8, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), 0.0, 1.4, 1,
                                       ls.ctypes.data_as(B.c_int_p), None, None, None, nnb.ctypes.data_as(B.c_int32_p))
        assert sibling in (B.NM_OK, B.NM_ERR_HIP)
        rc, msg, out = call(pos, box, ns=ns, s_cut=-INF)
        assert rc == sibling, msg
        if rc == B.NM_ERR_HIP:
            assert msg.startswith('nm_distr_entropy:') and 'no HIP device' in msg
            for k in NAMES:
                assert (out[k] == (ISENT if k in INTS else SENT)).all(), k


# ---- the command line
def test_parse_args_entropy_flags():
    a = distr.parse_args([])
    assert a.local_entropy is False and a.entropy_functional is False and a.entropy_radius == 0.0 and a.entropy_width == 0.0
    assert a.entropy_grid == 0 and a.entropy_average == 0.0 and a.entropy_threshold is None and a.entropy_atoms is False
    a = distr.parse_args(['-le', '-lr', '0.4', '-lw', '0.01', '-lg', '100', '-lv', '0.2', '-lt', '-4.5', '-la', '-ef'])
    assert a.local_entropy and a.entropy_functional and a.entropy_atoms
    assert (a.entropy_radius, a.entropy_width, a.entropy_grid, a.entropy_average, a.entropy_threshold) == (0.4, 0.01, 100, 0.2, -4.5)
    a = distr.parse_args(['--local_entropy', '--entropy_radius', '0.5', '--entropy_width', '0.02', '--entropy_grid', '1024',
                          '--entropy_average', '0.5', '--entropy_threshold', '0', '--entropy_atoms', '--entropy_functional'])
    assert a.entropy_grid == 1024 and a.entropy_threshold == 0.0 and a.bond_order is False and a.solid is False
    assert distr.parse_args(['-ef']).local_entropy is False
    for bad in (['-lr', '0.51'], ['-lr', '-0.1'], ['-lr', 'nan'], ['-lr'], ['-lw', '-0.1'], ['-lw', 'inf'], ['-lw', 'nan'], ['-lg', '1025'],
                ['-lg', '-1'], ['-lg', '2.5'], ['-lv', '0.6'], ['-lv', '-0.2'], ['-lv', 'nan'], ['-lt', 'nan'], ['-lt']):
        with pytest.raises(SystemExit):
            distr.parse_args(['-le'] + bad)
    for bad in (['-lt', '-4'], ['-la']):                                       # they belong to -le
        with pytest.raises(SystemExit):
            distr.parse_args(bad)


def test_the_entropy_flags_are_new():
    opts = [s for act in distr._parser()._actions for s in act.option_strings]
    assert len(opts) == len(set(opts))
    for f in ('-le', '-lr', '-lw', '-lg', '-lv', '-lt', '-la', '-ef', '--local_entropy', '--entropy_radius', '--entropy_width',
              '--entropy_grid', '--entropy_average', '--entropy_threshold', '--entropy_atoms', '--entropy_functional'):
        assert f in opts


def test_help_says_that_the_defaults_are_not_measured():
    txt = re.sub(r'\s+', ' ', distr._parser().format_help()).replace('Sutton- Chen', 'Sutton-Chen')   # the help's own line break
    flags = ['--entropy_radius', '--entropy_width', '--entropy_grid', '--entropy_average', '--entropy_threshold']
    for a, b in zip(flags[:-1], flags[1:]):
        assert 'a convenience whose suitability for the LJ and Sutton-Chen grids of this package has not yet been measured' in txt[txt.index(a):txt.index(b)]


def test_automatic_parameters():
    for n, sz in ((32, 2), (108, 3), (256, 4), (500, 5), (2048, 8)):
        rm, sigma, nbins, ravg = distr.entropy_params(distr.parse_args(['-le']), n)
        assert rm == min(0.5, 1.4 / sz) and sigma == 0.05 / sz and ravg == distr.bond_cutoff(0.0, n) == 0.853553 / sz
        assert nbins == min(1024, int(np.ceil(2.0 * rm / sigma))) and (nbins == 56 if sz >= 3 else nbins == 40)
    rm, sigma, nbins, ravg = distr.entropy_params(distr.parse_args(['-le', '-lr', '0.3', '-lw', '0.0001', '-lv', '0.25', '-bc', '0.4']), 256)
    assert (rm, sigma, nbins, ravg) == (0.3, 0.0001, 1024, 0.25)
    rm, sigma, nbins, ravg = distr.entropy_params(distr.parse_args(['-le', '-lg', '7', '-bc', '0.4']), 256)
    assert (rm, sigma, nbins, ravg) == (0.35, 0.0125, 7, 0.4)
    with pytest.raises(ValueError, match='-bc'):
        distr.entropy_params(distr.parse_args(['-le']), 4)                    # one cell: the first fcc shell is 0.85 of the box


def write_run(d, name, pn, tn, sn, pos, box):
    pref = str(d / ('%s.lj.fcc.lammps' % name))
    n = pos.shape[-2]
    np.save(pref + '.virial.trgt.npy', np.linspace(1, 8, pn, dtype=np.float32))
    np.save(pref + '.temp.trgt.npy', np.linspace(0.25, 2.5, tn, dtype=np.float32))
    np.save(pref + '.natoms.npy', np.full((pn, tn, sn), n, dtype=np.uint16))
    np.save(pref + '.box.npy', np.asarray(box, dtype=np.float32).reshape(pn, tn, sn))
    np.save(pref + '.pos.npy', np.asarray(pos, dtype=np.float32).reshape(pn, tn, sn, n, 3))
    return pref


def test_main_refuses_bad_parameters_before_any_file_is_written(tmp_path, monkeypatch):
    write_run(tmp_path, 'd1', 1, 1, 1, np.zeros((1, 4, 3)), [2.0])
    monkeypatch.chdir(tmp_path)
    before = sorted(os.listdir(tmp_path))
    for extra in (['-le'], ['-le', '-lr', '0.7'], ['-le', '-lv', '0.25', '-lg', '2000']):
        with pytest.raises(SystemExit):                                       # 4 atoms: the automatic r_avg is 0.85 of the box
            distr.main(['-n', 'd1', '-e', 'LJ'] + extra)
        assert sorted(os.listdir(tmp_path)) == before


def test_main_writes_the_entropy_files(tmp_path, monkeypatch):
    """distr.main with -le / -ef on a 2 x 1 grid of 2 samples each (32-atom fcc crystals and ideal gases in turn), the kernels replaced
    by the restatement (distr.local_entropy) and by a made-up rdf (distr.histograms): the files, their shapes, dtypes and values, the
    parameters handed on, and that the reweighting stage's loader takes the float64 files as they are; without the flags the file set
    is the earlier one"""
    rng = np.random.default_rng(78)
    pn, tn, sn, n = 2, 1, 2, 32
    ns = pn * tn * sn
    p, _ = fcc_integer(2)
    box = (4.0 + 0.25 * np.arange(ns)).astype(np.float32)
    pos = np.array([(p / 4.0 if s % 2 == 0 else rng.random(p.shape)) * b for s, b in enumerate(box)]).astype(np.float32)
    counts = rng.integers(0, 40, (ns, 8)).astype(np.float32) * n
    counts[:, :2] = 0
    seen = []

    def fake_entropy(natoms, box_, pos_, r_m, sigma, nbins, r_avg, s_cut=None, device=0):
        seen.append((r_m, sigma, nbins, r_avg, s_cut))
        o = R.entropy(pos_, box_, r_m, sigma, nbins, r_avg, -np.inf if s_cut is None else s_cut)
        f = lambda x: x.astype(np.float64)
        return f(o['s']), f(o['sbar']), o['nnb'], f(o['smean']), f(o['sbarmean']), o['nlow']

    def fake_histograms(natoms, box_, pos_, r, rv, device=0, **kw):
        return counts / n, np.zeros((ns,) + 3 * (rv.shape[1] - 1,), dtype=np.float32)

    monkeypatch.setattr(distr, 'local_entropy', fake_entropy)
    monkeypatch.setattr(distr, 'histograms', fake_histograms)
    l = float(box.min())
    base = 'd2.lj.fcc.lammps.'
    old = ['cdf', 'dn', 'dni', 'r', 'rdf', 'rv']
    cases = (('plain', [], None, []),
             ('le', ['-le'], (0.5 * l, 0.025 * l, 40, 0.853553 / 2 * l, None), ['leb', 'len', 'les']),
             ('all', ['-le', '-lr', '0.45', '-lw', '0.03', '-lg', '24', '-lv', '0.3', '-lt', '-1.5', '-la', '-ef'],
              (0.45 * l, 0.03 * l, 24, 0.3 * l, -1.5), ['ef', 'leb', 'leba', 'lef', 'len', 'les', 'lesa', 's2']),
             ('ef', ['-ef'], None, ['ef', 's2']))
    for sub, extra, params, new_files in cases:
        d = tmp_path / sub
        d.mkdir()
        write_run(d, 'd2', pn, tn, sn, pos, box)
        monkeypatch.chdir(d)
        before = set(os.listdir(d))
        calls = len(seen)
        distr.main(['-n', 'd2', '-e', 'LJ', '-sb', '8', '-cb', '2'] + extra)
        assert sorted(set(os.listdir(d)) - before) == [base + x + '.npy' for x in sorted(old + new_files)]
        load = lambda x: np.load(str(d / (base + x + '.npy')))
        if params is None:
            assert len(seen) == calls
        else:
            assert len(seen) == calls + 1 and seen[-1] == params
            o = R.entropy(pos, box, *params[:4], -np.inf if params[4] is None else params[4])
            for x, want in (('les', o['smean']), ('leb', o['sbarmean']), ('len', o['nnb'].mean(axis=1))):
                a = load(x)
                assert a.dtype == np.float64 and a.shape == (pn, tn, sn)
                np.testing.assert_array_equal(a.reshape(ns), want.astype(np.float64))
            assert (load('leb').reshape(ns)[0::2] < load('leb').reshape(ns)[1::2]).all()      # crystal below gas
            obs = reweight.load_observables(str(d / base[:-1]), ['les', 'leb'], (pn, tn, sn))   # reweight -ob / -hq take them as they are
            assert len(obs) == 2 and np.array_equal(obs[1], load('leb'))
        if '-lt' in extra:
            a = load('lef')
            assert a.dtype == np.float64 and a.shape == (pn, tn, sn)
            np.testing.assert_array_equal(a.reshape(ns), o['nlow'] / np.float64(n))
            assert 0.0 < a.mean() < 1.0
        if '-la' in extra:
            for x, want in (('lesa', o['s']), ('leba', o['sbar'])):
                a = load(x)
                assert a.dtype == np.float64 and a.shape == (pn, tn, sn, n)
                np.testing.assert_array_equal(a.reshape(ns, n), want.astype(np.float64))
        if '-ef' in extra:
            ef, s2, rdf, r = load('ef'), load('s2'), load('rdf'), load('r')
            assert ef.dtype == np.float32 and ef.shape == rdf.shape == (pn, tn, sn, 8) and s2.dtype == np.float64 and s2.shape == (pn, tn, sn)
            nrho = n / box.astype(np.float64) ** 3
            wef, ws2 = distr.entropy_functional(rdf.reshape(ns, 8), r, (np.float32(n) / box ** 3))
            np.testing.assert_array_equal(ef.reshape(ns, 8), wef.astype(np.float32))
            np.testing.assert_array_equal(s2.reshape(ns), ws2)
            g = rdf.reshape(ns, 8).astype(np.float64)
            assert (g[:, :2] == 0).all() and (g[:, 2:] > 0).any()
            np.testing.assert_allclose(ef.reshape(ns, 8)[:, 1], r[1] ** 2, rtol=1e-6)
            np.testing.assert_allclose(s2.reshape(ns), -2 * np.pi * nrho * wef.sum(axis=1) * (r[1] - r[0]), rtol=1e-6)
