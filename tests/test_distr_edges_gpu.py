"""nm_distr_histograms (include/nm_distr.h) at the sizes, limits and ties the golden keys do not reach, against the chunked
reference tests/distr_ref.py (itself bit-equal to the oracle and to the reference's outputs, tests/test_distr.py).

Every accepted call: rc 0, the raw counts bit-equal to the reference's, rdf[:, 0] == 0, every output entry written.  Covered:
atom counts on both sides of 64 (padding) and 256 (one atom per thread), 500 / 864 / 2048; the bin limits (sb 256, cb 32) and
the LDS limit of the host's own formula; several launch chunks of 4096 samples; one output NULL; grid positions whose
displacements sit on the cdf edges, on +-l/2 and on the last rdf edge; coincident atoms, unwrapped frames, mixed boxes in one
batch, metal-unit boxes; arbitrary increasing edges; the refusals (untouched outputs) and the 2^24 count guard.  The CLI's
.rdf/.cdf files equal the reference's expressions applied to the reference counts."""
import numpy as np
import pytest

import distr_ref as R
from neuralmelting_amd import _lib as B
from neuralmelting_amd import distr, lattice

pytestmark = pytest.mark.gpu

SENT = -3.5  # what the output buffers hold before a call: a written entry is a count >= 0


def edges(box, sb, cb):
    """r and the cdf edges of one axis as calculate_spatial makes them (l = min(box) over the batch)"""
    _, _, r, _, rv = distr.calculate_spatial(np.ones(len(box)), np.asarray(box, dtype=np.float32), sb, cb)
    return r, rv[0].copy()


def call(pos, box, r, ve, rdf=True, cdf=True, device=0, natoms=None, sbins=None, cbins=None, pass_ve=True):
    """the raw ABI, outputs pre-filled with SENT; returns (rc, message, rdf counts or None, cdf counts or None)"""
    L = B.load()
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    box = np.ascontiguousarray(box, dtype=np.float32)
    r = np.ascontiguousarray(r, dtype=np.float64)
    ve = np.ascontiguousarray(ve, dtype=np.float64)
    ns, n = pos.shape[0], pos.shape[1] if natoms is None else natoms
    sb = len(r) if sbins is None else sbins
    cb = len(ve) - 1 if cbins is None else cbins
    o_r = np.full((ns, max(sb, 1)), SENT, dtype=np.float32) if rdf else None
    o_c = np.full((ns, max(cb, 1) ** 3), SENT, dtype=np.float32) if cdf else None
    fp = lambda a: None if a is None else a.ctypes.data_as(B.c_float_p)
    rc = L.nm_distr_histograms(device, ns, n, fp(pos), fp(box), sb, r.ctypes.data_as(B.c_double_p), cb,
                               ve.ctypes.data_as(B.c_double_p) if pass_ve else None, fp(o_r), fp(o_c))
    msg = L.nm_distr_last_error().decode() if rc != 0 else ''
    if o_c is not None and rc == 0:
        o_c = o_c.reshape(ns, cb, cb, cb)
    return rc, msg, o_r, o_c


def exact(pos, box, r, ve):
    """the kernel's two histograms == the reference's counts, bit for bit; returns them"""
    rc, msg, rd, cd = call(pos, box, r, ve)
    assert rc == 0, msg
    er, ec = R.counts(pos, box, r, ve)
    assert (rd[:, 0] == 0).all()
    np.testing.assert_array_equal(rd, er.astype(np.float32))
    np.testing.assert_array_equal(cd, ec.astype(np.float32))
    assert er.max() < 2 ** 24 and ec.max() < 2 ** 24
    return rd, cd


def liquid(rng, ns, n, rho=0.9, spread=0.0):
    """ns random frames of n atoms at about density rho, boxes that differ by up to `spread`"""
    box = ((n / rho) ** (1 / 3) * (1.0 + spread * rng.random(ns))).astype(np.float32)
    pos = (rng.random((ns, n, 3)) * box[:, None, None]).astype(np.float32)
    return pos, box


def fcc(cells, a, ns, rng, w):
    """ns displaced fcc frames of 4 cells^3 atoms at lattice constant a (float32, as lammps_parse.py writes them)"""
    frac = lattice.fcc_fractional(cells)
    b = np.float32(cells * a)
    pos = np.array([(frac * b + w * (rng.random(frac.shape) - 0.5)).astype(np.float32) for _ in range(ns)])
    return pos, np.full(ns, b, dtype=np.float32)


# ---- atom counts: padding to 64, one or several atoms per thread (256 threads), production sizes
NS_OF = {864: 1, 2048: 1}
COUNTS = [(n, 64, 11) for n in (1, 2, 63, 64, 65, 255, 256, 257, 500, 511, 513, 864, 2048)]
COUNTS += [(n, sb, cb) for n in (1, 65, 257, 513) for sb, cb in ((2, 1), (17, 5))]


@pytest.mark.parametrize('n,sb,cb', COUNTS, ids=['n%d-sb%d-cb%d' % c for c in COUNTS])
def test_atom_counts_exact(n, sb, cb):
    rng = np.random.default_rng(1000 + n + sb)
    ns = NS_OF.get(n, 3 if n <= 257 else 2)
    pos, box = liquid(rng, ns, n, spread=0.05)
    r, ve = edges(box, sb, cb)
    rd, cd = exact(pos, box, r, ve)
    assert cd.sum() >= n * ns  # every self pair of image 0 sits at the centre


# ---- bin and LDS limits
def test_largest_bins_exact():
    """sb 256, cb 32 at 500 atoms: 146,552 B of LDS"""
    rng = np.random.default_rng(7)
    pos, box = fcc(5, 1.6, 2, rng, 0.2)
    r, ve = edges(box, 256, 32)
    exact(pos, box, r, ve)


def test_lds_edge_of_the_host_formula():
    """at sb 256, cb 32: 1216 atoms need 163,592 B of LDS (accepted, exact); 1217 atoms need 164,376 B > 160 KiB (refused)"""
    rng = np.random.default_rng(8)
    pos, box = liquid(rng, 1, 1217)
    r, ve = edges(box, 256, 32)
    exact(pos[:, :1216], box, r, ve)
    rc, msg, rd, cd = call(pos, box, r, ve)
    assert rc == B.NM_ERR_ARG and 'LDS' in msg
    assert (rd == SENT).all() and (cd == SENT).all()


REFUSED = {'natoms4096': dict(natoms=4096), 'natoms0': dict(natoms=0), 'sb1': dict(sbins=1), 'sb257': dict(sbins=257),
           'cb0': dict(cbins=0), 'cb33': dict(cbins=33), 'device-1': dict(device=-1), 'device4096': dict(device=4096)}


@pytest.mark.parametrize('case', sorted(REFUSED))
def test_refusals_leave_outputs_untouched(case):
    kw = REFUSED[case]
    rng = np.random.default_rng(9)
    n = kw.get('natoms') or 8
    pos, box = liquid(rng, 2, max(n, 1))
    sb, cb = kw.get('sbins', 64), kw.get('cbins', 11)
    r = np.linspace(1e-16, 0.5, max(sb, 1)) * box.min()
    ve = np.linspace(0, box.min(), max(cb, 0) + 1) - box.min() / 2
    rc, msg, rd, cd = call(pos, box, r, ve, **kw)
    assert rc == B.NM_ERR_ARG and msg.startswith('nm_distr_histograms:')
    assert (rd == SENT).all() and (cd == SENT).all()


# ---- launch chunks of 4096 samples
def test_several_launch_chunks_every_sample_exact():
    """2 * 4096 + 3 samples of 20 atoms, a box of its own per sample: three launches, the last one short"""
    rng = np.random.default_rng(10)
    ns = 2 * 4096 + 3
    pos, box = liquid(rng, ns, 20, rho=0.8, spread=0.3)
    r, ve = edges(box, 64, 11)
    rd, cd = exact(pos, box, r, ve)
    for s in (0, 4095, 4096, 8191, 8192, ns - 1):
        assert rd[s].sum() > 0 and cd[s].sum() > 0


# ---- one output NULL
@pytest.mark.parametrize('n', (65, 500))
def test_one_output_null_equals_that_half(n):
    rng = np.random.default_rng(11 + n)
    pos, box = liquid(rng, 3, n, spread=0.1)
    r, ve = edges(box, 64, 11)
    rd, cd = exact(pos, box, r, ve)
    for kw in (dict(cdf=False), dict(cdf=False, cbins=0, pass_ve=False)):
        rc, msg, rd1, cd1 = call(pos, box, r, ve, **kw)
        assert rc == 0, msg
        assert cd1 is None
        np.testing.assert_array_equal(rd1, rd)
    rc, msg, rd1, cd1 = call(pos, box, r, ve, rdf=False)
    assert rc == 0, msg
    np.testing.assert_array_equal(cd1, cd)
    na = np.full(3, n, dtype=np.uint16)
    rv = distr.calculate_spatial(na, box, 64, 11)[4]
    g_r, g_c = distr.histograms(na, box, pos, r, rv)
    o_r, none_c = distr.histograms(na, box, pos, r, rv, want_cdf=False)
    none_r, o_c = distr.histograms(na, box, pos, r, rv, want_rdf=False)
    assert none_c is None and none_r is None
    np.testing.assert_array_equal(o_r, g_r)
    np.testing.assert_array_equal(o_c, g_c)
    np.testing.assert_array_equal(g_r, R.normalized(rd.astype(np.int64), na))


# ---- ties and geometry
def grid_frames(rng, ns, n, L, h):
    """ns frames of n distinct points of the h-grid of the box L"""
    m = int(round(L / h))
    out = []
    for _ in range(ns):
        g = rng.choice(m ** 3, size=n, replace=False)
        out.append(np.stack([g // (m * m), (g // m) % m, g % m], axis=1) * h)
    return np.array(out, dtype=np.float32)


@pytest.mark.parametrize('sb,cb', ((64, 16), (64, 8), (33, 32), (64, 11)))
def test_dyadic_grid_ties(sb, cb):
    """L = 8 and a 0.25 grid: every displacement component is on a cdf edge (cb a power of 2), on +-l/2, and pairs at
    |d| = l/2 = the last rdf edge; the second frame adds coincident atoms (d = 0: outside the rdf, inside the cdf)"""
    rng = np.random.default_rng(12)
    L = 8.0
    pos = grid_frames(rng, 3, 96, L, 0.25)
    pos[0, :4] = [[0, 0, 0], [4, 0, 0], [0, 4, 0], [4, 4, 4]]
    pos[1, 10:20] = pos[1, 0:10]
    pos[2] += (rng.integers(-1, 2, pos[2].shape) * L).astype(np.float32)  # unwrapped
    box = np.full(3, L, dtype=np.float32)
    r, ve = edges(box, sb, cb)
    assert r[-1] == L / 2 and ve[0] == -L / 2 and ve[-1] == L / 2
    rd, cd = exact(pos, box, r, ve)
    comp = np.concatenate([(pos[0] - (pos[0] + L * br).reshape(-1, 1, 3)).ravel() for br in R.BR.astype(np.float32)])
    if cb in (8, 16, 32):
        assert np.isin(ve, comp).all()
    assert rd[0, -1] > 0


def test_coincident_atoms():
    rng = np.random.default_rng(13)
    pos, box = liquid(rng, 2, 300)
    pos[:, 1::2] = pos[:, 0::2]  # every atom has a twin
    r, ve = edges(box, 64, 11)
    rd, cd = exact(pos, box, r, ve)
    assert cd.sum() >= 2 * 300 * 2


def test_unwrapped_positions():
    """coordinates below 0 and at or above L, as in an unwrapped frame"""
    rng = np.random.default_rng(14)
    pos, box = liquid(rng, 3, 257)
    pos[0] -= box[0]                                                    # all negative
    pos[1] += (rng.integers(-2, 3, pos[1].shape) * box[1]).astype(np.float32)
    pos[2, :10, 0] = box[2]                                             # exactly L
    r, ve = edges(box, 64, 11)
    exact(pos, box, r, ve)


def test_mixed_boxes_in_one_batch():
    """l = min(box): larger boxes are histogrammed on the smallest one's domains"""
    rng = np.random.default_rng(15)
    pos, box = liquid(rng, 4, 500, spread=0.4)
    r, ve = edges(box, 64, 11)
    exact(pos, box, r, ve)


def test_metal_unit_boxes():
    """element Al in A: fcc at a = 4.046 (box 20.23) near-perfect and strongly displaced, and a 864-atom frame (box 24.3)"""
    rng = np.random.default_rng(16)
    pos, box = fcc(5, 4.046, 2, rng, 0.1)
    pos[1] += (1.2 * (rng.random(pos[1].shape) - 0.5)).astype(np.float32)
    for sb, cb in ((64, 11), (17, 5)):
        r, ve = edges(box, sb, cb)
        exact(pos, box, r, ve)
    pos, box = fcc(6, 4.046, 1, rng, 0.3)
    r, ve = edges(box, 64, 11)
    exact(pos, box, r, ve)


# ---- arbitrary increasing edges: the guess of bin_near is far off, the walk takes many steps
@pytest.mark.parametrize('which', ('geometric', 'offcentre', 'clustered', 'dyadic'))
def test_arbitrary_edges(which):
    """'dyadic': uneven edges on the 0.25 grid of the positions, so the walk up from a low guess ends on ties"""
    rng = np.random.default_rng(17)
    pos, box = liquid(rng, 2, 300)
    l = float(box.min())
    if which == 'dyadic':
        box = np.full(2, 8.0, dtype=np.float32)
        pos = grid_frames(rng, 2, 120, 8.0, 0.25)
        r = np.array([0.0, 0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 2.5, 3.0, 3.75, 4.0])
        ve = np.array([-4.0, -3.5, -3.25, -2.0, -1.0, -0.5, 0.0, 0.25, 0.5, 1.0, 3.0, 4.0])
    elif which == 'geometric':
        r, ve = np.geomspace(1e-3, l / 2, 64), np.geomspace(0.01, l / 2, 12) - 0.6
    elif which == 'offcentre':
        r, ve = np.linspace(0.3 * l, 0.45 * l, 40), np.linspace(-0.1 * l, 0.4 * l, 9)
    else:
        r = np.concatenate([np.linspace(0.0, 0.9, 200), np.linspace(1.0, l / 2, 56)])
        ve = np.concatenate([np.linspace(-l / 2, -l / 2 + 0.1, 30), [0.0, l / 4]])
    exact(pos, box, r, ve)


# ---- the 2^24 count guard
def test_count_of_2_24_is_refused():
    """10^3 fcc cells at a = 2 in L = 20: integer coordinates, so displacements sit on +-l/2 and count in two images per
    axis; at cb 1 the one cdf bin holds more than 2^24 counts (computed here exactly), and the call is refused"""
    c = np.array([[0, 0, 0], [1, 1, 0], [1, 0, 1], [0, 1, 1]])
    g = np.stack(np.meshgrid(*(np.arange(10),) * 3, indexing='ij'), -1).reshape(-1, 1, 3) * 2
    x = (g + c[None]).reshape(-1, 3).astype(np.int64)
    d = np.arange(-19, 20)                                              # x[a] - x[b] per axis
    images = (np.abs(d) <= 10).astype(np.int64) + (np.abs(d - 20) <= 10) + (np.abs(d + 20) <= 10)
    total = sum(int((images[dd[..., 0]] * images[dd[..., 1]] * images[dd[..., 2]]).sum())
                for dd in (x[a:a + 500, None, :] - x[None, :, :] + 19 for a in range(0, 4000, 500)))
    assert total == 18524000 and total >= 2 ** 24 > 4000 ** 2
    pos, box = x[None].astype(np.float32), np.float32([20.0])
    r, ve = edges(box, 64, 1)
    rc, msg, rd, cd = call(pos, box, r, ve)
    assert rc == B.NM_ERR_ARG and '2^24' in msg
    rc, msg, rd, cd = call(pos, box, r, ve, rdf=False)
    assert rc == B.NM_ERR_ARG and '2^24' in msg


def test_4000_random_atoms_accepted():
    """a 4000-atom random frame at cb 11 stays below 2^24 everywhere: accepted (an exact reference costs minutes on one core)"""
    rng = np.random.default_rng(18)
    pos, box = liquid(rng, 1, 4000)
    r, ve = edges(box, 64, 11)
    rc, msg, rd, cd = call(pos, box, r, ve)
    assert rc == 0, msg
    assert np.isfinite(rd).all() and np.isfinite(cd).all() and (rd >= 0).all() and (cd >= 0).all()
    assert (rd[:, 0] == 0).all() and 0 < cd.sum() <= 27 * 4000 ** 2 and cd.max() < 2 ** 24


# ---- the command line: values of .rdf.npy / .cdf.npy
def test_cli_values(tmp_path, monkeypatch):
    """distr.main at -sb 64 -cb 11 on 2 x 2 x 2 distinct 500-atom frames: .rdf / .cdf are the reference's expressions
    (lammps_distr.py:305-311, 361-362) on the reference counts, in (pn, tn, rns) order; .dni/.dn/.r/.rv are calculate_spatial's"""
    rng = np.random.default_rng(19)
    pn, tn, sn, n = 2, 2, 2, 500
    pref = str(tmp_path / 'd2.lj.fcc.lammps')
    np.save(pref + '.virial.trgt.npy', np.linspace(1, 8, pn, dtype=np.float32))
    np.save(pref + '.temp.trgt.npy', np.linspace(0.25, 2.5, tn, dtype=np.float32))
    pos, box = fcc(5, 1.6, pn * tn * sn, rng, 0.3)
    box = box + np.arange(pn * tn * sn, dtype=np.float32) * np.float32(0.05)
    pos = pos * (box / box[0])[:, None, None].astype(np.float32)
    natoms = np.full((pn, tn, sn), n, dtype=np.uint16)
    np.save(pref + '.natoms.npy', natoms)
    np.save(pref + '.box.npy', box.reshape(pn, tn, sn))
    np.save(pref + '.pos.npy', pos.reshape(pn, tn, sn, n, 3))
    monkeypatch.chdir(tmp_path)
    distr.main(['-n', 'd2', '-e', 'LJ', '-sb', '64', '-cb', '11'])
    na = natoms.reshape(-1)
    nrho, dni, r, dn, rv = distr.calculate_spatial(na, box, 64, 11)
    er, ec = R.counts(pos, box, r, rv[0])
    G = np.divide(np.array(list(R.normalized(er, na)), dtype=np.float32), dni).reshape(pn, tn, sn, 64)
    Cd = np.divide(np.array(list(R.normalized(ec, na)), dtype=np.float32), dn[:, None, None, None]).reshape(pn, tn, sn, 11, 11, 11)
    got_r, got_c = np.load(pref + '.rdf.npy'), np.load(pref + '.cdf.npy')
    assert got_r.dtype == G.dtype and got_c.dtype == Cd.dtype
    np.testing.assert_array_equal(got_r, G)
    np.testing.assert_array_equal(got_c, Cd)
    np.testing.assert_array_equal(np.load(pref + '.dni.npy'), dni.reshape(pn, tn, sn, 64))
    np.testing.assert_array_equal(np.load(pref + '.dn.npy'), dn)
    np.testing.assert_array_equal(np.load(pref + '.r.npy'), r)
    np.testing.assert_array_equal(np.load(pref + '.rv.npy'), rv)
    assert len({s.tobytes() for s in got_r.reshape(-1, 64)}) == pn * tn * sn
