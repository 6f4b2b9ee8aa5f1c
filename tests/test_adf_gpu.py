"""nm_distr_angles (include/nm_distr.h) on the GPU: the raw 64-bit counts through the C-ABI, bit-equal to the numpy
restatement tests/adf_ref.py in every case; the outputs are pre-filled with a sentinel and must be written completely.

Covered: random liquids on both sides of the wave (64) and of 256 atoms, production sizes with a shell of about 50
neighbours, 2 / 64 / 256 edges, boxes that differ inside a batch, more samples than one launch chunk; the fcc known answers;
the tie tests (an fcc lattice whose 60 and 120 degree angles sit on edges, an integer grid); a cluster whose neighbour lists
exceed one LDS tile, empty and single-neighbour shells, coincident atoms, an unwrapped frame, a metal-unit box; invariance
under a permutation of the atoms; edges that do not span [-1, 1]; the command line."""
import os

import numpy as np
import pytest

import adf_ref as A
from neuralmelting_amd import _lib as B
from neuralmelting_amd import distr, lattice

pytestmark = pytest.mark.gpu

SENT = 0xDEADBEEFDEADBEEF


def call(pos, box, ce, r_lo, r_hi, device=0):
    """the raw ABI on a sentinel-filled output; returns (rc, message, adf uint64 [ns][abins])"""
    L = B.load()
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    box = np.ascontiguousarray(box, dtype=np.float32)
    ce = np.ascontiguousarray(ce, dtype=np.float64)
    out = np.full((pos.shape[0], len(ce)), SENT, dtype=np.uint64)
    rc = L.nm_distr_angles(device, pos.shape[0], pos.shape[1], pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p),
                           float(r_lo), float(r_hi), len(ce), ce.ctypes.data_as(B.c_double_p), out.ctypes.data_as(B.c_uint64_p))
    return rc, (L.nm_distr_last_error().decode() if rc else ''), out


def exact(pos, box, ce, r_lo, r_hi):
    """the kernel's counts == the restatement's, bit for bit; returns (counts int64, triplets per sample)"""
    rc, msg, got = call(pos, box, ce, r_lo, r_hi)
    assert rc == 0, msg
    want, trip = A.counts(pos, box, ce, r_lo, r_hi)
    assert (got != SENT).all() and (got[:, 0] == 0).all()
    np.testing.assert_array_equal(got.astype(np.int64), want)
    return want, trip


def liquid(rng, ns, n, rho=0.9, spread=0.0):
    box = ((n / rho) ** (1 / 3) * (1.0 + spread * rng.random(ns))).astype(np.float32)
    pos = (rng.random((ns, n, 3)) * box[:, None, None]).astype(np.float32)
    return pos, box


def perfect_fcc(cells, a0):
    b = np.float32(cells * a0)
    return (lattice.fcc_fractional(cells) * b).astype(np.float32), b


# ---- random liquids, shell (1e-16 l, l/2]
@pytest.mark.parametrize('n', (1, 2, 3, 63, 64, 65, 255, 256, 257, 500))
def test_liquid_half_box_shell_exact(n):
    rng = np.random.default_rng(2000 + n)
    pos, box = liquid(rng, 2 if n <= 257 else 1, n)
    l = float(box.min())
    want, trip = exact(pos, box, A.angle_domain(64)[1], 1e-16 * l, 0.5 * l)
    assert n < 63 or (trip > 0.1 * n ** 3).all()
    assert (want.sum(axis=1) == trip).all()                                  # cos_edges spans [-1, 1]: nothing is dropped


@pytest.mark.parametrize('n', (864, 2048))
def test_production_sizes_fifty_neighbour_shell_exact(n):
    """r_hi = (50 / (4/3 pi rho))^(1/3): about 50 neighbours per centre, 1225 pairs each"""
    rng = np.random.default_rng(2100 + n)
    pos, box = liquid(rng, 1, n)
    r_hi = (50.0 / (4.0 / 3.0 * np.pi * 0.9)) ** (1 / 3)
    want, trip = exact(pos, box, A.angle_domain(64)[1], 1e-16 * float(box.min()), r_hi)
    assert 0.6 * 1225 * n < trip[0] < 1.5 * 1225 * n


@pytest.mark.parametrize('abins', (2, 64, 256))
def test_edge_counts_exact(abins):
    rng = np.random.default_rng(2200 + abins)
    pos, box = liquid(rng, 3, 150)
    l = float(box.min())
    exact(pos, box, A.angle_domain(abins)[1], 1e-16 * l, 0.5 * l)


def test_edges_inside_the_range_drop_the_rest():
    """arbitrary strictly decreasing edges that do not reach +-1: triplets outside are dropped"""
    rng = np.random.default_rng(2300)
    pos, box = liquid(rng, 2, 100)
    l = float(box.min())
    want, trip = exact(pos, box, np.array([0.95, 0.9, 0.5, 0.1, 0.0, -0.3, -0.31, -0.8]), 0.1 * l, 0.45 * l)
    assert (0 < want.sum(axis=1)).all() and (want.sum(axis=1) < trip).all()


def test_boxes_that_differ_inside_one_batch():
    rng = np.random.default_rng(2400)
    pos, box = liquid(rng, 5, 200, spread=0.4)
    l = float(box.min())
    want, _ = exact(pos, box, A.angle_domain(64)[1], 1e-16 * l, 0.5 * l)
    assert len({w.tobytes() for w in want}) == 5


def test_more_samples_than_one_launch_chunk():
    """4096 + 5 samples of 12 atoms: two launches, the second one short"""
    rng = np.random.default_rng(2500)
    ns = 4096 + 5
    pos, box = liquid(rng, ns, 12, rho=0.8, spread=0.3)
    l = float(box.min())
    want, trip = exact(pos, box, A.angle_domain(32)[1], 1e-16 * l, 0.5 * l)
    for s in (0, 4095, 4096, ns - 1):
        assert want[s].sum() > 0


# ---- known answers and ties
@pytest.mark.parametrize('cells,el', ((4, 'LJ'), (5, 'Al')))
def test_fcc_first_shell_known_answer(cells, el):
    a0 = lattice.lattice_constant(el)
    pos, b = perfect_fcc(cells, a0)
    n = len(pos)
    want, trip = exact(pos[None], [b], A.angle_domain(62)[1], 1e-16 * float(b), 0.85 * a0)
    known = np.zeros(62, dtype=np.int64)
    known[[21, 31, 41, 61]] = np.array([24, 12, 24, 6]) * n
    np.testing.assert_array_equal(want[0], known)


@pytest.mark.parametrize('cells,a0', ((4, 1.5276), (3, 1.5276), (4, 2.0)))
def test_fcc_lattice_with_angles_on_edges(cells, a0):
    """64 edges: a[21] = pi/3 and a[42] = 2 pi/3, so the 60 and 120 degree angles of the lattice sit on edges and the
    float32 rounding of the positions decides the side; a0 = 2 gives integer coordinates (cth = 0.5 and -0.5 exactly where
    the cosine table has its rounded values).  Compared with the restatement only."""
    pos, b = perfect_fcc(cells, a0)
    want, trip = exact(pos[None], [b], A.angle_domain(64)[1], 1e-16 * float(b), 0.85 * a0)
    assert trip[0] == 66 * len(pos)
    assert want[0, 20:24].sum() == 24 * len(pos) and want[0, 41:45].sum() == 24 * len(pos)


def test_integer_grid_ties():
    """distinct points of the integer grid of an 8-box, shell up to l/2 = 4 (displacements on +-l/2 count in two images): right
    angles, straight lines and cosines such as 1/2 and 1/sqrt(2) in bulk, against edges that hold exactly these values"""
    rng = np.random.default_rng(2600)
    g = np.array([rng.permutation(512)[:90] for _ in range(2)])
    pos = np.stack([g // 64, (g // 8) % 8, g % 8], axis=-1).astype(np.float32)
    box = np.full(2, 8.0, dtype=np.float32)
    ce = np.array([1.0, np.sqrt(0.5), 0.5, 0.0, -0.5, -np.sqrt(0.5), -1.0])
    want, trip = exact(pos, box, ce, 0.0, 4.0)
    exact(pos, box, A.angle_domain(64)[1], 0.0, 4.0)
    exact(pos, box, np.cos(np.linspace(0.0, np.pi, 5)), 1e-16, 3.0)
    assert (want.sum(axis=1) == trip).all()


# ---- neighbour lists and geometry
def test_cluster_every_atom_neighbours_every_other():
    """530 atoms inside a ball of diameter < l/2: 529 neighbours per centre, three LDS tiles (256 + 256 + 17)"""
    rng = np.random.default_rng(2700)
    n, L = 530, 10.0
    u = rng.normal(size=(n, 3))
    u *= (2.4 * rng.random(n) ** (1 / 3) / np.linalg.norm(u, axis=1))[:, None]
    pos = (u + 5.0).astype(np.float32)[None]
    want, trip = exact(pos, [np.float32(L)], A.angle_domain(64)[1], 1e-16 * L, 0.5 * L)
    assert trip[0] == n * (529 * 528 // 2)


def test_exact_tile_multiples():
    """257 and 513 atoms in a small ball: 256 and 512 neighbours per centre, lists that fill one and two tiles exactly"""
    rng = np.random.default_rng(2750)
    for n in (257, 513):
        u = rng.normal(size=(n, 3))
        u *= (2.4 * rng.random(n) ** (1 / 3) / np.linalg.norm(u, axis=1))[:, None]
        pos = (u + 5.0).astype(np.float32)[None]
        want, trip = exact(pos, [np.float32(10.0)], A.angle_domain(33)[1], 1e-16, 5.0)
        assert trip[0] == n * ((n - 1) * (n - 2) // 2)


def test_empty_and_single_neighbour_shells():
    """a dilute frame with a short shell: centres with no and with one neighbour contribute nothing"""
    rng = np.random.default_rng(2800)
    pos, box = liquid(rng, 2, 100, rho=0.05)
    r_hi = 0.9
    m = np.array([len(A.neighbours(pos[0], box[0], c, 1e-16, r_hi)) for c in range(100)])
    assert (m == 0).any() and (m == 1).any()
    exact(pos, box, A.angle_domain(64)[1], 1e-16, r_hi)
    pos[1] = pos[1, 0]                                                       # every atom on one point: all shells empty
    want, trip = exact(pos[1:], box[1:], A.angle_domain(64)[1], 1e-16, r_hi)
    assert trip[0] == 0 and not want.any()


def test_coincident_atoms():
    """every atom has a twin at d = 0 (outside the shell for r_lo >= 0); the twins share all other neighbours (cth = 1)"""
    rng = np.random.default_rng(2900)
    pos, box = liquid(rng, 2, 120)
    pos[:, 1::2] = pos[:, 0::2]
    l = float(box.min())
    want, _ = exact(pos, box, A.angle_domain(64)[1], 0.0, 0.5 * l)
    assert (want[:, 1] > 0).all()


def test_unwrapped_frame():
    rng = np.random.default_rng(3000)
    pos, box = liquid(rng, 3, 130)
    l = float(box.min())
    wrapped, _ = exact(pos, box, A.angle_domain(64)[1], 1e-16 * l, 0.3 * l)
    pos[0] -= box[0]
    pos[1] += (rng.integers(-1, 2, pos[1].shape) * box[1]).astype(np.float32)
    pos[2] += (rng.integers(-3, 4, pos[2].shape) * box[2]).astype(np.float32)   # beyond the 27 images: fewer neighbours
    got, _ = exact(pos, box, A.angle_domain(64)[1], 1e-16 * l, 0.3 * l)
    assert got[2].sum() < wrapped[2].sum()


def test_metal_unit_box():
    """element Al in Angstrom: displaced 5^3 fcc at a0 = 4.05 (box 20.25), first shell and half box"""
    rng = np.random.default_rng(3100)
    a0 = lattice.lattice_constant('Al')
    pos, b = perfect_fcc(5, a0)
    pos = (pos + 0.3 * (rng.random(pos.shape) - 0.5)).astype(np.float32)[None]
    exact(pos, [b], A.angle_domain(64)[1], 1e-16 * float(b), 0.85 * a0)
    exact(pos[:, :200], [b], A.angle_domain(64)[1], 1e-16 * float(b), 0.5 * float(b))


def test_invariance_under_a_permutation_of_the_atoms():
    rng = np.random.default_rng(3200)
    pos, box = liquid(rng, 2, 300)
    l = float(box.min())
    ce = A.angle_domain(64)[1]
    rc, msg, one = call(pos, box, ce, 1e-16 * l, 0.5 * l)
    assert rc == 0, msg
    rc, msg, two = call(pos[:, rng.permutation(300)], box, ce, 1e-16 * l, 0.5 * l)
    assert rc == 0, msg
    np.testing.assert_array_equal(one, two)
    assert one.sum() > 0


def test_device_ordinal_out_of_range_and_empty_batch():
    rng = np.random.default_rng(3300)
    pos, box = liquid(rng, 2, 20)
    ce = A.angle_domain(16)[1]
    rc, msg, out = call(pos, box, ce, 1e-16, 0.5 * float(box.min()), device=4096)
    assert rc == B.NM_ERR_ARG and msg.startswith('nm_distr_angles:') and (out == SENT).all()
    L = B.load()
    z = np.zeros(1, dtype=np.uint64)
    rc = L.nm_distr_angles(0, 0, 20, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), 1e-16, 1.0, 16,
                           ce.ctypes.data_as(B.c_double_p), z.ctypes.data_as(B.c_uint64_p))
    assert rc == B.NM_OK


# ---- the command line
def test_cli_writes_a_and_adf(tmp_path, monkeypatch):
    """distr.main with -ad on 2 x 2 x 2 frames of 108 atoms: .a.npy / .adf.npy with the documented shapes and dtypes, equal to the
    restatement's counts / natoms cast to float32; the six other files are byte-identical to a run without -ad, which writes
    neither new file"""
    rng = np.random.default_rng(3400)
    pn, tn, sn, n = 2, 2, 2, 108
    names = ('dni', 'r', 'rdf', 'dn', 'rv', 'cdf')
    a0 = 1.6
    frames, boxes = [], []
    for i in range(pn * tn * sn):
        p, b = perfect_fcc(3, a0 + 0.02 * i)
        frames.append((p + 0.25 * (rng.random(p.shape) - 0.5)).astype(np.float32))
        boxes.append(b)
    pos, box = np.array(frames), np.array(boxes, dtype=np.float32)
    natoms = np.full((pn, tn, sn), n, dtype=np.uint16)
    files = {}
    for sub, extra in (('plain', []), ('ang', ['-ad']), ('shell', ['-ad', '-ac', '0.28'])):
        d = tmp_path / sub
        d.mkdir()
        pref = str(d / 'd3.lj.fcc.lammps')
        np.save(pref + '.virial.trgt.npy', np.linspace(1, 8, pn, dtype=np.float32))
        np.save(pref + '.temp.trgt.npy', np.linspace(0.25, 2.5, tn, dtype=np.float32))
        np.save(pref + '.natoms.npy', natoms)
        np.save(pref + '.box.npy', box.reshape(pn, tn, sn))
        np.save(pref + '.pos.npy', pos.reshape(pn, tn, sn, n, 3))
        monkeypatch.chdir(d)
        distr.main(['-n', 'd3', '-e', 'LJ', '-sb', '48', '-cb', '7'] + extra)
        files[sub] = {f: open(os.path.join(d, f), 'rb').read() for f in sorted(os.listdir(d))}
    base = 'd3.lj.fcc.lammps.'
    assert not any(f.endswith(('.a.npy', '.adf.npy')) for f in files['plain'])
    assert sorted(set(files['ang']) - set(files['plain'])) == [base + 'a.npy', base + 'adf.npy']
    for sub in ('ang', 'shell'):
        for nm in names:
            assert files[sub][base + nm + '.npy'] == files['plain'][base + nm + '.npy'], nm
    l = float(box.min())
    for sub, cut in (('ang', 0.5), ('shell', 0.28)):
        a = np.load(str(tmp_path / sub / (base + 'a.npy')))
        adf = np.load(str(tmp_path / sub / (base + 'adf.npy')))
        assert a.dtype == np.float64 and a.shape == (48,)
        np.testing.assert_array_equal(a, np.linspace(1e-16, np.pi, 48))
        assert adf.dtype == np.float32 and adf.shape == (pn, tn, sn, 48)
        want, trip = A.counts(pos, box, np.cos(a), 1e-16 * l, cut * l)
        np.testing.assert_array_equal(adf.reshape(-1, 48), (want.astype(np.float64) / n).astype(np.float32))
        assert (trip > 0).all() and (adf[..., 0] == 0).all()
