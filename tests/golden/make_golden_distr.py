"""Golden fixtures for the structural histograms: runs the REFERENCE's own calculate_rdf / calculate_cdf
(scripts/lammps_distr.py of the checkout NM_REFERENCE names) — `numba` replaced by an identity `jit` stub, nothing else —
on float32 samples and stores inputs + outputs as numbers in ref_distr.npz.

Keys are <tag>_sb<S>_cb<C>_<field>; one tag is a group of samples that share the spatial domains of calculate_spatial
(l = min(box) over the group).  The first groups (n256, n6) come from rng 42; the production-shape and tie groups added
after them draw from a second generator, so the first ones regenerate bit-for-bit.

    NM_REFERENCE=<checkout of walkernr/neuralMelting> python tests/golden/make_golden_distr.py"""
import importlib.util
import os
import sys
import types

import numpy as np

os.environ['PYTHONDONTWRITEBYTECODE'] = '1'
sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from neuralmelting_amd import distr, lattice  # noqa: E402


def load_reference():
    nb = types.ModuleType('numba')

    def jit(*a, **k):
        if a and callable(a[0]):
            return a[0]
        return lambda f: f
    nb.jit = nb.njit = jit
    sys.modules['numba'] = nb
    spec = importlib.util.spec_from_file_location('lammps_distr_ref', os.path.join(os.environ['NM_REFERENCE'], 'scripts', 'lammps_distr.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    mod = load_reference()
    rng = np.random.default_rng(42)
    out = {}
    cases = []
    # (a) 256-atom displaced fcc crystals at two densities + a random "gas", as float32 like lammps_parse.py writes them
    for sz, boxes in ((4, (6.17, 6.42)),):
        frac = lattice.fcc_fractional(sz)
        for b in boxes:
            x = (frac * b + 0.08 * (rng.random(frac.shape) - 0.5)).astype(np.float32)
            cases.append((x, np.float32(b)))
    cases.append((rng.random((256, 3)).astype(np.float32) * np.float32(6.3), np.float32(6.3)))
    # (b) a tiny sample whose displacements sit exactly on bin edges (0, +-l/2, l/2 in radius)
    l = np.float32(6.0)
    x = np.array([[0, 0, 0], [3, 0, 0], [0, 3, 0], [1.5, 1.5, 0], [0.375, 0.75, 1.125], [5.625, 0, 3]], dtype=np.float32)
    cases.append((x, l))
    groups = {'n256': [c for c in cases if len(c[0]) == 256], 'n6': [c for c in cases if len(c[0]) == 6]}
    for tag, cs in groups.items():
        add_group(mod, out, tag, cs, ((64, 16), (17, 5)))
    for tag, cs, bins in production_and_tie_cases():
        add_group(mod, out, tag, cs, bins)
    np.savez_compressed(os.path.join(HERE, 'ref_distr.npz'), **out)
    print('wrote ref_distr.npz', os.path.getsize(os.path.join(HERE, 'ref_distr.npz')), 'bytes;', sorted(out)[:4])


def production_and_tie_cases():
    """(tag, [(pos, box)], [(sb, cb)]) of the groups after n256 / n6, from their own generator"""
    rng = np.random.default_rng(500)
    frac = lattice.fcc_fractional(5)                     # 5^3 cells: 500 atoms, the production run of run.sh
    # (c) LJ: displaced fcc at two boxes + a random "liquid"; lammps_distr.py -cb 11 (sb 64) as run.sh calls it
    lj = [((frac * b + 0.08 * (rng.random(frac.shape) - 0.5)).astype(np.float32), np.float32(b)) for b in (7.93, 8.31)]
    lj.append(((rng.random((500, 3)) * 8.6).astype(np.float32), np.float32(8.6)))
    # (d) element Al in metal units (A): fcc at a = 4.046 A, one near-perfect and one strongly displaced sample
    b = np.float32(5 * 4.046)
    al = [((frac * b + w * (rng.random(frac.shape) - 0.5)).astype(np.float32), b) for w in (0.1, 1.2)]
    # (e) 80 atoms on the 0.5 grid of a dyadic box L = 8: every displacement component is a multiple of 0.5, so it lands on
    # cdf edges (cb 16 and 8 put them on that grid), on +-l/2, and |d| = l/2 is the last rdf edge; the last atom repeats the
    # first (d = 0).  The second sample shifts a third of the atoms by +-L, as in an unwrapped frame.
    L = np.float32(8.0)
    g = rng.choice(16 ** 3, size=75, replace=False)
    grid = np.stack([g // 256, (g // 16) % 16, g % 16], axis=1) * 0.5
    fixed = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 4], [4, 4, 4]], dtype=np.float64)
    x = np.concatenate([fixed, grid, fixed[:1]]).astype(np.float32)
    xu = x.copy()
    sh = rng.integers(-1, 2, size=x.shape) * (rng.random(x.shape) < 1 / 3)
    xu += (sh * L).astype(np.float32)
    for cb in (16, 8):
        ve = np.linspace(0, L, cb + 1) - L / 2
        for y in (x, xu):
            comp = np.unique(np.concatenate([(y - (y + L * br).reshape(-1, 1, 3)).ravel() for br in BR]))
            assert np.isin(ve, comp).all()
    ties = [(x, L), (xu, L)]
    return [('n500', lj, ((64, 11),)), ('n500al', al, ((64, 11),)), ('n80', ties, ((64, 16), (33, 8)))]


BR = np.array([[b0, b1, b2] for b0 in (-1, 0, 1) for b1 in (-1, 0, 1) for b2 in (-1, 0, 1)], dtype=np.float32)


def add_group(mod, out, tag, cs, bins):
    """the reference's calculate_rdf / calculate_cdf on every sample of one group, at every (sb, cb)"""
    pos = np.array([c[0] for c in cs])
    box = np.array([c[1] for c in cs], dtype=np.float32)
    natoms = np.full(len(cs), pos.shape[1], dtype=np.uint16)
    for sb, cb in bins:
            nrho, dni, r, dn, rv = distr.calculate_spatial(natoms, box, sb, cb)
            rdf, cdf = [], []
            for i in range(len(cs)):
                rd = np.zeros(sb, dtype=np.float32)
                cd = np.zeros((cb, cb, cb), dtype=np.float32)
                rdf.append(np.array(mod.calculate_rdf(natoms[i], box[i], mod_br(mod), pos[i], r, rd)))
                cdf.append(np.array(mod.calculate_cdf(natoms[i], box[i], mod_br(mod), pos[i], rv, cd)))
            key = '%s_sb%d_cb%d_' % (tag, sb, cb)
            out[key + 'pos'], out[key + 'box'], out[key + 'natoms'] = pos, box, natoms
            out[key + 'r'], out[key + 'rv'] = r, rv
            out[key + 'rdf'], out[key + 'cdf'] = np.array(rdf), np.array(cdf)


def mod_br(mod):
    b = [-1, 0, 1]
    return np.array([[b[i], b[j], b[k]] for i in range(3) for j in range(3) for k in range(3)], dtype=np.int8)


if __name__ == '__main__':
    main()
