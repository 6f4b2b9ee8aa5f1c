"""Structural histograms on the GPU with lammps_distr.py's command line and outputs.

Mirrors the reference's scripts/lammps_distr.py ("distr"): loads <PREFIX>.natoms/.box/.pos.npy written by
lammps_parse.py, computes the per-sample radial distribution over the 27 periodic images (calculate_rdf, distr:123-135)
and the 3-D histogram of pair displacement vectors (calculate_cdf, distr:161-171) — here one kernel launch over all
samples (include/nm_distr.h) instead of a Dask/joblib map of numpy calls — and writes the same .dni/.r/.rdf/.dn/.rv/.cdf
files with the same shapes and dtypes.  With -ad it also writes the angular (bond-angle) distribution the reference names
.a.npy / .adf.npy but leaves switched off (definition: include/nm_distr.h, nm_distr_angles).  With -sf it also writes the
static structure factor on the reciprocal lattice of each sample's box, averaged and maximised over the shells |q| = const
(.q.npy / .sf.npy / .sfm.npy; definition: include/nm_distr.h, nm_distr_sfactor), and the number densities (.nrho.npy).
With -bo it also writes the Steinhardt bond-order parameters q_l, their neighbour average and the global Q_l (.bo*.npy;
definition: include/nm_distr.h, nm_distr_bondorder), and with -bw beside them the third-order invariants w_l, their neighbour average
and the global W_l (.bow*.npy; definition: include/nm_distr.h, nm_distr_bondorder_w).  With -so it also writes the solid-like atoms
and crystal clusters of each sample: the solid fraction, the largest cluster's share, the number of clusters and the mean number of connections (.so*.npy;
definition: include/nm_distr.h, nm_distr_solid).  With -cn it also writes the common neighbour analysis of each sample: the shares
of fcc, hcp, bcc and icosahedral atoms and of the eight signature columns (.cn*.npy; definition: include/nm_distr.h, nm_distr_cna).
With -le it also writes the pair entropy per atom (Piaggi and Parrinello's local-entropy fingerprint) and its neighbour average as
means over each sample (.le*.npy; definition: include/nm_distr.h, nm_distr_entropy).  With -ef it also writes the entropy functional
(g ln g - g + 1) r^2 of the rdf that lammps_distr.py names .ef.npy but leaves switched off, and its integral, the two-body excess
entropy of each sample (.s2.npy).

    python -m neuralmelting_amd.distr -v -n remcmc_init -e LJ -sb 64 -cb 16
    python -m neuralmelting_amd.distr -v -n remcmc_init -e LJ -sb 64 -cb 16 -ad -ac 0.2125
    python -m neuralmelting_amd.distr -v -n remcmc_init -e LJ -sb 64 -cb 16 -sf -sq 16
    python -m neuralmelting_amd.distr -v -n remcmc_init -e LJ -sb 64 -cb 16 -bo -bl 4 6
    python -m neuralmelting_amd.distr -v -n remcmc_init -e LJ -sb 64 -cb 16 -bo -bl 4 6 -bw
    python -m neuralmelting_amd.distr -v -n remcmc_init -e LJ -sb 64 -cb 16 -so -sl 6 -st 0.5 -sx 8
    python -m neuralmelting_amd.distr -v -n remcmc_init -e LJ -sb 64 -cb 16 -cn -cm adaptive
    python -m neuralmelting_amd.distr -v -n remcmc_init -e LJ -sb 64 -cb 16 -le -lt -5.0 -ef
"""
import argparse
import os

import numpy as np

from . import _lib as B
from ._stage import prefix as run_prefix

CNA_MODES = {'fixed': 0, 'adaptive': 1}                     # NM_CNA_FIXED, NM_CNA_ADAPTIVE (include/nm_distr.h)


def _parser():
    p = argparse.ArgumentParser()
    p.add_argument('-v', '--verbose', action='store_true')
    p.add_argument('-p', '--parallel', action='store_true')
    p.add_argument('-c', '--client', action='store_true')
    p.add_argument('-d', '--distributed', action='store_true')
    p.add_argument('-q', '--queue', type=str, default='jobqueue')
    p.add_argument('-a', '--allocation', type=str, default='startup')
    p.add_argument('-nn', '--nodes', type=int, default=1)
    p.add_argument('-np', '--procs_per_node', type=int, default=16)
    p.add_argument('-w', '--walltime', type=int, default=2)
    p.add_argument('-m', '--memory', type=int, default=32)
    p.add_argument('-nw', '--workers', type=int, default=16)
    p.add_argument('-nt', '--threads', type=int, default=1)
    p.add_argument('-mt', '--method', type=str, default='fork')
    p.add_argument('-n', '--name', type=str, default='remcmc_init')
    p.add_argument('-e', '--element', type=str, default='LJ')
    p.add_argument('-sb', '--spherical_bins', type=int, default=64)
    p.add_argument('-cb', '--cartesian_bins', type=int, default=16)
    p.add_argument('-ad', '--angular', action='store_true',
                   help='also write <PREFIX>.a.npy and <PREFIX>.adf.npy: the distribution of the angles between the neighbours of '
                        'each atom, on the domain a = linspace(1e-16, pi, spherical_bins)')
    p.add_argument('-ac', '--angular_cutoff', type=float, default=0.5,
                   help='outer radius of the neighbour shell of -ad as a fraction of the smallest box edge, in (0, 0.5]; '
                        'default 0.5 (the last radial edge).  The first shell of an fcc crystal of SZ cells per edge ends at '
                        'about 0.85/SZ')
    p.add_argument('-sf', '--structure_factor', action='store_true',
                   help='also write <PREFIX>.q.npy, .sf.npy, .sfm.npy and .nrho.npy: the static structure factor S(q) on the '
                        'reciprocal lattice of each sample\'s box, as the mean and the maximum over each shell of equal |q|')
    p.add_argument('-sq', '--q_max', type=int, default=16,
                   help='-sf takes every q = 2 pi (h, k, l) / box with 1 <= h^2 + k^2 + l^2 <= q_max^2; 1..32, default 16')
    p.add_argument('-bo', '--bond_order', action='store_true',
                   help='also write the Steinhardt bond-order parameters: <PREFIX>.bol.npy (the l values), .boq.npy (mean over the '
                        'atoms of q_l), .bob.npy (mean of the neighbour-averaged q_l), .bog.npy (the global Q_l) and .bon.npy (mean '
                        'number of neighbours)')
    p.add_argument('-bl', '--bond_l', type=int, nargs='+', default=[4, 6],
                   help='the l of -bo: 1 to 6 distinct values in 1..12, default 4 6')
    p.add_argument('-bc', '--bond_cutoff', type=float, default=0.0,
                   help='outer radius of the neighbour shell of -bo as a fraction of the smallest box edge, in (0, 0.5]; the '
                        'default 0 means the first fcc shell, 0.853553 / SZ for natoms = 4 SZ^3 (midway between the first and '
                        'second neighbour distances of the perfect crystal)')
    p.add_argument('-ba', '--bond_atoms', action='store_true',
                   help='with -bo also write the per-atom values: <PREFIX>.boqa.npy, .boba.npy and .bona.npy; 8 nl + 4 bytes per atom '
                        'and sample for nl values of l, about 10 GB for a grid of 2^20 samples of 500 atoms at two l')
    p.add_argument('-bw', '--bond_w', action='store_true',
                   help='with -bo also write Steinhardt\'s third-order invariants, normalised to [-1, 1]: <PREFIX>.bow.npy (mean over the '
                        'atoms of w_l), .bowb.npy (mean of the neighbour-averaged w_l) and .bowg.npy (the global W_l), with -ba also '
                        '.bowa.npy and .bowba.npy per atom; the values of -bl must be even (w_l vanishes for odd l)')
    p.add_argument('-so', '--solid', action='store_true',
                   help='also write the solid-like atoms and crystal clusters (ten Wolde, Ruiz-Montero and Frenkel): <PREFIX>.sof.npy '
                        '(solid-like atoms / natoms), .sol.npy (largest cluster / natoms), .soc.npy (number of clusters) and .son.npy '
                        '(mean number of connections per atom).  The neighbour shell is that of -bc')
    p.add_argument('-sl', '--solid_l', type=int, default=6, help='the l of -so: 1..12, default 6')
    p.add_argument('-st', '--solid_threshold', type=float, default=0.5,
                   help='a neighbour entry is a connection of -so if the normalised dot product of the two q_lm vectors exceeds this '
                        'value, in [-1, 1); default 0.5, a common choice whose suitability for the LJ and Sutton-Chen grids of this '
                        'package has not been measured')
    p.add_argument('-sx', '--solid_connections', type=int, default=8,
                   help='an atom is solid-like for -so if it has at least this many connections, >= 1; default 8, a common choice '
                        'whose suitability for the LJ and Sutton-Chen grids of this package has not been measured')
    p.add_argument('-sa', '--solid_atoms', action='store_true',
                   help='with -so also write the per-atom values: <PREFIX>.sona.npy (connections) and .sola.npy (cluster label: the '
                        'smallest atom index of the cluster, -1 for an atom that is not solid-like); 8 bytes per atom and sample')
    p.add_argument('-cn', '--common_neighbours', action='store_true',
                   help='also write the common neighbour analysis: <PREFIX>.cnf.npy, .cnh.npy, .cnb.npy and .cni.npy (fcc, hcp, bcc and '
                        'icosahedral atoms / natoms) and .cns.npy (the share of each of the eight signature columns 421 422 444 666 '
                        '555 544 433 other among the counted neighbour entries)')
    p.add_argument('-cm', '--cna_mode', type=str, choices=sorted(CNA_MODES), default='adaptive',
                   help='adaptive (default): a cutoff per atom from its own 12 and 14 nearest neighbours, no parameter; fixed: the '
                        'one cutoff of -cr for every atom')
    p.add_argument('-cr', '--cna_radius', type=float, default=0.0,
                   help='the search radius (adaptive) or the cutoff (fixed) of -cn as a fraction of the smallest box edge, in (0, 0.5]; '
                        'the default 0 means the first fcc shell of -bc for fixed and min(0.5, 1.3 / SZ) for adaptive, natoms = 4 SZ^3: '
                        'a sphere that holds the 14 nearest neighbours of a crystal with room to spare, whose suitability for the LJ '
                        'and Sutton-Chen grids of this package has not yet been measured')
    p.add_argument('-ca', '--cna_atoms', action='store_true',
                   help='with -cn also write the per-atom type: <PREFIX>.cnta.npy (0 other, 1 fcc, 2 hcp, 3 bcc, 4 ico), one byte per '
                        'atom and sample')
    unmeasured = 'a convenience whose suitability for the LJ and Sutton-Chen grids of this package has not yet been measured'
    p.add_argument('-le', '--local_entropy', action='store_true',
                   help='also write the pair entropy per atom (Piaggi and Parrinello) as float64 means over each sample: <PREFIX>.les.npy '
                        '(mean s), .leb.npy (mean of the neighbour-averaged s) and .len.npy (mean number of entries within the radius '
                        'of -lr), in units of k_B')
    p.add_argument('-lr', '--entropy_radius', type=float, default=0.0,
                   help='the upper limit r_m of the integral of -le as a fraction of the smallest box edge, in (0, 0.5]; the default 0 '
                        'means min(0.5, 1.4 / SZ) for natoms = 4 SZ^3, ' + unmeasured)
    p.add_argument('-lw', '--entropy_width', type=float, default=0.0,
                   help='the width sigma of the Gaussians of -le as a fraction of the smallest box edge, positive; the default 0 means '
                        '0.05 / SZ, ' + unmeasured)
    p.add_argument('-lg', '--entropy_grid', type=int, default=0,
                   help='the number of intervals of the radial grid of -le, 1..1024; the default 0 means min(1024, ceil(2 r_m / sigma)), '
                        + unmeasured)
    p.add_argument('-lv', '--entropy_average', type=float, default=0.0,
                   help='the radius of the neighbour average of -le as a fraction of the smallest box edge, in (0, 0.5]; the default 0 '
                        'means the first fcc shell of -bc, ' + unmeasured)
    p.add_argument('-lt', '--entropy_threshold', type=float, default=None,
                   help='with -le also write <PREFIX>.lef.npy: the atoms whose neighbour-averaged s lies below this value / natoms; no '
                        'default')
    p.add_argument('-la', '--entropy_atoms', action='store_true',
                   help='with -le also write the per-atom values: <PREFIX>.lesa.npy and .leba.npy, 16 bytes per atom and sample')
    p.add_argument('-ef', '--entropy_functional', action='store_true',
                   help='also write <PREFIX>.ef.npy, (g ln g - g + 1) r^2 for every bin of the rdf (r^2 where g = 0), and .s2.npy, the '
                        'two-body excess entropy -2 pi nrho sum over the bins of that times dr, in units of k_B')
    return p


def _cells(natoms):
    """SZ, the cells per edge of an fcc crystal of natoms = 4 SZ^3 atoms, at least 1"""
    return max(1, int(round((int(natoms) / 4.0) ** (1.0 / 3.0))))


def cna_radius(value, natoms, mode):
    """the radius of -cn as a fraction of the smallest box edge: value, or for value 0 bond_cutoff's first fcc shell (fixed) or
    min(0.5, 1.3 / SZ) (adaptive); ValueError outside (0, 0.5]"""
    cut = float(value)
    if cut == 0.0:
        cut = 0.853553 / _cells(natoms) if mode == 'fixed' else min(0.5, 1.3 / _cells(natoms))
    if not 0.0 < cut <= 0.5:
        raise ValueError('-cr/--cna_radius must lie in (0, 0.5]; got %g%s' % (cut, '' if float(value) else
                         ' as the first fcc shell of %d atoms: pass -cr' % int(natoms)))
    return cut


def entropy_params(a, natoms):
    """(r_m, sigma, nbins, r_avg) of -le from the parsed flags, the radii as fractions of the smallest box edge: the values given, or
    for 0 the automatic ones, r_m = min(0.5, 1.4 / SZ), sigma = 0.05 / SZ, nbins = min(1024, ceil(2 r_m / sigma)) and r_avg =
    bond_cutoff's first fcc shell; ValueError outside their ranges"""
    sz = _cells(natoms)
    rm = float(a.entropy_radius) or min(0.5, 1.4 / sz)
    sigma = float(a.entropy_width) or 0.05 / sz
    nbins = int(a.entropy_grid) or min(1024, int(np.ceil(2.0 * rm / sigma)))
    ravg = float(a.entropy_average) or bond_cutoff(a.bond_cutoff, natoms)
    if not 0.0 < rm <= 0.5:
        raise ValueError('-lr/--entropy_radius must lie in (0, 0.5]; got %g' % rm)
    if not (sigma > 0.0 and np.isfinite(sigma)):
        raise ValueError('-lw/--entropy_width must be positive; got %g' % sigma)
    if not 1 <= nbins <= 1024:
        raise ValueError('-lg/--entropy_grid must lie in 1..1024; got %d' % nbins)
    if not 0.0 < ravg <= 0.5:
        raise ValueError('-lv/--entropy_average must lie in (0, 0.5]; got %g' % ravg)
    return rm, sigma, nbins, ravg


def bond_cutoff(value, natoms):
    """the outer radius of -bo as a fraction of the smallest box edge: value, or for value 0 the first fcc shell
    0.853553 / round(cbrt(natoms / 4)); ValueError outside (0, 0.5]"""
    cut = float(value)
    if cut == 0.0:
        cut = 0.853553 / _cells(natoms)
    if not 0.0 < cut <= 0.5:
        raise ValueError('-bc/--bond_cutoff must lie in (0, 0.5]; got %g%s' % (cut, '' if float(value) else
                         ' as the first fcc shell of %d atoms: pass -bc' % int(natoms)))
    return cut


def parse_args(argv=None):
    """lammps_distr.py's flags (distr:15-53); the cluster flags are accepted and ignored"""
    p = _parser()
    a = p.parse_args(argv)
    if not 0.0 <= a.bond_cutoff <= 0.5:
        p.error('-bc/--bond_cutoff must lie in (0, 0.5], or be 0 for the first fcc shell')
    a.bond_l = sorted(a.bond_l)
    if not 1 <= len(a.bond_l) <= 6 or len(set(a.bond_l)) != len(a.bond_l) or a.bond_l[0] < 1 or a.bond_l[-1] > 12:
        p.error('-bl/--bond_l takes 1 to 6 distinct values in 1..12')
    if a.bond_w and not a.bond_order:
        p.error('-bw/--bond_w needs -bo/--bond_order')
    if a.bond_w and any(l % 2 for l in a.bond_l):
        p.error('-bw/--bond_w takes even -bl/--bond_l values only: the third-order invariant vanishes for odd l')
    if not 0.0 < a.angular_cutoff <= 0.5:
        p.error('-ac/--angular_cutoff must lie in (0, 0.5]')
    if not 1 <= a.q_max <= 32:
        p.error('-sq/--q_max must lie in 1..32')
    if not 1 <= a.solid_l <= 12:
        p.error('-sl/--solid_l must lie in 1..12')
    if not -1.0 <= a.solid_threshold < 1.0:
        p.error('-st/--solid_threshold must lie in [-1, 1)')
    if a.solid_connections < 1:
        p.error('-sx/--solid_connections must be at least 1')
    if not 0.0 <= a.cna_radius <= 0.5:
        p.error('-cr/--cna_radius must lie in (0, 0.5], or be 0 for the automatic value')
    if not 0.0 <= a.entropy_radius <= 0.5:
        p.error('-lr/--entropy_radius must lie in (0, 0.5], or be 0 for the automatic value')
    if not (0.0 <= a.entropy_width and np.isfinite(a.entropy_width)):
        p.error('-lw/--entropy_width must be positive, or 0 for the automatic value')
    if not 0 <= a.entropy_grid <= 1024:
        p.error('-lg/--entropy_grid must lie in 1..1024, or be 0 for the automatic value')
    if not 0.0 <= a.entropy_average <= 0.5:
        p.error('-lv/--entropy_average must lie in (0, 0.5], or be 0 for the first fcc shell')
    if a.entropy_threshold is not None and np.isnan(a.entropy_threshold):
        p.error('-lt/--entropy_threshold must be a number')
    if (a.entropy_threshold is not None or a.entropy_atoms) and not a.local_entropy:
        p.error('-lt/--entropy_threshold and -la/--entropy_atoms need -le/--local_entropy')
    return a


def calculate_spatial(natoms, box, sbins, cbins):
    """the domains of calculate_spatial (distr:73-120), same numpy expressions: returns nrho, dni, r, dn, rv"""
    nrho = np.divide(natoms, np.power(box, 3))
    l = np.min(box)
    mr = 1 / 2
    r = np.linspace(1e-16, mr, sbins)
    dr = r[1] - r[0]
    dv = 4 * np.pi * np.square(r) * dr
    r = r * l
    dv = dv * l ** 3
    dni = np.multiply(nrho[:, np.newaxis], dv[np.newaxis, :])
    cb = np.array(3 * (cbins + 1,))
    rv = np.array([np.linspace(0, l, cb[i]) for i in range(len(cb))])
    rv -= l / 2
    drv = rv[0, 1] - rv[0, 0]
    dn = nrho * drv ** 3
    return nrho, dni, r, dn, rv


def _frames(pos, box):
    """pos and box as the entry points of include/nm_distr.h take them: contiguous float32"""
    return np.ascontiguousarray(pos, dtype=np.float32), np.ascontiguousarray(box, dtype=np.float32)


def _device():
    """the device of a command-line run: the launcher's LOCAL_RANK, else 0"""
    return int(os.environ.get('LOCAL_RANK', '0'))


def histograms(natoms, box, pos, r, rv, device=0, want_rdf=True, want_cdf=True):
    """raw counts of calculate_rdf / calculate_cdf for all samples, divided by natoms as the reference does:
    rdf[ns][sbins] float32, cdf[ns][cb][cb][cb] float32"""
    pos, box = _frames(pos, box)
    ns, n = pos.shape[0], pos.shape[1]
    r = np.ascontiguousarray(r, dtype=np.float64)
    ve = np.ascontiguousarray(rv[0], dtype=np.float64)
    if not (np.array_equal(rv[0], rv[1]) and np.array_equal(rv[0], rv[2])):
        raise ValueError('the three cartesian axes must share their bin edges (they do in lammps_distr.py)')
    sb, cb = len(r), len(ve) - 1
    rdf = np.zeros((ns, sb), dtype=np.float32) if want_rdf else None
    cdf = np.zeros((ns, cb, cb, cb), dtype=np.float32) if want_cdf else None
    B.call('nm_distr_histograms', device, ns, n, pos, box, sb, r, cb, ve, rdf, cdf)
    na = np.asarray(natoms).reshape(-1)
    if want_rdf:
        rdf = rdf / na[:, None]                           # rd/natoms (distr:135): float32 / uint16 -> float32
    if want_cdf:
        cdf = cdf / na[:, None, None, None]               # cd/natoms (distr:171)
    return rdf, cdf


def angles(natoms, box, pos, a, r_lo, r_hi, device=0):
    """angular distribution of all samples on the angle edges a (float64 [sbins], increasing from about 0 to pi), neighbour
    shell r_lo < d <= r_hi: the raw counts of nm_distr_angles (each unordered neighbour pair of a centre once, unsigned 64-bit,
    adf[:, 0] = 0) divided by natoms in float64 and cast to float32 [ns][sbins], the dtype of the other histogram files.  The
    exact integers are available through the C-ABI."""
    pos, box = _frames(pos, box)
    ns, n = pos.shape[0], pos.shape[1]
    ce = np.ascontiguousarray(np.cos(np.asarray(a, dtype=np.float64)))   # bins are compared in cosine space
    adf = np.zeros((ns, len(ce)), dtype=np.uint64)
    B.call('nm_distr_angles', device, ns, n, pos, box, float(r_lo), float(r_hi), len(ce), ce, adf)
    na = np.asarray(natoms).reshape(-1).astype(np.float64)
    return (adf.astype(np.float64) / na[:, None]).astype(np.float32)


def sfactor_shells(qmax):
    """the shells of nm_distr_sfactor by enumeration: the n2 = h^2 + k^2 + l^2 in 1..qmax^2 that some integer triple reaches
    (increasing, int64) and the number of triples of each"""
    qmax = int(qmax)
    if not 1 <= qmax <= 32:
        raise ValueError('qmax must lie in 1..32')
    g = np.arange(-qmax, qmax + 1, dtype=np.int64) ** 2
    n2 = (g[:, None, None] + g[None, :, None] + g[None, None, :]).reshape(-1)
    mult = np.bincount(n2[n2 <= qmax * qmax], minlength=qmax * qmax + 1)
    mult[0] = 0
    shells = np.flatnonzero(mult)
    return shells.astype(np.int64), mult[shells].astype(np.int64)


def sfactor(natoms, box, pos, qmax, device=0):
    """static structure factor of all samples on the shells of sfactor_shells(qmax): the shell mean (nm_distr_sfactor's shell
    sum divided by the number of vectors of the shell) and the shell maximum, both float64 [ns][nshell].  natoms is accepted
    for symmetry with histograms() and angles(); the atom count is pos.shape[1]."""
    pos, box = _frames(pos, box)
    ns, n = pos.shape[0], pos.shape[1]
    shells, mult = sfactor_shells(qmax)
    nsh = int(qmax) * int(qmax) + 1
    ssum = np.zeros((ns, nsh), dtype=np.float64)
    smax = np.zeros((ns, nsh), dtype=np.float64)
    B.call('nm_distr_sfactor', device, ns, n, pos, box, int(qmax), ssum, smax)
    return ssum[:, shells] / mult[None, :], smax[:, shells]


def bond_order(natoms, box, pos, ls, r_lo, r_hi, device=0):
    """Steinhardt bond-order parameters of all samples for the l values ls (strictly increasing, 1..12, at most six), neighbour
    shell r_lo < d <= r_hi: q and qbar float64 [ns][natoms][nl] (per atom, qbar averaged over the atom and its neighbours), Q float64
    [ns][nl] (all bonds of the frame) and nb int32 [ns][natoms] (neighbours per atom).  nm_distr_bondorder returns the squares; the
    roots sqrt(max(x, 0)) are taken here in float64.  natoms is accepted for symmetry with histograms(); the atom count is
    pos.shape[1]."""
    pos, box = _frames(pos, box)
    ns, n = pos.shape[0], pos.shape[1]
    ls = np.ascontiguousarray(ls, dtype=np.int32).reshape(-1)
    nl = len(ls)
    q2 = np.zeros((ns, n, nl), dtype=np.float64)
    b2 = np.zeros((ns, n, nl), dtype=np.float64)
    g2 = np.zeros((ns, nl), dtype=np.float64)
    nb = np.zeros((ns, n), dtype=np.int32)
    B.call('nm_distr_bondorder', device, ns, n, pos, box, float(r_lo), float(r_hi), nl, ls, q2, b2, g2, nb)
    root = lambda x: np.sqrt(np.maximum(x, 0.0))
    return root(q2), root(b2), root(g2), nb


def bond_order_w(natoms, box, pos, ls, r_lo, r_hi, device=0):
    """Steinhardt's third-order invariants of all samples for the even l values ls (strictly increasing, 2..12, at most six), neighbour
    shell r_lo < d <= r_hi, beside what bond_order returns, from one call of nm_distr_bondorder_w: w and wbar float64 [ns][natoms][nl]
    (per atom, wbar of the moments averaged over the atom and its neighbours), W float64 [ns][nl] (all bonds of the frame), then q, qbar,
    Q and nb exactly as bond_order gives them.  The library returns the cubic forms w3 and the squares q2; the normalised
    w = w3 / q2^(3/2), in [-1, 1] up to rounding, is formed here in float64 and is 0 where q2 == 0.  Where q_l all but vanishes (l = 2 on
    a cubic lattice, l = 4 on an icosahedron) the ratio is rounding noise: such a w carries no information.  natoms is accepted for
    symmetry with histograms(); the atom count is pos.shape[1]."""
    pos, box = _frames(pos, box)
    ns, n = pos.shape[0], pos.shape[1]
    ls = np.ascontiguousarray(ls, dtype=np.int32).reshape(-1)
    nl = len(ls)
    w3, wb3, q2, b2 = (np.zeros((ns, n, nl), dtype=np.float64) for _ in range(4))
    W3, g2 = (np.zeros((ns, nl), dtype=np.float64) for _ in range(2))
    nb = np.zeros((ns, n), dtype=np.int32)
    B.call('nm_distr_bondorder_w', device, ns, n, pos, box, float(r_lo), float(r_hi), nl, ls, w3, wb3, W3, q2, b2, g2, nb)
    root = lambda x: np.sqrt(np.maximum(x, 0.0))
    hat = lambda w, x: np.divide(w, np.maximum(x, 0.0) ** 1.5, out=np.zeros_like(w), where=x > 0.0)
    return hat(w3, q2), hat(wb3, b2), hat(W3, g2), root(q2), root(b2), root(g2), nb


def solid(natoms, box, pos, l, r_lo, r_hi, s_min, n_min, device=0):
    """solid-like atoms and crystal clusters of all samples (include/nm_distr.h, nm_distr_solid) for one l in 1..12, neighbour shell
    r_lo < d <= r_hi, connection threshold s_min in [-1, 1) and n_min >= 1 connections for a solid-like atom: nconn int32 [ns][natoms]
    (connections per atom), label int32 [ns][natoms] (the smallest atom index of the atom's cluster, -1 if the atom is not solid-like),
    nsolid, nclus and largest int32 [ns] (solid-like atoms, clusters, size of the largest cluster).  natoms is accepted for symmetry
    with histograms(); the atom count is pos.shape[1]."""
    pos, box = _frames(pos, box)
    ns, n = pos.shape[0], pos.shape[1]
    nconn = np.zeros((ns, n), dtype=np.int32)
    label = np.zeros((ns, n), dtype=np.int32)
    nsolid = np.zeros(ns, dtype=np.int32)
    nclus = np.zeros(ns, dtype=np.int32)
    largest = np.zeros(ns, dtype=np.int32)
    B.call('nm_distr_solid', device, ns, n, pos, box, float(r_lo), float(r_hi), int(l), float(s_min), int(n_min), nconn, label, nsolid,
           nclus, largest)
    return nconn, label, nsolid, nclus, largest


def cna(natoms, box, pos, r_lo, r_hi, mode, device=0):
    """common neighbour analysis of all samples (include/nm_distr.h, nm_distr_cna), mode 'adaptive' or 'fixed' (or NM_CNA_ADAPTIVE = 1,
    NM_CNA_FIXED = 0), neighbour shell r_lo < d <= r_hi (adaptive: the search radius): type int32 [ns][natoms] (0 other, 1 fcc, 2 hcp,
    3 bcc, 4 ico), sig int32 [ns][natoms][8] (the atom's entries per signature column 421 422 444 666 555 544 433 other), ntype int32
    [ns][5] and nsig int32 [ns][8] (their sums over the atoms).  natoms is accepted for symmetry with histograms(); the atom count is
    pos.shape[1]."""
    pos, box = _frames(pos, box)
    ns, n = pos.shape[0], pos.shape[1]
    typ = np.zeros((ns, n), dtype=np.int32)
    sig = np.zeros((ns, n, 8), dtype=np.int32)
    ntype = np.zeros((ns, 5), dtype=np.int32)
    nsig = np.zeros((ns, 8), dtype=np.int32)
    B.call('nm_distr_cna', device, ns, n, pos, box, float(r_lo), float(r_hi), int(CNA_MODES.get(mode, mode)), typ, sig, ntype, nsig)
    return typ, sig, ntype, nsig


def local_entropy(natoms, box, pos, r_m, sigma, nbins, r_avg, s_cut=None, device=0):
    """pair entropy per atom of all samples (include/nm_distr.h, nm_distr_entropy) on the grid r_k = k r_m / nbins with Gaussians of
    width sigma, averaged over the entries within r_avg: s and sbar float64 [ns][natoms], nnb int32 [ns][natoms] (entries within r_m),
    smean and sbarmean float64 [ns] and nlow int32 [ns], the atoms with sbar < s_cut (none for s_cut None).  natoms is accepted for
    symmetry with histograms(); the atom count is pos.shape[1]."""
    pos, box = _frames(pos, box)
    ns, n = pos.shape[0], pos.shape[1]
    s = np.zeros((ns, n), dtype=np.float64)
    sbar = np.zeros((ns, n), dtype=np.float64)
    nnb = np.zeros((ns, n), dtype=np.int32)
    smean = np.zeros(ns, dtype=np.float64)
    sbarmean = np.zeros(ns, dtype=np.float64)
    nlow = np.zeros(ns, dtype=np.int32)
    B.call('nm_distr_entropy', device, ns, n, pos, box, float(r_m), float(sigma), int(nbins), float(r_avg),
           -np.inf if s_cut is None else float(s_cut), s, sbar, nnb, smean, sbarmean, nlow)
    return s, sbar, nnb, smean, sbarmean, nlow


def entropy_functional(g, r, nrho):
    """the entropy functional of the rdf g [ns][sbins] on the radii r [sbins] and its integral, in float64: ef = (g ln g - g + 1) r^2
    per bin with g ln g = 0 where g = 0, float64 [ns][sbins], and s2 = -2 pi nrho sum over the bins of ef * dr, float64 [ns], with
    dr = r[1] - r[0] (the radii are evenly spaced)"""
    g = np.asarray(g, dtype=np.float64)
    r = np.asarray(r, dtype=np.float64)
    glg = np.zeros(g.shape, dtype=np.float64)
    filled = g > 0.0
    glg[filled] = g[filled] * np.log(g[filled])
    ef = (glg - g + 1.0) * (r * r)[None, :]
    s2 = -2.0 * np.pi * np.asarray(nrho, dtype=np.float64).reshape(-1) * (ef.sum(axis=1) * (r[1] - r[0]))
    return ef, s2


def main(argv=None):
    a = parse_args(argv)
    dev = _device()
    prefix = run_prefix(a.name, a.element)
    P = np.load(prefix + '.virial.trgt.npy')
    T = np.load(prefix + '.temp.trgt.npy')
    pn, tn = P.size, T.size
    natoms = np.load(prefix + '.natoms.npy').reshape(-1)                      # load_data, distr:63-70
    box = np.load(prefix + '.box.npy').reshape(-1)
    pos = np.load(prefix + '.pos.npy').reshape(-1, natoms[0], 3)
    ns = natoms.size
    if a.bond_order or a.solid:
        try:
            bcut = bond_cutoff(a.bond_cutoff, natoms[0])
        except ValueError as e:                                               # the automatic value needs natoms: refused before any file is written
            raise SystemExit('distr: error: %s' % e)
    if a.common_neighbours:
        try:
            ccut = cna_radius(a.cna_radius, natoms[0], a.cna_mode)
        except ValueError as e:
            raise SystemExit('distr: error: %s' % e)
    if a.local_entropy:
        try:
            lrm, lsig, lbins, lavg = entropy_params(a, natoms[0])
        except ValueError as e:
            raise SystemExit('distr: error: %s' % e)
    nrho, dni, r, dn, rv = calculate_spatial(natoms, box, a.spherical_bins, a.cartesian_bins)
    rns = np.int32(ns / (pn * tn))
    if a.verbose:
        print('computing %s %s samples' % (ns, a.element.lower()))
    rdf, cdf = histograms(natoms, box, pos, r, rv, device=dev)
    g = np.divide(np.array(rdf, dtype=np.float32), dni)                        # distr:305-311
    np.save(prefix + '.dni.npy', dni.reshape(pn, tn, rns, r.size))
    np.save(prefix + '.r.npy', r)
    np.save(prefix + '.rdf.npy', g.reshape(pn, tn, rns, r.size))
    c = np.divide(np.array(cdf, dtype=np.float32), dn[:, np.newaxis, np.newaxis, np.newaxis])   # distr:361-362
    np.save(prefix + '.dn.npy', dn)
    np.save(prefix + '.rv.npy', rv)
    np.save(prefix + '.cdf.npy', c.reshape(pn, tn, rns, *(3 * (rv.shape[1] - 1,))))
    if a.angular:
        l = float(np.min(box))
        ang = np.linspace(1e-16, np.pi, a.spherical_bins)                     # distr:88
        adf = angles(natoms, box, pos, ang, 1e-16 * l, a.angular_cutoff * l, device=dev)
        np.save(prefix + '.a.npy', ang)
        np.save(prefix + '.adf.npy', adf.reshape(pn, tn, rns, ang.size))
    if a.structure_factor:
        shells, _ = sfactor_shells(a.q_max)
        sf, sfm = sfactor(natoms, box, pos, a.q_max, device=dev)
        np.save(prefix + '.q.npy', 2 * np.pi * np.sqrt(shells.astype(np.float64)))   # |q| of a sample = this / its box
        np.save(prefix + '.sf.npy', sf.astype(np.float32).reshape(pn, tn, rns, shells.size))
        np.save(prefix + '.sfm.npy', sfm.astype(np.float32).reshape(pn, tn, rns, shells.size))
        np.save(prefix + '.nrho.npy', nrho.reshape(pn, tn, rns))
    if a.bond_order:
        l = float(np.min(box))
        n, nl = int(natoms[0]), len(a.bond_l)
        if a.bond_w:
            w, wb, wg, q, qb, qg, nb = bond_order_w(natoms, box, pos, a.bond_l, 1e-16 * l, bcut * l, device=dev)
        else:
            q, qb, qg, nb = bond_order(natoms, box, pos, a.bond_l, 1e-16 * l, bcut * l, device=dev)
        np.save(prefix + '.bol.npy', np.array(a.bond_l, dtype=np.int64))
        np.save(prefix + '.boq.npy', q.mean(axis=1).astype(np.float32).reshape(pn, tn, rns, nl))
        np.save(prefix + '.bob.npy', qb.mean(axis=1).astype(np.float32).reshape(pn, tn, rns, nl))
        np.save(prefix + '.bog.npy', qg.astype(np.float32).reshape(pn, tn, rns, nl))
        np.save(prefix + '.bon.npy', nb.mean(axis=1).astype(np.float32).reshape(pn, tn, rns))
        if a.bond_atoms:
            np.save(prefix + '.boqa.npy', q.astype(np.float32).reshape(pn, tn, rns, n, nl))
            np.save(prefix + '.boba.npy', qb.astype(np.float32).reshape(pn, tn, rns, n, nl))
            np.save(prefix + '.bona.npy', nb.reshape(pn, tn, rns, n))
        if a.bond_w:
            np.save(prefix + '.bow.npy', w.mean(axis=1).astype(np.float32).reshape(pn, tn, rns, nl))
            np.save(prefix + '.bowb.npy', wb.mean(axis=1).astype(np.float32).reshape(pn, tn, rns, nl))
            np.save(prefix + '.bowg.npy', wg.astype(np.float32).reshape(pn, tn, rns, nl))
            if a.bond_atoms:
                np.save(prefix + '.bowa.npy', w.astype(np.float32).reshape(pn, tn, rns, n, nl))
                np.save(prefix + '.bowba.npy', wb.astype(np.float32).reshape(pn, tn, rns, n, nl))
    if a.solid:
        l = float(np.min(box))
        n = int(natoms[0])
        nconn, label, nsolid, nclus, largest = solid(natoms, box, pos, a.solid_l, 1e-16 * l, bcut * l, a.solid_threshold,
                                                     a.solid_connections, device=dev)
        np.save(prefix + '.sof.npy', (nsolid / np.float64(n)).astype(np.float32).reshape(pn, tn, rns))
        np.save(prefix + '.sol.npy', (largest / np.float64(n)).astype(np.float32).reshape(pn, tn, rns))
        np.save(prefix + '.soc.npy', nclus.reshape(pn, tn, rns))
        np.save(prefix + '.son.npy', nconn.mean(axis=1).astype(np.float32).reshape(pn, tn, rns))
        if a.solid_atoms:
            np.save(prefix + '.sona.npy', nconn.reshape(pn, tn, rns, n))
            np.save(prefix + '.sola.npy', label.reshape(pn, tn, rns, n))
    if a.common_neighbours:
        l = float(np.min(box))
        n = int(natoms[0])
        typ, _, ntype, nsig = cna(natoms, box, pos, 1e-16 * l, ccut * l, a.cna_mode, device=dev)
        for name, t in (('cnf', 1), ('cnh', 2), ('cnb', 3), ('cni', 4)):
            np.save(prefix + '.%s.npy' % name, (ntype[:, t] / np.float64(n)).astype(np.float32).reshape(pn, tn, rns))
        counted = nsig.sum(axis=1, dtype=np.int64)[:, None]
        share = np.divide(nsig, counted, out=np.zeros(nsig.shape, dtype=np.float64), where=counted > 0)
        np.save(prefix + '.cns.npy', share.astype(np.float32).reshape(pn, tn, rns, 8))
        if a.cna_atoms:
            np.save(prefix + '.cnta.npy', typ.astype(np.int8).reshape(pn, tn, rns, n))
    if a.local_entropy:
        l = float(np.min(box))
        n = int(natoms[0])
        s, sbar, nnb, smean, sbarmean, nlow = local_entropy(natoms, box, pos, lrm * l, lsig * l, lbins, lavg * l, a.entropy_threshold,
                                                            device=dev)
        np.save(prefix + '.les.npy', smean.reshape(pn, tn, rns))
        np.save(prefix + '.leb.npy', sbarmean.reshape(pn, tn, rns))
        np.save(prefix + '.len.npy', nnb.mean(axis=1, dtype=np.float64).reshape(pn, tn, rns))
        if a.entropy_threshold is not None:
            np.save(prefix + '.lef.npy', (nlow / np.float64(n)).reshape(pn, tn, rns))
        if a.entropy_atoms:
            np.save(prefix + '.lesa.npy', s.reshape(pn, tn, rns, n))
            np.save(prefix + '.leba.npy', sbar.reshape(pn, tn, rns, n))
    if a.entropy_functional:
        ef, s2 = entropy_functional(g, r, nrho)
        np.save(prefix + '.ef.npy', ef.astype(np.float32).reshape(pn, tn, rns, r.size))
        np.save(prefix + '.s2.npy', s2.reshape(pn, tn, rns))
    if a.verbose:
        print('all properties pickled')


if __name__ == '__main__':
    main()
