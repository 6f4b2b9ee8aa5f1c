"""numpy restatement of nm_distr_bondorder's definition (include/nm_distr.h), one centre atom at a time (test infrastructure).

Neighbour entries in float32 exactly as tests/adf_ref.py selects them (image-major, the order of lammps_distr.py:99-102), with
the atom index kept.  Everything after that in np.longdouble (x87 extended: eps 1.1e-19): n = v / |v|, the spherical harmonics
from the azimuth and the unnormalised associated-Legendre recurrence (not the route the kernel takes), the sums and the invariants.

tol() is the error bound derived at the kernels (neuralmelting_amd/csrc/nm_distr.h), u = 2^-53, M the largest neighbour count:
per bond e(l) = (3 l^2 + 7 l + 8) u of the norm of the vector (Y_lm)_m; e_q = e(l) + M u; e_qbar = e_q + (M + 1) u;
e_Q = e(l) + (M + 12 + ceil(natoms / 32)) u; and |dx| <= 2 e sqrt(x) + e^2 for each returned square x."""
from math import factorial

import numpy as np

from distr_ref import BR

LD = np.longdouble
U = 2.0 ** -53
PI = LD('3.14159265358979323846264338327950288')


def neighbours(pos, box, c, r_lo, r_hi):
    """(v float32 [M][3], atom index [M]) of the neighbour entries of centre c in one sample, image-major"""
    pos = np.asarray(pos, dtype=np.float32)
    q = pos[c][None, :] + np.float32(box) * BR.astype(np.float32)            # pos[c] + box*br[j], [27][3] float32
    v = pos[None, :, :] - q[:, None, :]                                      # [27][n][3] float32
    d2 = v[..., 0] * v[..., 0]
    d2 = d2 + v[..., 1] * v[..., 1]
    d2 = d2 + v[..., 2] * v[..., 2]
    d = np.sqrt(d2).astype(np.float64)
    keep = (d > r_lo) & (d <= r_hi)
    return v[keep], np.nonzero(keep)[1]


def unit(v):
    """n = v / |v| in long double from float32 (or any) components, [M][3]"""
    w = np.asarray(v).astype(LD).reshape(-1, 3)
    return w / np.sqrt((w * w).sum(axis=1))[:, None]


def harmonics(n, l):
    """Y_lm(n) for m = 0..l (orthonormal, Condon-Shortley phase) as (re, im) long double [M][l+1]; n [M][3] unit vectors"""
    n = np.asarray(n, dtype=LD).reshape(-1, 3)
    z = n[:, 2]
    st = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1])                      # sin(theta) >= 0
    phi = np.arctan2(n[:, 1], n[:, 0])
    re = np.zeros((len(n), l + 1), dtype=LD)
    im = np.zeros((len(n), l + 1), dtype=LD)
    for m in range(l + 1):
        pmm = LD(1)
        for k in range(1, m + 1):
            pmm = pmm * LD(-(2 * k - 1)) * st                                 # P_m^m = (-1)^m (2m-1)!! sin^m
        p1, p0 = np.zeros_like(z), pmm * np.ones_like(z)
        for k in range(m + 1, l + 1):                                         # (k-m) P_k^m = (2k-1) z P_(k-1)^m - (k+m-1) P_(k-2)^m
            p1, p0 = p0, (LD(2 * k - 1) * z * p0 - LD(k + m - 1) * p1) / LD(k - m)
        norm = np.sqrt(LD(2 * l + 1) / (4 * PI) * LD(factorial(l - m)) / LD(factorial(l + m)))
        re[:, m] = norm * p0 * np.cos(m * phi)
        im[:, m] = norm * p0 * np.sin(m * phi)
    return re, im


def invariant(re, im, l):
    """4 pi / (2l+1) sum_{m=-l..l} |q_lm|^2 from the m >= 0 components [..., l+1]"""
    a = re * re + im * im
    return 4 * PI / LD(2 * l + 1) * (a[..., 0] + 2 * a[..., 1:].sum(axis=-1))


def shell_q2(vectors, l):
    """q2 of one centre whose bonds are `vectors` [M][3] (any lengths)"""
    re, im = harmonics(unit(vectors), l)
    return invariant(re.mean(axis=0), im.mean(axis=0), l)


def bond_order2(pos, box, ls, r_lo, r_hi):
    """pos[ns][n][3], box[ns] float32.  Returns (q2, qbar2 long double [ns][n][nl], Q2 long double [ns][nl], nnb int32 [ns][n])"""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    box = np.ascontiguousarray(box, dtype=np.float32).reshape(-1)
    ns, n = pos.shape[0], pos.shape[1]
    nl = len(ls)
    q2 = np.zeros((ns, n, nl), dtype=LD)
    b2 = np.zeros((ns, n, nl), dtype=LD)
    g2 = np.zeros((ns, nl), dtype=LD)
    nnb = np.zeros((ns, n), dtype=np.int32)
    for s in range(ns):
        ent = [neighbours(pos[s], box[s], c, r_lo, r_hi) for c in range(n)]
        nnb[s] = [len(e[1]) for e in ent]
        rows = np.concatenate([np.full(len(e[1]), c) for c, e in enumerate(ent)]) if n else np.zeros(0, dtype=np.int64)
        allv = np.concatenate([e[0] for e in ent])
        un = unit(allv) if len(allv) else np.zeros((0, 3), dtype=LD)
        idx = np.concatenate([e[1] for e in ent])
        nb = nnb[s].astype(LD)
        for i, l in enumerate(ls):
            yre, yim = harmonics(un, l)
            sre = np.zeros((n, l + 1), dtype=LD)
            sim = np.zeros((n, l + 1), dtype=LD)
            np.add.at(sre, rows, yre)
            np.add.at(sim, rows, yim)
            den = np.where(nb > 0, nb, 1)[:, None]
            qre, qim = sre / den, sim / den                                   # q_lm(c), 0 where Nb = 0
            q2[s, :, i] = invariant(qre, qim, l)
            are, aim = qre.copy(), qim.copy()
            np.add.at(are, rows, qre[idx])
            np.add.at(aim, rows, qim[idx])
            b2[s, :, i] = invariant(are / (nb + 1)[:, None], aim / (nb + 1)[:, None], l)
            tot = nb.sum()
            if tot > 0:
                g2[s, i] = invariant(sre.sum(axis=0) / tot, sim.sum(axis=0) / tot, l)
    return q2, b2, g2, nnb


def e_bond(l):
    return (3 * l * l + 7 * l + 8) * U


def bounds(l, nbmax, natoms):
    """(e_q, e_qbar, e_Q) for one l"""
    eq = e_bond(l) + nbmax * U
    return eq, eq + (nbmax + 1) * U, e_bond(l) + (nbmax + 12 + (natoms + 31) // 32) * U


def tol(l, x, nbmax, natoms, which):
    """the derived bound on a returned square x (array or scalar): 2 e sqrt(x) + e^2, e = e_q / e_qbar / e_Q for which = 'q' / 'qbar' /
    'Q'"""
    e = bounds(l, nbmax, natoms)[('q', 'qbar', 'Q').index(which)]
    return 2 * e * np.sqrt(np.maximum(np.asarray(x, dtype=np.float64), 0.0)) + e * e
