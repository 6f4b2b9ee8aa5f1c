"""numpy restatement of nm_distr_bondorder_w's definition (include/nm_distr.h), one centre atom at a time (test infrastructure).

The moments q_lm(c), qbar_lm(c) and Q_lm are those of tests/bondorder_ref.py (its neighbour entries, unit vectors and harmonics, in
np.longdouble).  Wigner's 3j symbols (l l l; m1 m2 m3) come from Racah's formula in exact fractions.Fraction arithmetic: the square of
the symbol is a rational number, and only its root is taken, in 60 decimal digits, before the conversion to long double.  The triple
sum runs over every (m1, m2) with |m1 + m2| <= l in long double complex arithmetic.

tol() is the error bound derived at the kernels (neuralmelting_amd/csrc/nm_distr_w.h), u = 2^-53: with x the matching square, e the
matching e_q / e_qbar / e_Q of bondorder_ref.bounds and n_l non-zero terms,
|w3 - exact| <= 3 e x + 3 e^2 sqrt(x) + e^3 + (n_l + 12) u (sqrt(x) + e)^3."""
from decimal import Decimal, getcontext
from fractions import Fraction
from functools import lru_cache
from math import factorial

import numpy as np

import bondorder_ref as R

LD = R.LD
CLD = np.clongdouble
U = R.U


def n_terms(l):
    """the symbols (l l l; m1 m2 m3) that do not vanish: all 3 l^2 + 3 l + 1 triples but twelve at l = 8"""
    return {2: 19, 4: 61, 6: 127, 8: 205, 10: 331, 12: 469}[l]


def wigner3j_squared(j1, j2, j3, m1, m2, m3):
    """(sign, square) of the 3j symbol by Racah's formula, exact: the symbol is sign * sqrt(square)"""
    if m1 + m2 + m3 != 0 or abs(m1) > j1 or abs(m2) > j2 or abs(m3) > j3 or not abs(j1 - j2) <= j3 <= j1 + j2:
        return 0, Fraction(0)
    f = factorial
    delta = Fraction(f(j1 + j2 - j3) * f(j1 - j2 + j3) * f(-j1 + j2 + j3), f(j1 + j2 + j3 + 1))
    pref = delta * f(j1 + m1) * f(j1 - m1) * f(j2 + m2) * f(j2 - m2) * f(j3 + m3) * f(j3 - m3)
    s = Fraction(0)
    for k in range(0, j1 + j2 - j3 + 1):
        d = (j1 + j2 - j3 - k, j1 - m1 - k, j2 + m2 - k, j3 - j2 + m1 + k, j3 - j1 - m2 + k)
        if min(d) < 0:
            continue
        s += Fraction((-1) ** k, f(k) * f(d[0]) * f(d[1]) * f(d[2]) * f(d[3]) * f(d[4]))
    s *= -1 if (j1 - j2 - m3) % 2 else 1
    return (s > 0) - (s < 0), pref * s * s


def _root(fr):
    """sqrt of a non-negative Fraction as long double (60 digits before the conversion)"""
    getcontext().prec = 60
    return LD(str((Decimal(fr.numerator) / Decimal(fr.denominator)).sqrt()))


def wigner3j(j1, j2, j3, m1, m2, m3):
    sign, sq = wigner3j_squared(j1, j2, j3, m1, m2, m3)
    return LD(sign) * _root(sq)


@lru_cache(maxsize=None)
def table(l):
    """the terms of T_l: (m1 [n], m2 [n], m3 [n] int, symbol [n] long double), m1 ascending, then m2: the kernels' order"""
    rows = [(m1, m2, -m1 - m2) for m1 in range(-l, l + 1) for m2 in range(-l, l + 1) if abs(m1 + m2) <= l]
    rows = [r for r in rows if wigner3j_squared(l, l, l, *r)[0] != 0]
    assert len(rows) == n_terms(l)
    m = np.array(rows, dtype=np.int64)
    return m[:, 0], m[:, 1], m[:, 2], np.array([wigner3j(l, l, l, *r) for r in rows], dtype=LD)


def full(re, im, l):
    """the 2l+1 complex components [..., 2l+1] (index m + l) from the m >= 0 half [..., l+1]: a_-m = (-1)^m conj(a_m)"""
    a = np.asarray(re, dtype=LD).astype(CLD) + 1j * np.asarray(im, dtype=LD).astype(CLD)
    sign = np.array([(-1) ** m for m in range(l, 0, -1)], dtype=LD)
    return np.concatenate([np.conj(a[..., :0:-1]) * sign, a], axis=-1)


def cubic_general(a, l):
    """(sum_{m1+m2+m3=0} (l l l; m1 m2 m3) a_m1 a_m2 a_m3) as a complex long double, for ANY complex vector a [..., 2l+1], any l >= 0:
    without the prefactor (the odd-l property is about this sum)"""
    rows = [(m1, m2, -m1 - m2) for m1 in range(-l, l + 1) for m2 in range(-l, l + 1) if abs(m1 + m2) <= l]
    t = np.zeros(np.shape(a)[:-1], dtype=CLD)
    for m1, m2, m3 in rows:
        t = t + wigner3j(l, l, l, m1, m2, m3) * a[..., m1 + l] * a[..., m2 + l] * a[..., m3 + l]
    return t


def cubic(re, im, l):
    """T_l of the vector with the m >= 0 half (re, im) [..., l+1], long double"""
    a = full(re, im, l)
    m1, m2, m3, sym = table(l)
    t = (sym * (a[..., m1 + l] * a[..., m2 + l] * a[..., m3 + l]).real).sum(axis=-1)
    return (4 * R.PI / LD(2 * l + 1)) ** LD(1.5) * t


def shell(vectors, l):
    """(w3, q2) of one centre whose bonds are `vectors` [M][3] (any lengths), long double"""
    re, im = R.harmonics(R.unit(vectors), l)
    re, im = re.mean(axis=0), im.mean(axis=0)
    return cubic(re, im, l), R.invariant(re, im, l)


def w_hat(vectors, l):
    """Steinhardt's normalised w_l of one shell, float"""
    w3, q2 = shell(vectors, l)
    return float(w3 / q2 ** LD(1.5))


def bond_order_w(pos, box, ls, r_lo, r_hi):
    """pos[ns][n][3], box[ns] float32.  Returns a dict: w3, wbar3, q2, qbar2 long double [ns][n][nl], W3, Q2 long double [ns][nl], nnb
    int32 [ns][n]"""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    box = np.ascontiguousarray(box, dtype=np.float32).reshape(-1)
    ns, n, nl = pos.shape[0], pos.shape[1], len(ls)
    out = dict(w3=np.zeros((ns, n, nl), dtype=LD), wbar3=np.zeros((ns, n, nl), dtype=LD), W3=np.zeros((ns, nl), dtype=LD),
               q2=np.zeros((ns, n, nl), dtype=LD), qbar2=np.zeros((ns, n, nl), dtype=LD), Q2=np.zeros((ns, nl), dtype=LD),
               nnb=np.zeros((ns, n), dtype=np.int32))
    for s in range(ns):
        ent = [R.neighbours(pos[s], box[s], c, r_lo, r_hi) for c in range(n)]
        out['nnb'][s] = [len(e[1]) for e in ent]
        rows = np.concatenate([np.full(len(e[1]), c) for c, e in enumerate(ent)])
        allv = np.concatenate([e[0] for e in ent])
        un = R.unit(allv) if len(allv) else np.zeros((0, 3), dtype=LD)
        idx = np.concatenate([e[1] for e in ent])
        nb = out['nnb'][s].astype(LD)
        for i, l in enumerate(ls):
            yre, yim = R.harmonics(un, l)
            sre = np.zeros((n, l + 1), dtype=LD)
            sim = np.zeros((n, l + 1), dtype=LD)
            np.add.at(sre, rows, yre)
            np.add.at(sim, rows, yim)
            den = np.where(nb > 0, nb, 1)[:, None]
            qre, qim = sre / den, sim / den
            out['q2'][s, :, i] = R.invariant(qre, qim, l)
            out['w3'][s, :, i] = cubic(qre, qim, l)
            are, aim = qre.copy(), qim.copy()
            np.add.at(are, rows, qre[idx])
            np.add.at(aim, rows, qim[idx])
            are, aim = are / (nb + 1)[:, None], aim / (nb + 1)[:, None]
            out['qbar2'][s, :, i] = R.invariant(are, aim, l)
            out['wbar3'][s, :, i] = cubic(are, aim, l)
            tot = nb.sum()
            if tot > 0:
                gre, gim = sre.sum(axis=0) / tot, sim.sum(axis=0) / tot
                out['Q2'][s, i] = R.invariant(gre, gim, l)
                out['W3'][s, i] = cubic(gre, gim, l)
    return out


def tol(l, x, nbmax, natoms, which):
    """the derived bound on a returned cubic form whose matching square is x (array or scalar); which = 'q' / 'qbar' / 'Q'"""
    e = R.bounds(l, nbmax, natoms)[('q', 'qbar', 'Q').index(which)]
    r = np.sqrt(np.maximum(np.asarray(x, dtype=np.float64), 0.0))
    return 3 * e * r * r + 3 * e * e * r + e ** 3 + (n_terms(l) + 12) * U * (r + e) ** 3
