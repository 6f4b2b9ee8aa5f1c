"""numpy restatement of nm_distr_solid's definition (include/nm_distr.h) on top of tests/bondorder_ref.py (test infrastructure).

The neighbour entries, the unit vectors and the harmonics are bondorder_ref's (float32 entry test, everything after it in
np.longdouble); the moments q_lm(c), the norms, the bond values s(c, a) and the connections follow in long double; the clusters
come from a plain union-find over the undirected edges between solid-like atoms.

Every entry also gets a margin: the moments of the kernel are off by at most e_q (bondorder_ref.bounds, relative to the norm of the
harmonics' vector) per vector, so the normalised dot product of two of them is off by at most about e_q / |q(c)| + e_q / |q(a)|; the
margin is 4 (e_q / |q(c)| + e_q / |q(a)|) + 16 u, the factor 4 covering the harmonics' norm sqrt((2l + 1) / 4 pi) <= 1.42 and the
restatement's own error, the 16 u the kernel's dot product, norms, roots and division.  An entry is `decided` where its value lies
further than the margin from s_min: there the kernel's comparison must agree with the restatement's, and all five outputs are
integers that can be compared exactly."""
import numpy as np

import bondorder_ref as R

LD = R.LD
U = R.U


def decided(s, margin, s_min):
    """true where the comparison s > s_min cannot depend on the rounding errors of s"""
    return np.abs(np.asarray(s, dtype=LD) - LD(s_min)) > np.asarray(margin)


def clusters(n, solid, rows, idx):
    """label int64 [n] of one sample: the smallest index of the atom's component in the undirected graph with the edges
    {rows[k], idx[k]} between solid-like atoms, -1 for an atom that is not solid-like.  Plain union-find."""
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for c, a in zip(rows.tolist(), idx.tolist()):
        if solid[c] and solid[a]:
            rc, ra = find(c), find(a)
            if rc != ra:
                parent[max(rc, ra)] = min(rc, ra)
    return np.array([find(c) if solid[c] else -1 for c in range(n)], dtype=np.int64)


def entries(pos, box, r_lo, r_hi):
    """the neighbour entries of a batch: (v float32 [E][3], sample [E], centre [E], atom [E], nnb int [ns][n]), centre-major per sample"""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    box = np.ascontiguousarray(box, dtype=np.float32).reshape(-1)
    ns, n = pos.shape[0], pos.shape[1]
    vs, ss, cs, ats = [np.zeros((0, 3), dtype=np.float32)], [], [], []
    nnb = np.zeros((ns, n), dtype=np.int64)
    for s in range(ns):
        for c in range(n):
            v, a = R.neighbours(pos[s], box[s], c, r_lo, r_hi)
            nnb[s, c] = len(a)
            if len(a):
                vs.append(v)
                ss.append(np.full(len(a), s))
                cs.append(np.full(len(a), c))
                ats.append(a)
    cat = lambda x: np.concatenate(x).astype(np.int64) if x else np.zeros(0, dtype=np.int64)
    return np.concatenate(vs), cat(ss), cat(cs), cat(ats), nnb


def bonds(pos, box, l, r_lo, r_hi):
    """pos[ns][n][3], box[ns] float32.  What does not depend on s_min and n_min, as a dict: per entry (centre-major per sample) sample,
    centre, atom, s (long double) and margin (float64); nnb [ns][n]; ns, n"""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    ns, n = pos.shape[0], pos.shape[1]
    v, es, ec, ea, nnb = entries(pos, box, r_lo, r_hi)
    row, col = es * n + ec, es * n + ea
    qre = np.zeros((ns * n, l + 1), dtype=LD)
    qim = np.zeros((ns * n, l + 1), dtype=LD)
    if len(v):
        yre, yim = R.harmonics(R.unit(v), l)
        np.add.at(qre, row, yre)
        np.add.at(qim, row, yim)
    nb = nnb.reshape(-1).astype(LD)
    den = np.where(nb > 0, nb, 1)[:, None]
    qre, qim = qre / den, qim / den                                           # q_lm(c), 0 where Nb = 0
    w = np.ones(l + 1, dtype=LD)
    w[1:] = 2
    norm = np.sqrt(((qre * qre + qim * qim) * w).sum(axis=1))                 # |q(c)|
    dot = ((qre[row] * qre[col] + qim[row] * qim[col]) * w).sum(axis=1)
    prod = norm[row] * norm[col]
    s = np.where(prod > 0, dot / np.where(prod > 0, prod, 1), LD(0))
    eq = R.bounds(l, int(nnb.max()) if nnb.size else 0, n)[0]
    # e_q / |q|; an atom without entries has q = 0 exactly, here and in the kernel; a vanishing norm with entries decides nothing
    rel = np.where(norm > 0, eq / np.where(norm > 0, norm, 1).astype(np.float64), np.where(nb > 0, np.inf, 0.0)).astype(np.float64)
    margin = 4 * (rel[row] + rel[col]) + 16 * U
    return dict(sample=es, centre=ec, atom=ea, s=s, margin=margin, nnb=nnb, ns=ns, n=n)


def classify(b, s_min, n_min):
    """the five outputs from bonds(): nconn, label int32 [ns][n]; nsolid, nclus, largest int32 [ns]; the entries are passed on"""
    ns, n, es, ec, ea = b['ns'], b['n'], b['sample'], b['centre'], b['atom']
    conn = b['s'] > LD(s_min)
    nconn = np.bincount((es * n + ec)[conn], minlength=ns * n).reshape(ns, n).astype(np.int32)
    is_solid = nconn >= n_min
    label = np.full((ns, n), -1, dtype=np.int32)
    nsolid = np.zeros(ns, dtype=np.int32)
    nclus = np.zeros(ns, dtype=np.int32)
    largest = np.zeros(ns, dtype=np.int32)
    first = np.searchsorted(es, np.arange(ns + 1))                            # the entries are sorted by sample
    for k in range(ns):
        sel = slice(first[k], first[k + 1])
        label[k] = clusters(n, is_solid[k], ec[sel], ea[sel])
        sizes = np.bincount(label[k][label[k] >= 0], minlength=1)
        nsolid[k], nclus[k], largest[k] = is_solid[k].sum(), (sizes > 0).sum(), sizes.max()
    out = dict(b)
    out.update(nconn=nconn, label=label, nsolid=nsolid, nclus=nclus, largest=largest)
    return out


def solid(pos, box, l, r_lo, r_hi, s_min, n_min):
    """classify(bonds(...)): the five outputs and the entries with their values and margins"""
    return classify(bonds(pos, box, l, r_lo, r_hi), s_min, n_min)


def undecided(ref, s_min):
    """the number of entries whose connection the rounding errors could flip"""
    return int((~decided(ref['s'], ref['margin'], s_min)).sum())
