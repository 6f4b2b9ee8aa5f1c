"""Common neighbour analysis (include/nm_distr.h, nm_distr_cna) restated in plain numpy, one centre at a time: float32 arithmetic
by explicit casts (every operand array is float32, so numpy rounds each operation to float32), float64 sums in the stated order, a
plain sort by (d, image, atom), a set-based component search.  It shares no code with the package."""
import numpy as np

F = np.float32
FIXED, ADAPTIVE = 0, 1
OTHER, FCC, HCP, BCC, ICO = 0, 1, 2, 3, 4
COLUMNS = ((4, 2, 1), (4, 2, 2), (4, 4, 4), (6, 6, 6), (5, 5, 5), (5, 4, 4), (4, 3, 3))   # column 7 is `other`
C421, C422, C444, C666, C555, C544, C433, COTHER = range(8)
K12 = 1.2071067811865475          # (1 + sqrt 2) / 2
K14 = 1.1547005383792517          # 2 / sqrt 3
BR = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)], dtype=F)   # image-major: the scan order


def length(v):
    """float32 lengths of float32 vectors [..., 3]: the sequential sum of the three squares, the correctly rounded root"""
    v = np.asarray(v)
    assert v.dtype == F
    s = v[..., 0] * v[..., 0]
    s = s + v[..., 1] * v[..., 1]
    s = s + v[..., 2] * v[..., 2]
    assert s.dtype == F
    return np.sqrt(s)


def entries(pos, box, c, r_lo, r_hi):
    """the entries of centre c in scan order: d float32 [Nb], image [Nb], atom [Nb], v float32 [Nb][3]"""
    pos = np.asarray(pos, dtype=F)
    q = pos[c][None, :] + F(box) * BR                      # pos[c] + box*br[j], float32 [27][3]
    v = pos[None, :, :] - q[:, None, :]                    # float32 [27][natoms][3]
    d = length(v)
    keep = (r_lo < d.astype(np.float64)) & (d.astype(np.float64) <= r_hi)
    img, atom = np.nonzero(keep)                           # row-major: image-major, then atom
    return d[img, atom], img, atom, v[img, atom]


def adjacency(vecs, r_lo, rc):
    """the graph on the vertices vecs float32 [n][3]: a list of neighbour sets"""
    vecs = np.asarray(vecs, dtype=F).reshape(-1, 3)
    dw = length(vecs[None, :, :] - vecs[:, None, :]).astype(np.float64)     # w = v_m - v_k at [k][m]
    bond = (r_lo < dw) & (dw <= rc)
    assert np.array_equal(bond, bond.T)
    return [set(np.flatnonzero(row).tolist()) for row in bond]


def signature(adj, k):
    """(ncn, nb, nlc) of vertex k"""
    cn = adj[k]
    bonds = [(a, b) for a in sorted(cn) for b in sorted(adj[a] & cn) if a < b]
    comps = []                                             # the components of the bonds, as sets of vertices
    for a, b in bonds:
        touching = [s for s in comps if a in s or b in s]
        comps = [s for s in comps if not (a in s or b in s)] + [{a, b}.union(*touching)]
    nlc = max([sum(1 for a, b in bonds if a in s) for s in comps], default=0)
    return len(cn), len(bonds), nlc


def column(sig):
    return COLUMNS.index(sig) if sig in COLUMNS else COTHER


def columns(vecs, r_lo, rc):
    adj = adjacency(vecs, r_lo, rc)
    out = np.zeros(8, dtype=np.int64)
    for k in range(len(adj)):
        out[column(signature(adj, k))] += 1
    return out


def close_packed(n):
    """fcc, hcp or ico from the column counts of 12 vertices, else other"""
    if n[C421] == 12:
        return FCC
    if n[C421] == 6 and n[C422] == 6:
        return HCP
    if n[C555] == 12:
        return ICO
    return OTHER


def cutoffs(d):
    """rc12 and rc14 (None with fewer than 14) from the sorted float32 lengths"""
    s = np.float64(0.0)
    for x in d[:12]:
        s = s + np.float64(x)
    rc12 = np.float64(K12) * s / np.float64(12.0)
    if len(d) < 14:
        return float(rc12), None
    s = np.float64(0.0)
    for k, x in enumerate(d[:14]):
        s = s + (np.float64(x) * np.float64(K14) if k < 8 else np.float64(x))
    return float(rc12), float(np.float64(K12) * s / np.float64(14.0))


def centre(pos, box, c, r_lo, r_hi, mode):
    """(type, sig[8]) of centre c"""
    d, img, atom, v = entries(pos, box, c, r_lo, r_hi)
    nb = len(d)
    if mode == FIXED:
        if nb > 32:
            sig = np.zeros(8, dtype=np.int64)
            sig[COTHER] = nb
            return OTHER, sig
        sig = columns(v, r_lo, r_hi)
        if nb == 12:
            return close_packed(sig), sig
        if nb == 14 and sig[C444] == 6 and sig[C666] == 8:
            return BCC, sig
        return OTHER, sig
    if nb < 12:
        return OTHER, np.zeros(8, dtype=np.int64)
    order = sorted(range(nb), key=lambda e: (d[e], img[e], atom[e]))
    d, v = d[order], v[order]
    rc12, rc14 = cutoffs(d)
    sig12 = columns(v[:12], r_lo, rc12)
    t = close_packed(sig12)
    if t != OTHER or nb < 14:
        return t, sig12
    sig14 = columns(v[:14], r_lo, rc14)
    if sig14[C444] == 6 and sig14[C666] == 8:
        return BCC, sig14
    return OTHER, sig12


_cache = {}


def cna(pos, box, r_lo, r_hi, mode):
    """type int32 [ns][natoms], sig int32 [ns][natoms][8], ntype int32 [ns][5], nsig int32 [ns][8] of a batch; a result is
    computed once per input and handed out read-only"""
    pos = np.ascontiguousarray(pos, dtype=F)
    box = np.ascontiguousarray(box, dtype=F).reshape(-1)
    key = (pos.tobytes(), pos.shape, box.tobytes(), float(r_lo), float(r_hi), int(mode))
    if key not in _cache:
        ns, n = pos.shape[0], pos.shape[1]
        typ = np.zeros((ns, n), dtype=np.int32)
        sig = np.zeros((ns, n, 8), dtype=np.int32)
        for s in range(ns):
            for c in range(n):
                typ[s, c], sig[s, c] = centre(pos[s], box[s], c, float(r_lo), float(r_hi), mode)
        ntype = np.zeros((ns, 5), dtype=np.int32)
        for s in range(ns):
            ntype[s] = np.bincount(typ[s], minlength=5)
        res = (typ, sig, ntype, sig.sum(axis=1, dtype=np.int64).astype(np.int32))
        for a in res:
            a.setflags(write=False)
        _cache[key] = res
    return _cache[key]
