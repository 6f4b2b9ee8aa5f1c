"""Restatements of include/nm_cluster.h and include/nm_tsne.h that do not cost N^2, for tests at the sizes where a workgroup of the
all-pairs scans walks several tiles: plain numpy and scipy's KD-tree, nothing shared with the kernels and nothing imported from the
package.  tests/cluster_ref.py and tests/tsne_ref.py stay the definitions; tests/test_scan_big.py holds these equal to them at the
sizes the dense ones reach.

The KD-tree only proposes candidate pairs.  Every decision is taken on d2 recomputed here in float64, c ascending, every product and
sum rounded on its own.  dbscan_kd is fed data on a dyadic grid only, where that d2 is exact and so is the kernels' (whose fused
multiply-add then rounds nothing); neighbours_kd states include/nm_tsne.h's order of operations."""
import numpy as np
from scipy.sparse import coo_matrix
from scipy.sparse.csgraph import connected_components
from scipy.spatial import cKDTree


def d2_pairs(x, i, j):
    """d2 of the pairs (i, j): sum_c (x[i][c] - x[j][c])^2, c ascending; i and j broadcast against each other"""
    acc = None
    for c in range(x.shape[1]):
        d = x[i, c] - x[j, c]
        acc = d * d if acc is None else acc + d * d
    return acc


def dbscan_kd(x, eps, min_pts):
    """(label (N,) int32, degree (N,) int32, nclusters) by the rules of include/nm_cluster.h"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = x.shape[0]
    e2 = float(eps) * float(eps)
    pairs = cKDTree(x).query_pairs(float(eps) * (1.0 + 2.0 ** -20), output_type='ndarray')         # i < j, a little beyond the bound
    i, j = pairs[:, 0], pairs[:, 1]
    near = d2_pairs(x, i, j) <= e2
    i, j = i[near], j[near]
    degree = (1 + np.bincount(i, minlength=n) + np.bincount(j, minlength=n)).astype(np.int32)      # the point itself among them
    core = degree >= min_pts
    both = core[i] & core[j]
    graph = coo_matrix((np.ones(int(both.sum()), dtype=np.int8), (i[both], j[both])), shape=(n, n))
    comp = connected_components(graph, directed=False)[1]
    label = np.full(n, -1, dtype=np.int32)
    cores = np.nonzero(core)[0]                                 # ascending: a component is numbered at its smallest core index
    seen, first = np.unique(comp[cores], return_index=True)
    number = np.full(n, -1, dtype=np.int64)                     # by component
    number[seen[np.argsort(first)]] = np.arange(seen.size)
    label[cores] = number[comp[cores]]
    # a border takes the lowest number among its core neighbours; either end of a pair may be the border
    big = np.iinfo(np.int32).max
    best = np.full(n, big, dtype=np.int64)
    for a, b in ((i, j), (j, i)):
        m = ~core[a] & core[b]
        np.minimum.at(best, a[m], label[b[m]])
    border = ~core & (best < big)
    label[border] = best[border]
    return label, degree, int(seen.size)


def candidates(x, m):
    """of every row its m nearest points as the tree returns them, sorted by (d2, index) with the row itself in front (its d2 is
    given as -1): (cand (N, m), d2 (N, m), found (N,) whether the row itself was among them)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    n = x.shape[0]
    cand = cKDTree(x).query(x, m)[1].reshape(n, m).astype(np.int64)
    rows = np.arange(n)[:, None]
    d2 = d2_pairs(x, rows, cand)
    own = cand == rows
    d2[own] = -1.0
    order = np.lexsort((cand, d2), axis=1)
    return np.take_along_axis(cand, order, axis=1), np.take_along_axis(d2, order, axis=1), own.any(axis=1)


def neighbours_kd(x, k, extra=24):
    """(nbr (N, k) int32, complete (N,) bool, tied (N,) bool): of every row the k points j != i with the smallest (d2, j), in that
    order, chosen among the k + 1 + extra nearest that the tree returns.  complete[i] says that the row's last candidate lies strictly
    farther than its k-th neighbour, so no point outside the candidates can tie with or precede one inside the list.  A caller may
    use nbr only where complete holds for every row.  tied[i]: the k-th and the next candidate lie at one distance (the index
    decided)."""
    n = np.shape(x)[0]
    m = min(n, k + 1 + extra)
    cand, d2, found = candidates(x, m)
    nbr = np.ascontiguousarray(cand[:, 1:k + 1], dtype=np.int32)
    complete = found & ((d2[:, -1] > d2[:, k]) | (m == n))
    tied = d2[:, k] == d2[:, k + 1] if m > k + 1 else np.zeros(n, dtype=bool)
    return nbr, complete, tied


def symmetric(nbr, p):
    """the symmetric affinities as (row, column, P_ij) over the pairs listed in either direction: (p_{j|i} + p_{i|j}) / (2 N)"""
    n, k = nbr.shape
    cond = coo_matrix((np.asarray(p, dtype=np.float64).ravel(), (np.repeat(np.arange(n), k), np.asarray(nbr, dtype=np.int64).ravel())),
                      shape=(n, n)).tocsr()
    both = (cond + cond.T).tocoo()
    return both.row.astype(np.int64), both.col.astype(np.int64), both.data / (2.0 * n)


def gradient_grouped(nbr, p, centres, member, exaggeration=1.0):
    """tests/tsne_ref.py's gradient (grad, kl, Z, mag, klmag) for the embedding y = centres[member]: the repulsive sums and Z run
    over the m distinct locations weighted by how many points lie at each, the attractive sums and kl over the symmetric lists.
    A point's own term has w = 1 and no direction: it is part of its location's row sum and is taken out of Z there."""
    centres = np.asarray(centres, dtype=np.float64)
    member = np.asarray(member, dtype=np.int64)
    n, nc = member.size, centres.shape[1]
    m = centres.shape[0]
    mult = np.bincount(member, minlength=m).astype(np.float64)
    diff = centres[:, None, :] - centres[None, :, :]            # (m, m, nc)
    d2 = None
    for c in range(nc):
        d2 = diff[..., c] * diff[..., c] if d2 is None else d2 + diff[..., c] * diff[..., c]
    w = 1.0 / (1.0 + d2)
    zrow = (w * mult[None, :]).sum(axis=1) - 1.0               # of one point at the location: every other point
    z = float((zrow * mult).sum())
    ww = (w * w * mult[None, :])[..., None]
    rep, repmag = (ww * diff).sum(axis=1), (ww * np.abs(diff)).sum(axis=1)      # (m, nc)
    y = centres[member]
    i, j, pij = symmetric(nbr, p)
    dy = y[i] - y[j]
    wy = 1.0 / (1.0 + d2_pairs(y, i, j))
    att, attmag = np.empty((n, nc)), np.empty((n, nc))
    for c in range(nc):
        att[:, c] = np.bincount(i, weights=pij * wy * dy[:, c], minlength=n)
        attmag[:, c] = np.bincount(i, weights=pij * wy * np.abs(dy[:, c]), minlength=n)
    grad = 4.0 * (exaggeration * att - rep[member] / z)
    mag = 4.0 * (exaggeration * attmag + repmag[member] / z)
    pos = pij > 0.0
    kl = float((pij[pos] * np.log(pij[pos] * z / wy[pos])).sum())
    klmag = float((pij[pos] * (np.abs(np.log(pij[pos])) + np.abs(np.log(wy[pos])) + abs(np.log(z)))).sum())
    return grad, kl, z, mag, klmag
