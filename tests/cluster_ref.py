"""A plain numpy restatement of include/nm_cluster.h, for tests: the dense matrix of squared distances, a sequential union-find
and the header's rules, nothing shared with the kernels.  For a few thousand points."""
import numpy as np


def d2_matrix(x):
    """d2[i][j] = sum_c (x[i][c] - x[j][c])^2 in float64, c ascending"""
    x = np.asarray(x, dtype=np.float64)
    d2 = np.zeros((x.shape[0], x.shape[0]))
    for c in range(x.shape[1]):
        d = x[:, None, c] - x[None, :, c]
        d2 += d * d
    return d2


def margin(x, eps):
    """the smallest |d2 - eps^2| / eps^2 over all pairs: how far the nearest pair is from changing sides"""
    e2 = float(eps) * float(eps)
    return float(np.abs(d2_matrix(x) - e2).min() / e2)


def _find(parent, a):
    while parent[a] != a:
        parent[a] = parent[parent[a]]
        a = parent[a]
    return a


def dbscan(x, eps, min_pts):
    """(label (N,) int32, degree (N,) int32, nclusters) by the header's definitions"""
    near = d2_matrix(x) <= float(eps) * float(eps)
    n = near.shape[0]
    degree = near.sum(axis=1).astype(np.int32)
    core = degree >= min_pts
    parent = list(range(n))
    for i in np.nonzero(core)[0]:
        for j in np.nonzero(near[i, :i] & core[:i])[0]:         # near is symmetric: every edge once, from its larger end
            a, b = _find(parent, int(i)), _find(parent, int(j))
            if a != b:
                parent[max(a, b)] = min(a, b)
    label = np.full(n, -1, dtype=np.int32)
    number = {}
    for i in np.nonzero(core)[0]:                   # ascending: a component is numbered at its smallest core index
        label[i] = number.setdefault(_find(parent, int(i)), len(number))
    for i in np.nonzero(~core)[0]:
        mine = label[near[i] & core]
        if mine.size:
            label[i] = mine.min()
    return label, degree, len(number)
