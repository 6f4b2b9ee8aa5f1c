"""The definitions of nm_distr_lof (include/nm_distr.h) restated in numpy, for one set: the distance in the header's order of
operations (a loop over the coordinates, every difference, product and sum an array operation of its own: no einsum, no matrix
product), the lexicographic (d2, j) selection, and every sum in list order."""
import numpy as np

FLOOR = 1e-10           # sklearn's, added to the mean reach
U = 2.0 ** -53


def d2(x):
    """(n, n) squared distances of x (n, ndim), c ascending"""
    x = np.asarray(x, dtype=np.float64)
    d = x[:, None, 0] - x[None, :, 0]
    acc = d * d
    for c in range(1, x.shape[1]):
        d = x[:, None, c] - x[None, :, c]
        acc = acc + d * d
    return acc


def neighbours(x, k):
    """(nbr (n, k) int32, their d2 (n, k)): the k points j != i with the smallest (d2(i, j), j), in that order"""
    dd = d2(x)
    n = dd.shape[0]
    j = np.arange(n - 1)[None, :] + (np.arange(n - 1)[None, :] >= np.arange(n)[:, None])      # row i: every j != i, ascending
    order = np.argsort(np.take_along_axis(dd, j, axis=1), axis=1, kind='stable')[:, :k]       # stable: equal d2 stay in ascending j
    nbr = np.take_along_axis(j, order, axis=1)
    return nbr.astype(np.int32), np.take_along_axis(dd, nbr, axis=1)


def lof(x, k):
    """(lof (n,), lrd (n,), kdist (n,), nbr (n, k) int32) of one set x (n, ndim)"""
    nbr, dd = neighbours(x, k)
    dist = np.sqrt(dd)
    kdist = dist[:, k - 1].copy()
    total = np.zeros(dist.shape[0])
    for m in range(k):
        total = total + np.maximum(dist[:, m], kdist[nbr[:, m]])
    lrd = 1.0 / (total / float(k) + FLOOR)
    total = np.zeros(dist.shape[0])
    for m in range(k):
        total = total + lrd[nbr[:, m]] / lrd
    return total / float(k), lrd, kdist, nbr


def batch(x, k):
    """lof of every set of x (nsets, npts, ndim): (lof, lrd, kdist (nsets, npts), nbr (nsets, npts, k))"""
    parts = [lof(s, k) for s in np.asarray(x, dtype=np.float64)]
    return tuple(np.stack([p[q] for p in parts]) for q in range(4))


def bounds(ndim, k):
    """the header's relative bounds of (lof, lrd, kdist)"""
    return (ndim + 3 * k + 16) * U, (ndim / 2 + k + 8) * U, (ndim / 2 + 3) * U
