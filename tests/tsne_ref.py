"""A plain numpy restatement of include/nm_tsne.h, for tests: dense, O(N^2), one row at a time, on tests/cluster_ref.py's matrix of
squared distances; nothing shared with the kernels.  For about a thousand points."""
import numpy as np

from cluster_ref import d2_matrix

STEPS = 200


def neighbours(d2, k):
    """nbr (N, k) int32: of every row the k columns j != i with the smallest (d2, j), in that order"""
    n = d2.shape[0]
    nbr = np.empty((n, k), dtype=np.int32)
    for i in range(n):
        order = np.lexsort((np.arange(n), d2[i]))                     # by d2, then by index
        nbr[i] = order[order != i][:k]
    return nbr


def entropy(t, beta):
    """(H, p, S) of one row at beta: t = d - dmin >= 0"""
    e = np.exp(-(beta * t))
    s = e.sum()
    return float(np.log(s) + beta * ((t * e).sum() / s)), e / s, float(s)


def search(t, logpx):
    """the header's bracketing on one row: the last iterate formed"""
    beta, lo, hi = 1.0, -np.inf, np.inf
    for _ in range(STEPS):
        h = entropy(t, beta)[0]
        if h == logpx:
            break
        if h > logpx:
            lo = beta
            nb = beta * 2.0 if hi == np.inf else (beta + hi) / 2.0
        else:
            hi = beta
            nb = beta / 2.0 if lo == -np.inf else (beta + lo) / 2.0
        if nb == beta:
            break
        beta = nb
    return beta


def affinities(x, perplexity, k):
    """(nbr (N, k) int32, p (N, k), beta (N,), d (N, k) the rows' squared distances)"""
    d2 = d2_matrix(x)
    nbr = neighbours(d2, k)
    d = np.take_along_axis(d2, nbr.astype(np.int64), axis=1)
    p, beta = np.empty_like(d), np.empty(d.shape[0])
    with np.errstate(over='ignore', under='ignore'):
        for i in range(d.shape[0]):
            t = d[i] - d[i, 0]
            beta[i] = search(t, np.log(perplexity))
            p[i] = entropy(t, beta[i])[1]
    return nbr, p, beta, d


def dense(nbr, p):
    """P (N, N): (p_{j|i} + p_{i|j}) / (2 N), 0 where neither direction is listed"""
    n = nbr.shape[0]
    cond = np.zeros((n, n))
    for i in range(n):
        cond[i, nbr[i]] = p[i]
    return (cond + cond.T) / (2.0 * n)


def gradient(nbr, p, y, exaggeration=1.0):
    """(grad (N, NC), kl, Z, mag (N, NC), klmag): the header's quantities, the sum of the magnitudes of the terms of every component
    of the gradient, and of kl's"""
    y = np.asarray(y, dtype=np.float64)
    n, nc = y.shape
    P = dense(nbr, p)
    w = 1.0 / (1.0 + d2_matrix(y))
    off = w.copy()
    np.fill_diagonal(off, 0.0)
    z = float(off.sum())
    grad, mag = np.empty((n, nc)), np.empty((n, nc))
    for i in range(n):
        diff = y[i][None, :] - y                                      # (N, NC)
        grad[i] = 4.0 * (((exaggeration * P[i] - w[i] / z) * w[i])[:, None] * diff).sum(axis=0)
        mag[i] = 4.0 * (((exaggeration * P[i] + w[i] / z) * w[i])[:, None] * np.abs(diff)).sum(axis=0)
    m = P > 0.0
    kl = float((P[m] * np.log(P[m] * z / w[m])).sum())
    klmag = float((P[m] * (np.abs(np.log(P[m])) + np.abs(np.log(w[m])) + abs(np.log(z)))).sum())
    return grad, kl, z, mag, klmag


def update_step(y, update, gains, g, momentum, learning_rate):
    """the header's update, in place"""
    inc = update * g < 0.0
    gains[inc] += 0.2
    gains[~inc] *= 0.8
    np.maximum(gains, 0.01, out=gains)
    update[:] = momentum * update - learning_rate * (g * gains)
    y += update


def descend(nbr, p, y, update, gains, niter, exaggeration, momentum, learning_rate):
    """niter steps in place: the trace (niter, 3)"""
    trace = np.empty((niter, 3))
    for s in range(niter):
        g, kl, z = gradient(nbr, p, y, exaggeration)[:3]
        trace[s] = kl, z, np.sqrt((g * g).sum())
        update_step(y, update, gains, g, momentum, learning_rate)
    return trace
