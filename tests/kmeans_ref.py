"""A plain numpy restatement of the k-means definitions of include/nm_distr.h (nm_cluster_kmeans), for tests: the dense matrix of
squared distances of a pass, numpy's own sums, nothing shared with the kernels.  For a few ten thousand points."""
import collections

import numpy as np

Run = collections.namedtuple('Run', 'label centre count inertia iters status margin empties shifts')


def d2_matrix(x, centre):
    """d2[i][j] = sum_c (x[i][c] - centre[j][c])^2 in float64, c ascending"""
    d2 = np.zeros((x.shape[0], centre.shape[0]))
    for c in range(x.shape[1]):
        d = x[:, None, c] - centre[None, :, c]
        d2 += d * d
    return d2


def assign(x, centre):
    """(labels: the nearest centre, the lowest index on equal bits; their d2; the smallest relative gap (second - best) / second of
    any point's two nearest centres: 0 where a point has a tie, inf with one centre)"""
    d2 = d2_matrix(x, centre)
    label = d2.argmin(axis=1)                                   # numpy's argmin returns the first of equal minima
    best = d2[np.arange(x.shape[0]), label]
    if centre.shape[0] == 1:
        return label.astype(np.int32), best, np.inf
    second = np.partition(d2, 1, axis=1)[:, 1]
    gap = np.where(second > 0.0, (second - best) / np.where(second > 0.0, second, 1.0), 0.0)
    return label.astype(np.int32), best, float(gap.min())


def update(x, label, centre):
    """(the members' means, a cluster without members keeping its centre; the counts)"""
    count = np.bincount(label, minlength=centre.shape[0]).astype(np.int32)
    new = centre.copy()
    for j in np.nonzero(count)[0]:
        new[j] = x[label == j].sum(axis=0) / count[j]
    return new, count


def lloyd(x, init, max_iter, tol):
    """one restart by the header's steps: Run(label, centre, count, inertia, iters, status; margin, the smallest gap over all its
    assignment passes; empties, the passes that left a cluster without members; shifts, the shift of every update)"""
    x, centre = np.ascontiguousarray(x, dtype=np.float64), np.array(init, dtype=np.float64)
    margin, empties, shifts, before = np.inf, 0, [], None
    for t in range(1, max_iter + 1):
        label, near, gap = assign(x, centre)
        margin = min(margin, gap)
        empties += int(np.bincount(label, minlength=centre.shape[0]).min() == 0)
        if t > 1 and np.array_equal(label, before):
            status, iters = 0, t - 1
            break
        before = label
        new, _ = update(x, label, centre)
        shift = 0.0
        for d in (new - centre).reshape(-1):                    # j then c ascending
            shift += d * d
        shifts.append(shift)
        centre = new
        if shift <= tol or t == max_iter:
            status, iters = (1 if shift <= tol else 2), t
            label, near, gap = assign(x, centre)                # the result is the assignment against the returned centres
            margin = min(margin, gap)
            empties += int(np.bincount(label, minlength=centre.shape[0]).min() == 0)
            break
    count = np.bincount(label, minlength=centre.shape[0]).astype(np.int32)
    return Run(label, centre, count, float(near.sum()), iters, status, margin, empties, shifts)
