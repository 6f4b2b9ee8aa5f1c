"""Bounded-memory numpy restatement of the angular distribution of include/nm_distr.h (test infrastructure): the integer
counts nm_distr_angles returns, one centre atom at a time.

Per sample s and centre c: v = pos[a] - (pos[c] + box*br[j]) in float32 over the 27 image shifts br (the order of
lammps_distr.py:99-102), d = float32 sqrt of the sequential float32 sum of the three squares, neighbours are the (j, a)
with r_lo < float64(d) <= r_hi.  For every unordered pair of distinct neighbours, in float64 from the float32 components:
n_i = (x_i*x_i + y_i*y_i) + z_i*z_i, dot = (x1*x2 + y1*y2) + z1*z2, cth = clip(dot / sqrt(n1*n2), -1, 1).  Bin k holds
cos_edges[k] >= cth > cos_edges[k+1] (the last bin also cth == cos_edges[-1]), outside is dropped, adf[s][k+1] += 1."""
import numpy as np

from distr_ref import BR


def neighbours(pos, box, c, r_lo, r_hi):
    """float32 displacement vectors [M][3] of the neighbours of centre c in one sample, image-major"""
    pos = np.asarray(pos, dtype=np.float32)
    q = pos[c][None, :] + np.float32(box) * BR.astype(np.float32)            # pos[c] + box*br[j], [27][3] float32
    v = pos[None, :, :] - q[:, None, :]                                      # [27][n][3] float32
    d2 = v[..., 0] * v[..., 0]
    d2 = d2 + v[..., 1] * v[..., 1]
    d2 = d2 + v[..., 2] * v[..., 2]
    d = np.sqrt(d2).astype(np.float64)
    return v[(d > r_lo) & (d <= r_hi)]


def cosines(v, rows=None):
    """cth of every unordered pair of the rows of v (float32 [M][3]), as a flat float64 array, in blocks of `rows` rows"""
    w = v.astype(np.float64)
    m = len(w)
    n = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
    rows = rows or max(1, (1 << 21) // max(m, 1))
    out = []
    for i0 in range(0, m, rows):
        a = w[i0:i0 + rows]
        dot = (a[:, None, 0] * w[None, :, 0] + a[:, None, 1] * w[None, :, 1]) + a[:, None, 2] * w[None, :, 2]
        with np.errstate(invalid='ignore', divide='ignore'):
            cth = np.clip(dot / np.sqrt(n[i0:i0 + rows, None] * n[None, :]), -1.0, 1.0)
        keep = np.arange(m)[None, :] > np.arange(i0, i0 + len(a))[:, None]   # j > i: each unordered pair once
        out.append(cth[keep])
    return np.concatenate(out) if out else np.zeros(0)


def cos_bins(cos_edges, cth):
    """bin index of every cth under the cosine-table rule, -1 = dropped"""
    neg = -np.asarray(cos_edges, dtype=np.float64)                           # increasing; -e[k] <= -c < -e[k+1]
    k = np.searchsorted(neg, -cth, side='right') - 1
    k[(k == len(neg) - 1) & (-cth == neg[-1])] = len(neg) - 2                # cth == cos_edges[-1] lands in the last bin
    k[k == len(neg) - 1] = -1
    return k


def counts(pos, box, cos_edges, r_lo, r_hi, angle_edges=None):
    """pos[ns][n][3], box[ns] float32.  Returns (adf[ns][abins] int64 with adf[:, 0] = 0, triplets[ns] int64: the number of
    unordered neighbour pairs summed over the centres).  With angle_edges (the `a` of calculate_spatial) the bins are
    np.histogram(np.arccos(cth), a) instead of the cosine table: the variant the cosine table is checked against."""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    box = np.ascontiguousarray(box, dtype=np.float32).reshape(-1)
    ns, n = pos.shape[0], pos.shape[1]
    nb = len(cos_edges)
    adf = np.zeros((ns, nb), dtype=np.int64)
    trip = np.zeros(ns, dtype=np.int64)
    for s in range(ns):
        for c in range(n):
            v = neighbours(pos[s], box[s], c, r_lo, r_hi)
            m = len(v)
            trip[s] += m * (m - 1) // 2
            if m < 2:
                continue
            cth = cosines(v)
            if angle_edges is not None:
                adf[s, 1:] += np.histogram(np.arccos(cth), angle_edges)[0]
            else:
                k = cos_bins(cos_edges, cth)
                adf[s, 1:] += np.bincount(k[k >= 0], minlength=nb - 1)
    return adf, trip


def angle_domain(sbins):
    """the angular domain of calculate_spatial (lammps_distr.py:88) and its cosine table"""
    a = np.linspace(1e-16, np.pi, sbins)
    return a, np.cos(a)
