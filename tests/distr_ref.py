"""Bounded-memory reference of the structural histograms (test infrastructure): the integer counts of calculate_rdf /
calculate_cdf (lammps_distr.py:123-171) for batches of samples, before the reference's division by natoms.

It restates the arithmetic of oracle/distr_oracle.py, which holds all 27 n^2 displacements of a sample at once, in blocks of
(samples x rows b) that stay below `budget` elements: dvm[b][a] = pos[a] - (pos[b] + box*br) in float32, |d| as a sequential
float32 sum of the three squares and a float32 sqrt, and float64 comparisons against the edges with numpy's rules
(np.histogram: e[k] <= d < e[k+1], the last bin also d == e[-1]; np.histogramdd: the same per axis, outside dropped).
tests/test_distr.py proves it bit-equal to the oracle and to every key of tests/golden/ref_distr.npz."""
import numpy as np

# br, lammps_distr.py:99-102
_B = [-1, 0, 1]
BR = np.array([[_B[i], _B[j], _B[k]] for i in range(3) for j in range(3) for k in range(3)], dtype=np.int8)


def _bins(e, x):
    """bin of every float64 x inside [e[0], e[-1]] under numpy's right-edge-inclusive rule"""
    k = np.searchsorted(e, x, side='right') - 1
    k[k == len(e) - 1] = len(e) - 2                      # x == e[-1] lands in the last bin
    return k


def counts(pos, box, r=None, ve=None, budget=1 << 22):
    """pos[ns][n][3], box[ns] float32; r = rdf edges (sbins), ve = cdf edges of one axis (cbins + 1), float64, or None.
    Returns (rdf[ns][sbins] int64 with rdf[:, 0] = 0, cdf[ns][cb][cb][cb] int64), None for a histogram not asked for."""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    box = np.ascontiguousarray(box, dtype=np.float32).reshape(-1)
    ns, n = pos.shape[0], pos.shape[1]
    sb = 0 if r is None else len(r)
    cb = 0 if ve is None else len(ve) - 1
    rdf = np.zeros((ns, sb), dtype=np.int64) if r is not None else None
    cdf = np.zeros((ns, cb ** 3), dtype=np.int64) if ve is not None else None
    if r is not None:
        r = np.asarray(r, dtype=np.float64)
    if ve is not None:
        ve = np.asarray(ve, dtype=np.float64)
    rows = max(1, min(n, budget // n))                   # rows b per block
    batch = max(1, min(ns, budget // (rows * n)))        # samples per block
    for s0 in range(0, ns, batch):
        s1 = min(ns, s0 + batch)
        p = pos[s0:s1]
        for b0 in range(0, n, rows):
            q0 = p[:, b0:b0 + rows]
            sid = np.broadcast_to(np.arange(s1 - s0)[:, None, None], q0.shape[:2] + (n,))   # sample of each (b, a)
            for br in BR:
                q = q0 + (box[s0:s1, None, None] * br.reshape(1, 1, 3))      # pos[b] + box*br, float32
                dvm = p[:, None, :, :] - q[:, :, None, :]                    # [s][b][a][3], float32
                if r is not None:
                    d2 = dvm[..., 0] * dvm[..., 0]
                    d2 = d2 + dvm[..., 1] * dvm[..., 1]
                    d2 = d2 + dvm[..., 2] * dvm[..., 2]
                    d = np.sqrt(d2).astype(np.float64)
                    m = (d >= r[0]) & (d <= r[-1])
                    k = _bins(r, d[m]) + 1                                   # rd[1:] += np.histogram(d, r)[0]
                    rdf[s0:s1] += np.bincount(sid[m] * sb + k, minlength=(s1 - s0) * sb).reshape(s1 - s0, sb)
                if ve is not None:
                    v = dvm.astype(np.float64)
                    m = ((v >= ve[0]) & (v <= ve[-1])).all(-1)
                    w = v[m]
                    kx, ky, kz = _bins(ve, w[:, 0]), _bins(ve, w[:, 1]), _bins(ve, w[:, 2])
                    idx = ((sid[m] * cb + kx) * cb + ky) * cb + kz
                    cdf[s0:s1] += np.bincount(idx, minlength=(s1 - s0) * cb ** 3).reshape(s1 - s0, cb ** 3)
    return rdf, (cdf.reshape(ns, cb, cb, cb) if ve is not None else None)


def normalized(c, natoms):
    """what the reference's calculate_rdf / calculate_cdf return per sample: float32 counts / natoms (uint16),
    lammps_distr.py:135, 171"""
    na = np.asarray(natoms, dtype=np.uint16).reshape((-1,) + (1,) * (c.ndim - 1))
    return c.astype(np.float32) / na
