"""numpy restatement of nm_distr_sfactor's definition (include/nm_distr.h) in np.longdouble (x87 extended: eps 1.1e-19).

u = float64(pos) / float64(box) is the definition's float64 quotient; everything after it is long double: the products m * u
(exact: 53 + 6 bits), their reduction to [-1/2, 1/2] turns, cos and sin of 2 pi times that, the product of the three axis
factors, the sum over the atoms, |rho|^2 / N and the shell sums.  Every vector of the full sphere is evaluated (no use of
S(-q) = S(q)), in chunks over samples and vectors so that the memory stays bounded.  Its own error is about N * 1e-18,
eight orders below the tolerance tol() that the tests grant the kernel."""
import numpy as np

LD = np.longdouble
TWO_PI = LD(8) * np.arctan(LD(1))
CHUNK = 1 << 21                       # elements of the [samples, vectors, atoms] work array


def vectors(qmax):
    """all integer triples with 1 <= h^2 + k^2 + l^2 <= qmax^2: (v int64 [nv][3], n2 int64 [nv])"""
    g = np.arange(-qmax, qmax + 1, dtype=np.int64)
    v = np.stack(np.meshgrid(g, g, g, indexing='ij'), axis=-1).reshape(-1, 3)
    n2 = (v * v).sum(axis=1)
    keep = (n2 >= 1) & (n2 <= qmax * qmax)
    return v[keep], n2[keep]


def reduced(pos, box):
    """u = (double)pos / (double)box, float64 [ns][n][3]"""
    return np.asarray(pos, dtype=np.float32).astype(np.float64) / np.asarray(box, dtype=np.float32).astype(np.float64)[:, None, None]


def tol(n, qmax, umax):
    """4 N e, e = (6 pi qmax max|u| + 16) 2^-53: twice the bound |dS| <= 2 N e of include/nm_distr.h"""
    return 4.0 * n * (6.0 * np.pi * qmax * umax + 16.0) * 2.0 ** -53


def per_vector(pos, box, qmax):
    """S(hkl) of every vector of vectors(qmax): long double [ns][nv]"""
    pos = np.asarray(pos, dtype=np.float32)
    if pos.ndim == 2:
        pos, box = pos[None], [box]
    u = reduced(pos, box).astype(LD)
    ns, n = u.shape[:2]
    v, _ = vectors(qmax)
    m = np.arange(-qmax, qmax + 1).astype(LD)
    out = np.empty((ns, len(v)), dtype=LD)
    sc = max(1, min(ns, CHUNK // (n * 64)))
    for s0 in range(0, ns, sc):
        ph = m[None, :, None, None] * u[s0:s0 + sc, None]                      # [sc][2 qmax + 1][n][3] turns, exact
        ph = TWO_PI * (ph - np.rint(ph))
        e = np.cos(ph) - 1j * np.sin(ph)                                       # exp(-2 pi i m u), clongdouble
        vc = max(1, CHUNK // (e.shape[0] * n))
        for v0 in range(0, len(v), vc):
            i = v[v0:v0 + vc] + qmax
            rho = (e[..., 0][:, i[:, 0]] * e[..., 1][:, i[:, 1]] * e[..., 2][:, i[:, 2]]).sum(axis=-1)   # [sc][vc]
            out[s0:s0 + sc, v0:v0 + vc] = (rho.real * rho.real + rho.imag * rho.imag) / LD(n)
    return out


def shells(pos, box, qmax):
    """(sf_sum, sf_max) long double [ns][qmax^2 + 1] as nm_distr_sfactor defines them"""
    sv = per_vector(pos, box, qmax)
    _, n2 = vectors(qmax)
    ssum = np.zeros((sv.shape[0], qmax * qmax + 1), dtype=LD)
    smax = np.zeros_like(ssum)
    for s in range(sv.shape[0]):
        np.add.at(ssum[s], n2, sv[s])
        np.maximum.at(smax[s], n2, sv[s])
    return ssum, smax
