"""Spectral clustering's embedding in plain numpy (include/nm_distr.h, nm_cluster_spectral: the definitions): the dense affinity, the
degree with sums in long double, the operator M and numpy.linalg.eigh; the sign rule and the embedding; the largest principal angle
between two column spaces; the header's error bounds; and a restatement of the filtered iteration that is used only to predict the
order of magnitude of a pass count.  Nothing here is called by the package."""
import collections

import numpy as np

U = 2.0 ** -53
LD = np.longdouble


def d2(x, dtype=np.float64):
    """the squared distances (N, N) of x (N, ND), the coordinates added one after the other"""
    x = np.asarray(x, dtype=dtype)
    out = np.zeros((x.shape[0], x.shape[0]), dtype=dtype)
    for c in range(x.shape[1]):
        out += (x[:, c, None] - x[None, :, c]) ** 2
    return out


def affinity(x, gamma, dtype=np.float64):
    """A(i, j) = exp(-gamma d2(i, j)), A(i, i) = 0"""
    a = np.exp(-dtype(gamma) * d2(x, dtype))
    np.fill_diagonal(a, 0.0)
    return a


Dense = collections.namedtuple('Dense', 'deg deg_slack m lam vec gmax')


def dense(x, gamma):
    """deg (N,) long double; deg_slack (N,) = sum_j t_ij A_ij, the header's term of the arguments' errors; m (N, N) long double the
    operator; lam (N,) descending and vec (N, N) its eigenpairs in float64; gmax = gamma times the largest d2"""
    t = LD(gamma) * d2(x, LD)
    a = np.exp(-t)
    np.fill_diagonal(a, 0.0)
    deg = a.sum(axis=1)
    rs = 1.0 / np.sqrt(deg)
    m = a * rs[:, None] * rs[None, :]
    lam, vec = np.linalg.eigh(m.astype(np.float64))
    return Dense(deg, (t * a).sum(axis=1), m, lam[::-1].copy(), vec[:, ::-1].copy(), float(t.max()))


def deg_bound(ref, n, ndim):
    """the header's bound of |deg[i] - exact|, (N,)"""
    return U * ((ndim + 3) * ref.deg_slack + (2 * n + 2) * ref.deg).astype(np.float64)


def eps_m(ref, n, ndim):
    """the header's bound of one application of M to a unit vector"""
    return (2 * (ndim + 3) * ref.gmax + 4 * n + 16) * U


def eps_r(ref, n, ndim, nblock):
    """the header's bound of a returned residual"""
    return np.sqrt(nblock) * eps_m(ref, n, ndim) + 160 * U


def signed(embed):
    """every column with its entry of largest magnitude, the first on equal magnitudes, positive"""
    embed = np.array(embed, dtype=np.float64)
    for c in range(embed.shape[1]):
        if embed[np.argmax(np.abs(embed[:, c])), c] < 0.0:
            embed[:, c] = -embed[:, c]
    return embed


def embedding(ref, k):
    """embed (N, k) of the reference: v_c / sqrt(deg), signed"""
    return signed(ref.vec[:, :k] / np.sqrt(ref.deg.astype(np.float64))[:, None])


def sine(p, q):
    """the sine of the largest principal angle between the column spaces of p and q (N, k), of the same dimension"""
    p, q = np.linalg.qr(np.asarray(p, dtype=np.float64))[0], np.linalg.qr(np.asarray(q, dtype=np.float64))[0]
    return float(np.linalg.norm(q - p @ (p.T @ q), 2))


def residuals(ref, embed, deg, eigval):
    """||M v_c - eigval[c] v_c||_2 for v_c = embed[:, c] sqrt(deg), in long double; the v_c; and the 2-norm of the block of residuals"""
    v = np.asarray(embed, dtype=LD) * np.sqrt(np.asarray(deg, dtype=LD))[:, None]
    r = ref.m @ v - v * np.asarray(eigval, dtype=LD)[None, : v.shape[1]]
    return np.sqrt((r * r).sum(axis=0)).astype(np.float64), v.astype(np.float64), float(np.linalg.norm(r.astype(np.float64), 2))


def sines(v, space):
    """the sine of the angle between every column of v and the space of the orthonormal columns of `space`"""
    v = np.asarray(v, dtype=np.float64)
    return np.linalg.norm(v - space @ (space.T @ v), axis=0) / np.linalg.norm(v, axis=0)


def labels_agree(a, b):
    """whether two labellings are the same partition"""
    a, b = np.asarray(a), np.asarray(b)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def lloyd(x, k, seed, restarts=10):
    """k-means of x on the host, the best of `restarts` runs from points drawn without replacement: the labels"""
    rng = np.random.default_rng(seed)
    best = None
    for _ in range(restarts):
        c = x[rng.choice(x.shape[0], k, replace=False)].copy()
        for _ in range(300):
            label = ((x[:, None, :] - c[None, :, :]) ** 2).sum(axis=2).argmin(axis=1)
            new = np.stack([x[label == j].mean(axis=0) if (label == j).any() else c[j] for j in range(k)])
            if np.array_equal(new, c):
                break
            c = new
        inertia = ((x - c[label]) ** 2).sum()
        if best is None or inertia < best[0]:
            best = inertia, label
    return best[1]


def filtered(m, init, ncomp, degree, max_pass, tol):
    """the header's method on the dense operator m in float64: (passes, status, theta, resid, v).  A restatement for pass counts:
    its sums run in numpy's order, not the library's."""
    m = np.asarray(m, dtype=np.float64)
    v = np.linalg.qr(np.asarray(init, dtype=np.float64))[0]
    nb, passes, low = v.shape[1], 0, 0.0
    for rnd in range(max_pass):
        w = m @ v
        passes += 1
        h = v.T @ w
        theta, q = np.linalg.eigh(0.5 * (h + h.T))
        theta, q = theta[::-1], q[:, ::-1]
        v, w = v @ q, w @ q
        resid = np.linalg.norm(w - v * theta[None, :], axis=0)
        if resid[:ncomp].max() <= tol:
            return passes, 0, theta, resid, v
        if passes + degree > max_pass:
            return passes, 2, theta, resid, v
        if rnd == 0 or nb > ncomp:
            low = max(theta[-1], -1.0 + 2.0 ** -10)
        e, c = 0.5 * (low + 1.0), 0.5 * (low - 1.0)
        sigma1 = sigma = e / (1.0 - c)
        prev, cur = v, (sigma1 / e) * (w - c * v)
        for _ in range(2, degree + 1):
            sigma2 = 1.0 / (2.0 / sigma1 - sigma)
            prev, cur = cur, 2.0 * (sigma2 / e) * (m @ cur - c * cur) - sigma * sigma2 * prev
            passes += 1
            sigma = sigma2
        v = np.linalg.qr(cur)[0]
    raise AssertionError('unreachable')
