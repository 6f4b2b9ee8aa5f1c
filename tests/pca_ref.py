"""A numpy restatement of the principal component stage (include/nm_pca.h, neuralmelting_amd/pca.py): the moments and the
projections in np.longdouble, the host pipeline (scalers, eigh, ordering, sign rule) in float64, and the header's error bounds."""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
TILE, KC, SL, SLICES, BATCH, MCH = 64, 16, 4096, 8, 32768, 1024     # csrc/nm_pca.h


def gamma(k):
    return LD(k) * U / (1 - LD(k) * U)


def mean(x):
    return LD(x).sum(axis=0) / x.shape[0]


def gram(x, m):
    """sum_n a a^T in longdouble, a = x - m taken in FLOAT64 as the definition says (m: the mean the device returned)"""
    a = LD(np.asarray(x, dtype=np.float64) - np.asarray(m, dtype=np.float64))
    return a.T @ a, np.abs(a).T @ np.abs(a)


def mean_bound(x):
    n = x.shape[0]
    k = min(n - 1, 258 + -(-n // MCH)) + 1
    return gamma(k) * np.abs(LD(x)).sum(axis=0) / n


def gram_bound(n, absgram):
    m = min(n, -(-n // BATCH) * SL)
    return gamma(m + min(SLICES, -(-n // SL)) + 1) * absgram


def project(x, m, inv, comp):
    """(z, norm2, sum_j |y comp|) in longdouble from the float64 y = (x - m) * inv that the definition names"""
    y = LD(np.asarray(x, dtype=np.float64)) - LD(m)
    y = y * LD(inv)
    c = LD(np.atleast_2d(comp))
    return y @ c.T, (y * y).sum(axis=1), np.abs(y) @ np.abs(c).T


def z_bound(d, absz):
    return gamma(min(d, -(-d // 64) + 6) + 2) * absz


def norm2_bound(d, norm2):
    return gamma(min(d, -(-d // 64) + 6) + 4) * norm2


def scales(scaler, lo, hi, g, n):
    d = len(lo)
    if scaler == 'none':
        return np.ones(d)
    if scaler == 'global':
        return np.full(d, float(np.max(hi) - np.min(lo)))
    if scaler == 'standard':
        s = np.array([np.sqrt(g[j, j] / n) for j in range(d)])
    else:
        s = np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64)
    s[s == 0.0] = 1.0
    return s


def fit(lo, hi, g, n, scaler, ld):
    """(s, comp (ld, D), eigenvalues (ld,), shares (ld,)): eigenvalues descending, negative ones 0, signs as eigh left them"""
    g = np.asarray(g, dtype=np.float64)
    s = scales(scaler, lo, hi, g, n)
    cov = g / np.outer(s, s) / (n - 1)
    w, v = np.linalg.eigh(cov)
    order = np.argsort(-w, kind='stable')
    w, v = w[order], v[:, order]
    w = np.where(w < 0.0, 0.0, w)
    tot = w.sum()
    return s, v[:, :ld].T.copy(), w[:ld], (w[:ld] / tot if tot > 0 else np.zeros(ld))


def orient(comp, zgrid, T):
    """the signs: zgrid (PN, TN, SN, ld) are the projections on comp as it stands"""
    hot, cold = zgrid[:, np.argmax(T)], zgrid[:, np.argmin(T)]
    sign = np.ones(comp.shape[0])
    for c in range(comp.shape[0]):
        h, k = hot[..., c].mean(), cold[..., c].mean()
        if h < k:
            sign[c] = -1.0
        elif h == k:
            big = np.abs(comp[c]).max()
            first = [j for j in range(comp.shape[1]) if abs(comp[c, j]) == big][0]
            sign[c] = -1.0 if comp[c, first] < 0 else 1.0
    return sign


def pipeline(feat, T, scaler, ld, skip=0, stride=1):
    """the whole stage on feat (PN, TN, SN, ...) in longdouble moments and float64 host arithmetic: dict keyed by suffix"""
    pn, tn, sn = feat.shape[:3]
    x = np.asarray(feat, dtype=np.float32).reshape(pn, tn, sn, -1)
    d = x.shape[-1]
    xf = x[:, :, skip::stride].reshape(-1, d)
    n = xf.shape[0]
    m = np.asarray(mean(xf), dtype=np.float64)
    g = np.asarray(gram(xf, m)[0], dtype=np.float64)
    lo, hi = xf.min(axis=0).astype(np.float64), xf.max(axis=0).astype(np.float64)
    s, comp, w, share = fit(lo, hi, g, n, scaler, ld)
    z, norm2, _ = project(x.reshape(-1, d), m, 1.0 / s, comp)
    z = np.asarray(z, dtype=np.float64).reshape(pn, tn, sn, ld)
    sign = orient(comp, z, T)
    comp, z = comp * sign[:, None], z * sign
    pcr = np.asarray(norm2, dtype=np.float64).reshape(pn, tn, sn) - (z * z).sum(axis=-1)
    return dict(pcm=m, pcs=s, pcc=comp, pcv=np.stack([w, share]), pcz=z, pcr=pcr, n=n)
