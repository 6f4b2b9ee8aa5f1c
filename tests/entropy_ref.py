"""numpy restatement of nm_distr_entropy's definition (include/nm_distr.h), one centre atom at a time (test infrastructure).

Entries in float32 exactly as tests/bondorder_ref.py selects them (image-major, the order of lammps_distr.py:99-102) with r_lo = 0,
the float32 length d and the atom index kept.  The grid D = r_m / nbins, r_k = k * D is float64, as the definition says; everything
after that in np.longdouble (x87 extended: eps 1.1e-19): the density, the exponentials, the sums, the logarithms, the trapezoid
rule, the averages.  No term is taken out.

bounds() is the error bound derived at the kernels (neuralmelting_amd/csrc/nm_distr.h), u = 2^-53, E = 50, M the largest number of
entries of the call, M_a the largest number of entries within r_avg:
  e_s = (7 E + M + nbins + 30) u A + omitted,  A = 2 pi rho D sum' (h_k |ln(h_k / r_k^2)| + h_k + r_k^2),
  omitted = 2 pi rho D sum' om (1 + |ln(om / r_k^2)| + |ln(h_k / r_k^2)|),  om = M exp(-E) (1 + 1e-12) / (4 pi rho sigma sqrt(2 pi)),
  e_sbar = max e_s + (M_a + 2) u max |s|,  e_smean = max e_s + (natoms + 1) u max |s|,  e_sbarmean = max e_s + (M_a + natoms + 3) u max |s|
(the maxima over the atoms of the sample)."""
import numpy as np

from distr_ref import BR

LD = np.longdouble
U = 2.0 ** -53
EMAX = 50.0
PI = LD('3.14159265358979323846264338327950288')


def entries(pos, box, c, r_hi):
    """(d float32 [M], atom index [M]) of the entries of centre c in one sample with 0 < (double)d <= r_hi, image-major"""
    pos = np.asarray(pos, dtype=np.float32)
    q = pos[c][None, :] + np.float32(box) * BR.astype(np.float32)            # pos[c] + box*br[j], [27][3] float32
    v = pos[None, :, :] - q[:, None, :]                                      # [27][n][3] float32
    d2 = v[..., 0] * v[..., 0]
    d2 = d2 + v[..., 1] * v[..., 1]
    d2 = d2 + v[..., 2] * v[..., 2]
    d = np.sqrt(d2)
    assert d.dtype == np.float32
    dd = d.astype(np.float64)
    keep = (dd > 0.0) & (dd <= r_hi)
    return d[keep], np.nonzero(keep)[1]


def grid(r_m, nbins):
    """(D, r_k [nbins + 1]) in float64: one division, one product per point"""
    D = np.float64(r_m) / np.float64(nbins)
    return D, np.arange(nbins + 1, dtype=np.float64) * D


def trapezoid(I):
    """I_0 / 2 + I_1 + ... + I_nbins / 2 along the last axis, long double"""
    w = np.ones(I.shape[-1], dtype=LD)
    w[0] = w[-1] = LD(0.5)
    return (I * w).sum(axis=-1)


def smeared(d, rho, sigma, rk):
    """h_k [nbins + 1] long double of one centre from its entries' d"""
    t = rk.astype(LD)[None, :] - np.asarray(d).astype(LD)[:, None]
    g = np.exp(-(t * t) / (2 * LD(sigma) * LD(sigma))).sum(axis=0)
    return g / (4 * PI * rho * LD(sigma) * np.sqrt(2 * PI))


def log_ratio(h, r2):
    """ln(h / r2) where h > 0 and r2 > 0, else 0"""
    ok = (h > 0) & (r2 > 0)
    out = np.zeros(h.shape, dtype=LD)
    out[ok] = np.log(h[ok] / r2[ok])
    return out


def integrand(h, rk):
    """I_k long double: 0 at k = 0, r_k^2 where h_k == 0, else h ln(h / r^2) - h + r^2"""
    r2 = rk.astype(LD) ** 2
    I = h * log_ratio(h, r2) - h + r2
    I[..., 0] = 0
    return I


def local(pos, box, c, r_m, sigma, nbins):
    """one centre of one sample: (s long double, A long double, h [nbins + 1] long double, rho long double, number of entries)"""
    D, rk = grid(r_m, nbins)
    r2 = rk.astype(LD) ** 2
    L = LD(np.float64(np.float32(box)))
    rho = LD(np.asarray(pos).shape[0]) / (L * L * L)
    d, _ = entries(pos, box, c, r_m)
    h = smeared(d, rho, sigma, rk)
    scale = h * np.abs(log_ratio(h, r2)) + h + r2
    scale[0] = 0
    w = 2 * PI * rho * LD(D)
    return -w * trapezoid(integrand(h, rk)), w * trapezoid(scale), h, rho, len(d)


def entropy(pos, box, r_m, sigma, nbins, r_avg, s_cut=-np.inf):
    """pos[ns][n][3], box[ns] float32.  Returns a dict: s, sbar long double [ns][n], nnb, navg int32 [ns][n] (entries within r_m and within
    r_avg), smean, sbarmean long double [ns], nlow int32 [ns], and the bounds e_s [ns][n], e_sbar, e_smean, e_sbarmean [ns] float64"""
    pos = np.ascontiguousarray(pos, dtype=np.float32)
    box = np.ascontiguousarray(box, dtype=np.float32).reshape(-1)
    ns, n = pos.shape[0], pos.shape[1]
    D, rk = grid(r_m, nbins)
    s = np.zeros((ns, n), dtype=LD)
    sbar = np.zeros((ns, n), dtype=LD)
    nnb = np.zeros((ns, n), dtype=np.int32)
    navg = np.zeros((ns, n), dtype=np.int32)
    A = np.zeros((ns, n), dtype=LD)
    hs = np.zeros((ns, n, nbins + 1), dtype=LD)
    rhos = np.zeros(ns, dtype=LD)
    for i in range(ns):
        for c in range(n):
            s[i, c], A[i, c], hs[i, c], rhos[i], nnb[i, c] = local(pos[i], box[i], c, r_m, sigma, nbins)
        for c in range(n):
            _, idx = entries(pos[i], box[i], c, r_avg)
            navg[i, c] = len(idx)
            sbar[i, c] = (s[i, c] + s[i, idx].sum()) / LD(len(idx) + 1)
    out = dict(s=s, sbar=sbar, nnb=nnb, navg=navg, smean=s.mean(axis=1), sbarmean=sbar.mean(axis=1),
               nlow=(sbar < LD(s_cut)).sum(axis=1).astype(np.int32))
    out.update(bounds(A, hs, rhos, rk, D, sigma, nbins, int(nnb.max()) if nnb.size else 0, int(navg.max()) if navg.size else 0, s))
    return out


def bounds(A, hs, rhos, rk, D, sigma, nbins, M, Ma, s):
    """the derived bounds (module docstring) as float64: e_s [ns][n], e_sbar, e_smean, e_sbarmean [ns]"""
    ns, n = A.shape
    r2 = rk.astype(LD) ** 2
    omitted = np.zeros((ns, n), dtype=LD)
    if M > 0:
        for i in range(ns):
            om = LD(M) * np.exp(LD(-EMAX)) * (1 + LD(1e-12)) / (4 * PI * rhos[i] * LD(sigma) * np.sqrt(2 * PI))
            per = np.zeros((n, nbins + 1), dtype=LD)
            per[:, 1:] = om * (1 + np.abs(np.log(om / r2[1:]))[None, :] + np.abs(log_ratio(hs[i][:, 1:], np.broadcast_to(r2[1:], (n, nbins)))))
            omitted[i] = 2 * PI * rhos[i] * LD(D) * trapezoid(per)
    es = ((7 * EMAX + M + nbins + 30) * U * A + omitted).astype(np.float64)
    smax = np.abs(s).max(axis=1).astype(np.float64) if n else np.zeros(ns)
    emax = es.max(axis=1) if n else np.zeros(ns)
    return dict(e_s=es, e_sbar=emax + (Ma + 2) * U * smax, e_smean=emax + (n + 1) * U * smax,
                e_sbarmean=emax + (Ma + n + 3) * U * smax)


def no_entries(natoms, box, r_m, nbins):
    """the closed form of an atom without entries: -2 pi rho (r_m^3 / 3 + r_m D^2 / 6) (the trapezoid rule on r^2 is exact up to that
    term), long double from the float64 grid"""
    D, _ = grid(r_m, nbins)
    L = LD(np.float64(np.float32(box)))
    rm = LD(D) * nbins
    return -2 * PI * (LD(natoms) / (L * L * L)) * (rm ** 3 / 3 + rm * LD(D) ** 2 / 6)
