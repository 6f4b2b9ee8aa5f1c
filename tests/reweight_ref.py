"""numpy longdouble restatement of include/nm_reweight.h: the map, the iteration and the expectations, in blocks of samples (no
K x N array beyond a block), and the tolerance the GPU tests hold the library to.  The samples are centred on their means and
the states' offsets s_k = b_k e0 + c_k v0 are carried exactly (fractions), which changes nothing in exact arithmetic and keeps
the restatement's own error at a few 2^-64 of the centred magnitudes whatever common offset e and v carry."""
from fractions import Fraction

import numpy as np

LD = np.longdouble
UNIT = 2.0 ** -53
BLOCK = 8192


def tol_map(n, k, u_max):
    """(N + K + 64) u + 16 u U: what any fixed-order float64 summation meets, sequential worst case"""
    return (n + k + 64) * UNIT + 16 * UNIT * u_max


def u_max(b, c, e, v):
    """U = max |b_k (e_n - mean e) + c_k (v_n - mean v)| over states (or targets) and samples"""
    e, v = np.asarray(e, np.float64), np.asarray(v, np.float64)
    ec, vc = e - e.mean(), v - v.mean()
    return max(float(np.abs(bk * ec + ck * vc).max()) for bk, ck in zip(np.atleast_1d(b), np.atleast_1d(c)))


def _ld(fr):
    """a Fraction as a longdouble (two float64 pieces)"""
    hi = float(fr)
    return LD(hi) + LD(float(fr - Fraction(hi)))


def _lse(x, axis):
    m = x.max(axis=axis, keepdims=True)
    return np.squeeze(m + np.log(np.exp(x - m).sum(axis=axis, keepdims=True)), axis=axis)


class Problem:
    """the centred samples and the exact offsets of the states"""

    def __init__(self, b, c, count, e, v):
        self.b, self.c = np.asarray(b, np.float64), np.asarray(c, np.float64)
        self.count = np.asarray(count, np.int64)
        e, v = np.asarray(e, np.float64).reshape(-1), np.asarray(v, np.float64).reshape(-1)
        assert self.count.sum() == e.size == v.size
        self.e0, self.v0 = float(e.astype(LD).mean()), float(v.astype(LD).mean())
        self.ec, self.vc = e.astype(LD) - LD(self.e0), v.astype(LD) - LD(self.v0)
        self.n = e.size

    def offset(self, b, c):
        return Fraction(float(b)) * Fraction(self.e0) + Fraction(float(c)) * Fraction(self.v0)

    def logd(self, f):
        on = self.count > 0
        a = np.array([LD(np.log(LD(int(n)))) + _ld(Fraction(float(fk)) - self.offset(bk, ck))
                      for n, fk, bk, ck in zip(self.count[on], np.asarray(f, np.float64)[on], self.b[on], self.c[on])], dtype=LD)
        bb, cc = self.b[on].astype(LD)[:, None], self.c[on].astype(LD)[:, None]
        out = np.empty(self.n, dtype=LD)
        for i in range(0, self.n, BLOCK):
            out[i:i + BLOCK] = _lse(a[:, None] - (bb * self.ec[None, i:i + BLOCK] + cc * self.vc[None, i:i + BLOCK]), 0)
        return out

    def log_weights(self, tb, tc, logd):
        """t[n] = -(tb ec + tc vc) - logd[n]: the log weights up to the target's offset and tf"""
        return -(LD(tb) * self.ec + LD(tc) * self.vc) - logd

    def free(self, tb, tc, logd):
        """tf = -LSE_n(-u_t(n) - logd[n])"""
        return _ld(self.offset(tb, tc)) - _lse(self.log_weights(tb, tc, logd), 0)


def apply_map(b, c, count, f, e, v):
    """one application: (f_new = F(f) - F(f)[0], logd of the f that went in), longdouble"""
    p = Problem(b, c, count, e, v)
    ld = p.logd(f)
    big = np.array([p.free(bk, ck, ld) for bk, ck in zip(p.b, p.c)], dtype=LD)
    return big - big[0], ld


def _map64(b, c, lc, on, f, ec, vc):
    """the same map in float64 on centred data, for the bulk of the iteration"""
    ld = np.empty(ec.size)
    for i in range(0, ec.size, BLOCK):
        t = (lc[on] + f[on])[:, None] - (b[on, None] * ec[None, i:i + BLOCK] + c[on, None] * vc[None, i:i + BLOCK])
        m = t.max(axis=0)
        ld[i:i + BLOCK] = m + np.log(np.exp(t - m).sum(axis=0))
    big = np.empty(b.size)
    for k in range(b.size):
        t = -(b[k] * ec + c[k] * vc) - ld
        m = t.max()
        big[k] = -(m + np.log(np.exp(t - m).sum()))
    return big - big[0]


def solve(b, c, count, f0, e, v, tol=1e-12, max_iter=100000):
    """the fixed point: iterated in float64 on the centred problem until delta <= 1e-11, then in longdouble until delta <= tol;
    returns (f as float64, longdouble iterations made)"""
    p = Problem(b, c, count, e, v)
    off = np.array([float(p.offset(bk, ck) - p.offset(p.b[0], p.c[0])) for bk, ck in zip(p.b, p.c)])
    ec, vc = p.ec.astype(np.float64), p.vc.astype(np.float64)
    on = p.count > 0
    lc = np.log(np.maximum(p.count, 1).astype(np.float64))
    f = np.asarray(f0, np.float64) - off
    for _ in range(max_iter):
        fn = _map64(p.b, p.c, lc, on, f, ec, vc)
        delta = np.abs(fn - f).max()
        f = fn
        if delta <= 1e-11:
            break
    f = f + off
    for it in range(1, 50):
        fn = apply_map(b, c, count, f, e, v)[0]
        delta = float(np.abs(fn - f.astype(LD)).max())
        f = fn.astype(np.float64)
        if delta <= tol:
            break
    return f, it


def expect(b, c, count, f, e, v, tb, tc, obs=None):
    """dict of tf, ess (T,), mean (T, 2), cov (T, 3), omean (T, nobs) in longdouble: central moments by a second pass"""
    p = Problem(b, c, count, e, v)
    ld = p.logd(f)
    tb, tc = np.atleast_1d(tb), np.atleast_1d(tc)
    obs = np.zeros((0, p.n), dtype=LD) if obs is None else np.asarray(obs, np.float64).reshape(-1, p.n).astype(LD)
    nt = tb.size
    out = dict(tf=np.empty(nt, LD), ess=np.empty(nt, LD), mean=np.empty((nt, 2), LD), cov=np.empty((nt, 3), LD),
               omean=np.empty((nt, obs.shape[0]), LD))
    for t in range(nt):
        lw = p.log_weights(tb[t], tc[t], ld)
        w = np.exp(lw - _lse(lw, 0))
        w = w / w.sum()
        out['tf'][t] = p.free(tb[t], tc[t], ld)
        out['ess'][t] = 1 / (w * w).sum()
        me, mv = (w * p.ec).sum(), (w * p.vc).sum()
        out['mean'][t] = LD(p.e0) + me, LD(p.v0) + mv
        de, dv = p.ec - me, p.vc - mv
        out['cov'][t] = (w * de * de).sum(), (w * de * dv).sum(), (w * dv * dv).sum()
        out['omean'][t] = (w[None, :] * obs).sum(axis=1)
    return out


# ---- the known-answer set shared by the CPU and the GPU tests
GAMMA_A, GAMMA_M = 8.0, 6.0
GAMMA_B = 1.0 * 1.15 ** np.arange(6)
GAMMA_C = 0.5 * 1.12 ** np.arange(6)
GAMMA_COUNT = 6000


def gamma_set(count=GAMMA_COUNT, seed=20081231):
    """K = 6 overlapping states: e ~ Gamma(a, 1/b_k), v ~ Gamma(m, 1/c_k), independent; (b, c, counts, e, v), samples in state
    order.  Exact: f_k - f_0 = a ln(b_k/b_0) + m ln(c_k/c_0); at (tb, tc): <e> = a/tb, var_e = a/tb^2, <v> = m/tc, var_v =
    m/tc^2, cov_ev = 0."""
    rng = np.random.default_rng(seed)
    e = np.concatenate([rng.gamma(GAMMA_A, 1.0 / bk, count) for bk in GAMMA_B])
    v = np.concatenate([rng.gamma(GAMMA_M, 1.0 / ck, count) for ck in GAMMA_C])
    return GAMMA_B.copy(), GAMMA_C.copy(), np.full(6, count, dtype=np.int64), e, v


def gamma_exact_f():
    return GAMMA_A * np.log(GAMMA_B / GAMMA_B[0]) + GAMMA_M * np.log(GAMMA_C / GAMMA_C[0])


def gamma_targets():
    """the six states and the five points between neighbours"""
    tb = np.concatenate([GAMMA_B, np.sqrt(GAMMA_B[:-1] * GAMMA_B[1:])])
    tc = np.concatenate([GAMMA_C, np.sqrt(GAMMA_C[:-1] * GAMMA_C[1:])])
    return tb, tc


def gamma_exact_moments(tb, tc):
    """(mean (T, 2), cov (T, 3))"""
    z = np.zeros_like(tb)
    return np.stack([GAMMA_A / tb, GAMMA_M / tc], 1), np.stack([GAMMA_A / tb ** 2, z, GAMMA_M / tc ** 2], 1)


def gamma_start(b, c, count, e, v):
    """the mean of u_k over state k's own samples"""
    k = len(b)
    return b * e.reshape(k, -1).mean(axis=1) + c * v.reshape(k, -1).mean(axis=1)
