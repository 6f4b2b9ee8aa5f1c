"""numpy longdouble restatement of include/nm_reweight_boot.h: a replicate is the problem of nm_reweight.h on the multiset in which
sample n occurs mult[n] times.  Written directly in the log-sum-exp form with ln mult over the samples of non-zero multiplicity,
not in the perturbative form the kernels use; builds on reweight_ref.Problem.  And the statistical inefficiency as a plain
O(n^2) sum."""
import numpy as np

import reweight_ref as R

LD = R.LD


class Replicate(R.Problem):
    def __init__(self, b, c, count, e, v, mult):
        super().__init__(b, c, count, e, v)
        mult = np.asarray(mult).reshape(-1).astype(np.int64)
        assert mult.size == self.n and mult.sum() == self.n and (mult >= 0).all()
        self.mult = mult
        self.on = mult > 0
        self.lm = np.log(mult[self.on].astype(LD))

    def free(self, tb, tc, logd):
        """F_r = -LSE over the n with mult > 0 of (ln mult[n] - u_t(n) - logd[n])"""
        return R._ld(self.offset(tb, tc)) - R._lse(self.lm + self.log_weights(tb, tc, logd)[self.on], 0)


def apply_map(b, c, count, f, e, v, mult):
    """one application for one replicate: (f_new = F_r(f) - F_r(f)[0], F_r(f) itself), longdouble"""
    p = Replicate(b, c, count, e, v, mult)
    ld = p.logd(f)
    big = np.array([p.free(bk, ck, ld) for bk, ck in zip(p.b, p.c)], dtype=LD)
    return big - big[0], big


def _map64(b, c, lc, on, f, ec, vc, lm, sel):
    """the replicate's map in float64 on centred data (states' offsets folded into f by the caller)"""
    t = (lc[on] + f[on])[:, None] - (b[on, None] * ec[None, :] + c[on, None] * vc[None, :])
    m = t.max(axis=0)
    ld = m + np.log(np.exp(t - m).sum(axis=0))
    t = lm[None, :] - (b[:, None] * ec[None, sel] + c[:, None] * vc[None, sel]) - ld[None, sel]
    m = t.max(axis=1)
    big = -(m + np.log(np.exp(t - m[:, None]).sum(axis=1)))
    return big - big[0]


def solve(b, c, count, f, e, v, mult, tol=1e-12, max_iter=200, exact=True):
    """the replicate's iteration from the start f: (the iterates as float64 [f_1, f_2, ...], their deltas).  exact: every
    application in longdouble; otherwise float64 on the centred problem (for the iteration count of the larger sets)"""
    iterates, deltas = [], []
    if exact:
        cur = np.asarray(f, np.float64).astype(LD)
        for _ in range(max_iter):
            new = apply_map(b, c, count, cur.astype(np.float64), e, v, mult)[0]
            deltas.append(float(np.abs(new - cur).max()))
            cur = new.astype(np.float64).astype(LD)
            iterates.append(cur.astype(np.float64))
            if deltas[-1] <= tol:
                break
        return iterates, deltas
    p = Replicate(b, c, count, e, v, mult)
    off = np.array([float(p.offset(bk, ck) - p.offset(p.b[0], p.c[0])) for bk, ck in zip(p.b, p.c)])
    ec, vc = p.ec.astype(np.float64), p.vc.astype(np.float64)
    on = p.count > 0
    lc = np.log(np.maximum(p.count, 1).astype(np.float64))
    cur = np.asarray(f, np.float64) - off
    for _ in range(max_iter):
        new = _map64(p.b, p.c, lc, on, cur, ec, vc, p.lm.astype(np.float64), p.on)
        deltas.append(float(np.abs(new - cur).max()))
        cur = new
        iterates.append(cur + off)
        if deltas[-1] <= tol:
            break
    return iterates, deltas


def expect(b, c, count, fr, e, v, mult, tb, tc, obs=None):
    """dict of tf, ess (T,), mean (T, 2), cov (T, 3), omean (T, nobs) of one replicate in longdouble: the weights of the multiset,
    w_n = mult[n] exp(-u_t(n) - logd_r[n] + tf); ess = (sum m w)^2 / sum m w^2 with w the weight of one copy"""
    p = Replicate(b, c, count, e, v, mult)
    ld = p.logd(fr)
    tb, tc = np.atleast_1d(tb), np.atleast_1d(tc)
    obs = np.zeros((0, p.n), dtype=LD) if obs is None else np.asarray(obs, np.float64).reshape(-1, p.n).astype(LD)
    nt = tb.size
    out = dict(tf=np.empty(nt, LD), ess=np.empty(nt, LD), mean=np.empty((nt, 2), LD), cov=np.empty((nt, 3), LD),
               omean=np.empty((nt, obs.shape[0]), LD))
    m = p.mult[p.on].astype(LD)
    ec, vc, ob = p.ec[p.on], p.vc[p.on], obs[:, p.on]
    for t in range(nt):
        lw = p.log_weights(tb[t], tc[t], ld)[p.on]          # of one copy
        one = np.exp(lw - R._lse(p.lm + lw, 0))
        w = m * one
        w = w / w.sum()
        out['tf'][t] = p.free(tb[t], tc[t], ld)
        out['ess'][t] = (m * one).sum() ** 2 / (m * one * one).sum()
        me, mv = (w * ec).sum(), (w * vc).sum()
        out['mean'][t] = LD(p.e0) + me, LD(p.v0) + mv
        de, dv = ec - me, vc - mv
        out['cov'][t] = (w * de * de).sum(), (w * de * dv).sum(), (w * dv * dv).sum()
        out['omean'][t] = (w[None, :] * ob).sum(axis=1)
    return out


def inefficiency(x):
    """g = 1 + 2 sum_{t >= 1} (1 - t/n) C(t) up to the first C(t) <= 0, with explicit loops"""
    x = [float(y) for y in x]
    n = len(x)
    if n < 2:
        return 1.0
    mean = sum(x) / n
    dx = [y - mean for y in x]
    var = sum(y * y for y in dx) / n
    if not var > 0.0:
        return 1.0
    g = 1.0
    for t in range(1, n):
        ct = sum(dx[i] * dx[i + t] for i in range(n - t)) / ((n - t) * var)
        if ct <= 0.0:
            break
        g += 2.0 * (1.0 - t / n) * ct
    return max(g, 1.0)
