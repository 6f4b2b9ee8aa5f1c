"""numpy longdouble restatement of include/nm_reweight_hist.h on top of reweight_ref.Problem: the normalised weights as
reweight_ref.expect forms them, the bins by np.searchsorted on the float64 edges with np.histogram's rule (edges[j] <= x <
edges[j+1], the last bin closed on the right), per-bin longdouble sums, and the weight below and above the edges; the tolerance
the GPU tests hold the library to; the Erlang distribution function of the Gamma known answer."""
import math

import numpy as np

import reweight_ref as R

LD = R.LD
TRUNC = 2.0 ** -96      # the accumulator's truncation unit per sample (include/nm_reweight_hist.h)


def codes(x, edges):
    """per sample the bin 0 .. nbins - 1, -1 below edges[0], nbins above edges[-1]; float64 comparisons with the edges only"""
    x, edges = np.asarray(x, np.float64), np.asarray(edges, np.float64)
    nbins = edges.size - 1
    j = np.searchsorted(edges, x, side='right') - 1          # edges[j] <= x < edges[j + 1]; -1 below; nbins from the last edge on
    return np.where(x == edges[-1], nbins - 1, j)


def weights(p, tb, tc, logd):
    """the normalised weights of one target, longdouble (as reweight_ref.expect)"""
    lw = p.log_weights(tb, tc, logd)
    w = np.exp(lw - R._lse(lw, 0))
    return w / w.sum()


def histogram(b, c, count, f, e, v, tb, tc, x, edges):
    """(hist (T, nq, nbins), outside (T, nq, 2) = (below, above), ess (T,)) in longdouble"""
    p = R.Problem(b, c, count, e, v)
    ld = p.logd(f)
    tb, tc = np.atleast_1d(tb), np.atleast_1d(tc)
    x, edges = np.atleast_2d(np.asarray(x, np.float64)), np.atleast_2d(np.asarray(edges, np.float64))
    nq, nbins = x.shape[0], edges.shape[1] - 1
    slot = [codes(x[q], edges[q]) + 1 for q in range(nq)]   # 0 below, 1 .. nbins the bins, nbins + 1 above
    hist, outside, ess = np.zeros((tb.size, nq, nbins), LD), np.zeros((tb.size, nq, 2), LD), np.zeros(tb.size, LD)
    for t in range(tb.size):
        w = weights(p, tb[t], tc[t], ld)
        ess[t] = 1 / (w * w).sum()
        for q in range(nq):
            acc = np.zeros(nbins + 2, LD)
            np.add.at(acc, slot[q], w)
            hist[t, q], outside[t, q] = acc[1:-1], (acc[0], acc[-1])
    return hist, outside, ess


def tol(n, k, u_max, want):
    """per bin: logd and tf each lie within tol_map and the argument's error is the weight's relative error; every sample's weight
    is truncated by less than 2^-96"""
    return 2 * R.tol_map(n, k, u_max) * np.asarray(want, np.float64) + n * TRUNC


def erlang_cdf(a, rate, x):
    """P(X < x) of Gamma(shape a, rate) for an integer a: 1 - exp(-rate x) sum_{i < a} (rate x)^i / i!"""
    y = rate * np.asarray(x, np.float64)
    return 1.0 - np.exp(-y) * sum(y ** i / math.factorial(i) for i in range(int(a)))
