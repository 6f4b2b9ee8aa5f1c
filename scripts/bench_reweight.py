"""Timing of the reweighting stage (include/nm_reweight.h) on one GPU: seconds per application of the map from the difference
of two series of synchronous nm_reweight_solve calls with different iteration counts (set-up, copies and the first launches cancel), the
iterations to a tolerance, the expectation call, and the same map as blocked float64 numpy on a thread pool for comparison.

    python scripts/bench_reweight.py                      # K = 32 x 32 states, N = 2^20 samples of Gamma data
    python scripts/bench_reweight.py --numpy 16           # adds the host restatement at N / 16, scaled by K N
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/bench_reweight.py --profile    # per-launch times, a run of its own
    python scripts/bench_reweight.py --hist 3 128         # only: nm_reweight_histogram (3 quantities, 128 bins) against nm_reweight_expect
                                                          # with 3 observables, whole calls alternated in one process; with --profile one call of each
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralmelting_amd import reweight  # noqa: E402


def gamma_grid(side, per_state, seed=1):
    """side x side states b_i = 1.03^i, c_j = 0.5 * 1.03^j; e ~ Gamma(8, 1/b), v ~ Gamma(6, 1/c), per_state samples each"""
    rng = np.random.default_rng(seed)
    b = np.repeat(1.03 ** np.arange(side), side)
    c = np.tile(0.5 * 1.03 ** np.arange(side), side)
    e = rng.gamma(8.0, 1.0 / b[:, None], (b.size, per_state))
    v = rng.gamma(6.0, 1.0 / c[:, None], (b.size, per_state))
    return b, c, np.full(b.size, per_state, dtype=np.int64), e.reshape(-1), v.reshape(-1)


def numpy_map(b, c, count, f, e, v, threads, block=4096):
    """one application of the map in float64, blocks of samples on a thread pool (numpy releases the GIL inside exp)"""
    a = np.log(count) + f
    ld = np.empty(e.size)

    def denom(i):
        t = a[:, None] - (b[:, None] * e[None, i:i + block] + c[:, None] * v[None, i:i + block])
        m = t.max(axis=0)
        ld[i:i + block] = m + np.log(np.exp(t - m).sum(axis=0))

    def free(k):
        t = -(b[k] * e + c[k] * v) - ld
        m = t.max()
        return -(m + np.log(np.exp(t - m).sum()))

    with ThreadPoolExecutor(threads) as pool:
        list(pool.map(denom, range(0, e.size, block)))
        big = np.array(list(pool.map(free, range(b.size))))
    return big - big[0]


def timed(fn, repeats):
    out = []
    for _ in range(repeats):
        t = time.perf_counter()
        res = fn()
        out.append(time.perf_counter() - t)
    return float(np.median(out)), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=32, help='states per axis: K = side^2')
    ap.add_argument('--per_state', type=int, default=1024, help='samples per state: N = K * per_state')
    ap.add_argument('--iters', type=int, nargs=2, default=[8, 32], help='the two iteration counts whose difference is timed')
    ap.add_argument('--calls', type=int, default=16, help='solve calls per timed region (a region should last a good fraction of a second)')
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--tol', type=float, default=1e-9)
    ap.add_argument('--targets', type=int, default=256, help='fine temperatures per pressure for the expectation call')
    ap.add_argument('--numpy', type=int, default=0, help='time the host restatement on N / this many samples (0: skip)')
    ap.add_argument('--threads', type=int, default=16)
    ap.add_argument('--profile', action='store_true', help='only 20 iterations and one expectation call, for a kernel trace')
    ap.add_argument('--hist', type=int, nargs=2, metavar=('NQ', 'NBINS'), default=None,
                    help='only the histogram leg: NQ quantities (e, v, then noise) in NBINS bins over their range at the --targets grid')
    a = ap.parse_args()
    b, c, count, e, v = gamma_grid(a.side, a.per_state)
    f0 = b * e.reshape(b.size, -1).mean(axis=1) + c * v.reshape(b.size, -1).mean(axis=1)
    tb = np.repeat(1.03 ** np.linspace(0, a.side - 1, a.targets), a.side)
    tc = np.tile(c[:a.side], a.targets)
    res = dict(states=int(b.size), samples=int(e.size))
    reweight.solve(b, c, count, e, v, f0, 0.0, 2)                                            # warm-up: code objects, allocator
    if a.hist:
        nq, nbins = a.hist
        rng = np.random.default_rng(2)
        x = np.stack([e, v] + [rng.normal(size=e.size) for _ in range(nq - 2)])[:nq]
        edges = reweight.linear_edges(x, nbins)
        f, iters, delta = reweight.solve(b, c, count, e, v, f0, a.tol, 20000)
        both = (lambda: reweight.expect(b, c, count, f, e, v, tb, tc, x), lambda: reweight.histogram(b, c, count, f, e, v, tb, tc, x, edges))
        for fn in both:                                                                      # warm-up: code objects, allocator
            fn()
        if a.profile:
            return
        times = ([], [])
        for _ in range(a.repeats):                                                           # alternated: the box is shared
            for fn, out in zip(both, times):
                out.append(timed(fn, 1)[0])
        hist, outside = both[1]()
        res.update(targets=int(tb.size), nq=nq, nbins=nbins, iterations=iters, delta=delta, expect_s=float(np.median(times[0])),
                   histogram_s=float(np.median(times[1])), expect_all_s=times[0], histogram_all_s=times[1],
                   largest_sum_error=float(np.abs(hist.sum(axis=2) + outside.sum(axis=2) - 1).max()))
        res['histogram_over_expect'] = res['histogram_s'] / res['expect_s']
        print(json.dumps(res))
        return
    if a.profile:
        f, _, _ = reweight.solve(b, c, count, e, v, f0, 0.0, 20)
        reweight.expect(b, c, count, f, e, v, tb, tc)
        return
    lo, hi = a.iters

    def calls(n):
        # tol = 0 still ends the iteration once it reaches its exact floating-point fixed point (delta = 0): a count that large times nothing
        for _ in range(a.calls):
            if reweight.solve(b, c, count, e, v, f0, 0.0, n)[1] != n:
                raise SystemExit('--iters %d: the iteration reached its fixed point earlier; time smaller counts' % n)

    t_lo, _ = timed(lambda: calls(lo), a.repeats)
    t_hi, _ = timed(lambda: calls(hi), a.repeats)
    res.update(calls=a.calls, calls_s={str(lo): t_lo, str(hi): t_hi}, s_per_iteration=(t_hi - t_lo) / (hi - lo) / a.calls)
    res['exp_per_s'] = 2.0 * b.size * e.size / res['s_per_iteration']
    t_solve, (f, iters, delta) = timed(lambda: reweight.solve(b, c, count, e, v, f0, a.tol, 20000), 1)
    res.update(tol=a.tol, iterations=iters, delta=delta, solve_s=t_solve)
    t_ex, _ = timed(lambda: reweight.expect(b, c, count, f, e, v, tb, tc), a.repeats)
    res.update(targets=int(tb.size), expect_s=t_ex)
    if a.numpy:
        n = e.size // a.numpy
        pick = np.arange(e.size).reshape(b.size, -1)[:, :a.per_state // a.numpy].reshape(-1)
        cs = np.full(b.size, a.per_state // a.numpy, dtype=np.int64)
        t_np, _ = timed(lambda: numpy_map(b, c, cs, f0, e[pick], v[pick], a.threads), 2)
        res.update(numpy_samples=int(n), numpy_threads=a.threads, numpy_s_per_iteration=t_np,
                   numpy_s_per_iteration_scaled_to_N=t_np * e.size / pick.size)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
