"""Timing of the block-bootstrap error bars (include/nm_reweight_boot.h) on one GPU, on the set of scripts/bench_reweight.py
(K = 32 x 32 states, N = 2^20 Gamma samples, the base f converged to 1e-9), R = 64 replicates, 8192 targets.  Medians of the host
clock over whole calls:

  batched    one nm_reweight_boot_solve plus one nm_reweight_boot_expect over all replicates;
  baseline   what the interface of nm_reweight.h alone allows: per replicate materialise the resampled set with np.repeat,
             nm_reweight_solve from f, nm_reweight_expect.  --baseline replicates (8) are timed and the sum is SCALED by R / 8.

    python scripts/bench_reweight_boot.py
    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/bench_reweight_boot.py --profile    # per-launch times, a run of its own
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_reweight import gamma_grid  # noqa: E402
from neuralmelting_amd import reweight  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--side', type=int, default=32, help='states per axis: K = side^2')
    ap.add_argument('--per_state', type=int, default=1024, help='samples per state: N = K * per_state')
    ap.add_argument('--replicates', type=int, default=64)
    ap.add_argument('--block', type=int, default=8, help='block length of the resampling (the Gamma samples are independent: any length serves)')
    ap.add_argument('--baseline', type=int, default=8, help='replicates of the baseline that are timed; the sum is scaled to --replicates')
    ap.add_argument('--targets', type=int, default=256, help='fine temperatures per pressure: side * this many targets')
    ap.add_argument('--tol', type=float, default=1e-9)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--profile', action='store_true', help='only one batched solve and expectation, for a kernel trace')
    a = ap.parse_args()
    b, c, count, e, v = gamma_grid(a.side, a.per_state)
    f0 = b * e.reshape(b.size, -1).mean(axis=1) + c * v.reshape(b.size, -1).mean(axis=1)
    tb = np.repeat(1.03 ** np.linspace(0, a.side - 1, a.targets), a.side)
    tc = np.tile(c[:a.side], a.targets)
    f, iters, delta = reweight.solve(b, c, count, e, v, f0, a.tol, 20000)
    mult = reweight.block_multiplicities(a.per_state, np.full(b.size, a.block), a.replicates, 256).reshape(a.replicates, -1)
    res = dict(states=int(b.size), samples=int(e.size), replicates=a.replicates, targets=int(tb.size), tol=a.tol, base_iterations=iters,
               base_delta=delta)

    def batched():
        fr, it, de, st = reweight.boot_solve(b, c, count, e, v, f, mult, a.tol, 20000)
        return fr, it, de, st, reweight.boot_expect(b, c, count, f, e, v, mult, fr, tb, tc)

    def single(r):
        idx = np.repeat(np.arange(e.size), mult[r])
        er, vr = e[idx], v[idx]
        fr, it, de = reweight.solve(b, c, count, er, vr, f, a.tol, 20000)
        return fr, it, reweight.expect(b, c, count, fr, er, vr, tb, tc)

    reweight.boot_solve(b, c, count, e, v, f, mult[:2], 0.0, 1)                              # warm-up: code objects, allocator
    reweight.boot_expect(b, c, count, f, e, v, mult[:2], np.stack([f, f]), tb[:8], tc[:8])
    if a.profile:
        batched()
        return
    single(0)
    t_batched, t_base = [], []
    for _ in range(a.repeats):                                                               # alternated: the machine is shared
        t = time.perf_counter()
        fr, it, de, st, ex = batched()
        t_batched.append(time.perf_counter() - t)
        t = time.perf_counter()
        ones = [single(r) for r in range(a.baseline)]
        t_base.append((time.perf_counter() - t) * a.replicates / a.baseline)
    res.update(batched_s=float(np.median(t_batched)), batched_all_s=t_batched, baseline_timed_replicates=a.baseline,
               baseline_scaled_s=float(np.median(t_base)), baseline_scaled_all_s=t_base,
               replicate_iterations=[int(it.min()), int(it.max())], baseline_iterations=[int(o[1]) for o in ones],
               status_counts=[int((st == k).sum()) for k in range(3)],
               # the two paths solve the same problems: the baseline centres on other sample means and sums in another order
               largest_f_difference=float(max(np.abs(fr[r] - ones[r][0]).max() for r in range(a.baseline))),
               largest_mean_e_difference=float(max(np.abs(ex['mean'][r, :, 0] - ones[r][2]['mean'][:, 0]).max() for r in range(a.baseline))))
    res['speedup'] = res['baseline_scaled_s'] / res['batched_s']
    print(json.dumps(res))


if __name__ == '__main__':
    main()
