"""Where the time of k-means goes: nm_cluster_kmeans on two Gaussian blobs at the grid a user runs, 32 x 32
points x 1024 samples, k = 2 and 10 restarts from k-means++ seeds, tol = 0.  nm_cluster_kmeans_last_timing's device events split
the call into the upload and screen, the assignment passes and the update passes; the wall time of the whole call beside them says
what share is launches and the host's looks.  Two baselines from the same initial centres, alternated with the library in one
process after a warm-up: sklearn's KMeans on 16 threads, restart after restart, and a float64 torch restatement on the same GPU
(cdist, argmin, index_add_).  The labels of the library's best restart are compared with both.  The baselines take seconds a round
(index_add_ adds 2^20 rows into two with atomics), so they run in the first --baselines rounds only.  Without a GPU it fails: the
library has no fallback and the torch baseline asks for the device.

    python scripts/probe_kmeans.py [--npoints 1048576] [--ndim 2 8] [--restarts 10] [--repeats 3] [--baselines 1]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
from sklearn.cluster import KMeans

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralmelting_amd import _lib as B  # noqa: E402
from neuralmelting_amd import cluster  # noqa: E402

HBM = 6.29e12                               # bytes per second: the floor of a step is one read of x
MAX_ITER = 300


def timing():
    ms = np.zeros(3)
    B.load().nm_cluster_kmeans_last_timing(ms)
    return ms


def two_blobs(n, nd, rng):
    x = rng.standard_normal((n, nd))
    x[n // 2:, 0] += 6.0
    return x[rng.permutation(n)]


def sklearn_restarts(x, init):
    """[(labels, inertia, steps)] of sklearn's Lloyd iteration from every initial set"""
    out = []
    for c in init:
        km = KMeans(n_clusters=c.shape[0], init=c, n_init=1, algorithm='lloyd', tol=0, max_iter=MAX_ITER).fit(x)
        out.append((km.labels_, km.inertia_, km.n_iter_))
    return out


def torch_restarts(x, init):
    """the same on the GPU in float64, x already there: a step is cdist, argmin, index_add_ and a comparison of the labels"""
    out = []
    for c in torch.as_tensor(init, device=x.device):
        before = None
        for step in range(1, MAX_ITER + 1):
            label = torch.cdist(x, c).argmin(dim=1)
            if before is not None and torch.equal(label, before):
                break
            before = label
            count = torch.bincount(label, minlength=c.shape[0])
            total = torch.zeros_like(c).index_add_(0, label, x)
            c = torch.where(count[:, None] > 0, total / count[:, None].clamp(min=1), c)
        inertia = ((x - c[label]) ** 2).sum()
        out.append((label.cpu().numpy(), float(inertia), step - 1))
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--npoints', type=int, nargs='+', default=[32 * 32 * 1024])
    p.add_argument('--ndim', type=int, nargs='+', default=[2, 8])
    p.add_argument('--clusters', type=int, default=2)
    p.add_argument('--restarts', type=int, default=10)
    p.add_argument('--repeats', type=int, default=3)
    p.add_argument('--baselines', type=int, default=1, help='the rounds in which the two baselines run as well (0: the library alone)')
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('probe_kmeans: no GPU')
    rng = np.random.default_rng(256)
    dev = torch.device('cuda')
    warm = two_blobs(4096, 2, rng)
    cluster.kmeans(warm, cluster.seeds(warm, 2, 2, 1))                      # the warm-up: the library and its kernels are loaded
    torch_restarts(torch.as_tensor(warm, device=dev), cluster.seeds(warm, 2, 2, 1))
    sklearn_restarts(warm, cluster.seeds(warm, 2, 2, 1))
    for n in a.npoints:
        for nd in a.ndim:
            x = two_blobs(n, nd, rng)
            init = cluster.seeds(x, a.clusters, a.restarts, 256)
            rows, sk_ms, th_ms = [], [], []
            for rep in range(a.repeats):
                t0 = time.perf_counter()
                label, centre, count, inertia, iters, status, best = cluster.kmeans(x, init, MAX_ITER, 0.0)
                rows.append(np.append(timing(), (time.perf_counter() - t0) * 1e3))
                if rep >= a.baselines:
                    continue
                t0 = time.perf_counter()
                sk = sklearn_restarts(x, init)
                sk_ms.append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                xd = torch.as_tensor(x, device=dev)                         # the upload is in the library's wall time too
                th = torch_restarts(xd, init)
                torch.cuda.synchronize()
                th_ms.append((time.perf_counter() - t0) * 1e3)
            up, assign, update, wall = np.min(np.array(rows), axis=0)
            steps = int(iters.max()) + 1                                    # the last restart's steps, its closing assignment among them
            res = dict(npoints=n, ndim=nd, k=a.clusters, restarts=a.restarts, repeats=a.repeats, iters=iters.tolist(), status=status.tolist(),
                       best=best, steps=steps, upload_ms=up, assign_ms=assign, update_ms=update, wall_ms=wall,
                       assign_us_per_step=assign / steps * 1e3, update_us_per_step=update / steps * 1e3,
                       floor_us_per_step=n * nd * 8 / HBM * 1e6, share_outside_device_events=1.0 - (up + assign + update) / wall,
                       inertia=float(inertia[best]))
            if a.baselines > 0:
                res.update(baseline_rounds=len(sk_ms), sklearn_ms=min(sk_ms), sklearn_threads=int(os.environ.get('OMP_NUM_THREADS', 0)),
                           torch_ms=min(th_ms), sklearn_steps=[int(s[2]) for s in sk], torch_steps=[int(t[2]) for t in th],
                           labels_differ_from_sklearn=int((sk[best][0] != label).sum()),
                           labels_differ_from_torch=int((th[best][0] != label).sum()), sklearn_inertia=float(sk[best][1]), torch_inertia=th[best][1])
            print(json.dumps({k: (float('%.5g' % v) if isinstance(v, float) else v) for k, v in res.items()}))
            sys.stdout.flush()
    return 0


if __name__ == '__main__':
    sys.exit(main())
