"""What the manifold stage costs: nm_tsne_affinities and one nm_tsne_gradient at --npoints with --k neighbours,
split by nm_tsne_last_timing's device events, the all-pairs pass beside the float64 vector rate of the part; then the whole
schedule (--iterations steps, sklearn's defaults) on a synthetic --grid of two-phase projections, and, with --host,
sklearn.manifold.TSNE(method='barnes_hut') on the same points on the host: the only existing baseline.  The trustworthiness of both
embeddings is taken on the same --sample points.  One JSON line per measurement.

    python scripts/bench_manifold.py [--npoints 32768] [--k 1536] [--ndim 8] [--grid 8 8 512] [--iterations 1000] [--host]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralmelting_amd import _lib as B  # noqa: E402
from neuralmelting_amd import manifold  # noqa: E402

F64_RATE = 256 * 4 * 16 * 2.4e9             # float64 vector operations per second: 256 CUs x 4 SIMDs x 16 lanes per clock at 2.4 GHz
THREADS = 16


def timing():
    ms = np.zeros(5)
    B.load().nm_tsne_last_timing(ms.ctypes.data_as(B.c_double_p))
    return ms


def two_phase(n, nd, rng):
    """projections like pca's on a melting grid: two blobs along component 0, the variance falling with the component"""
    x = rng.standard_normal((n, nd)) * (0.6 ** np.arange(nd))
    x[:, 0] = 0.3 * x[:, 0] + np.where(rng.random(n) < 0.5, 1.0, -1.0)
    return x


def show(**res):
    print(json.dumps({k: (float('%.5g' % v) if isinstance(v, float) else v) for k, v in res.items()}))
    sys.stdout.flush()


def trust(x, y, sample, rng):
    from sklearn.manifold import trustworthiness
    sub = rng.choice(x.shape[0], min(sample, x.shape[0]), replace=False)
    return float(trustworthiness(x[sub], y[sub], n_neighbors=12))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--npoints', type=int, nargs='*', default=[32768])
    p.add_argument('--k', type=int, default=1536)
    p.add_argument('--ndim', type=int, default=8)
    p.add_argument('--ncomp', type=int, default=2)
    p.add_argument('--repeats', type=int, default=2)
    p.add_argument('--grid', type=int, nargs=3, default=[8, 8, 512])
    p.add_argument('--iterations', type=int, default=1000)
    p.add_argument('--sample', type=int, default=4096)
    p.add_argument('--host', action='store_true', help="time sklearn's Barnes-Hut t-SNE on the grid's points as well")
    p.add_argument('--no-device', action='store_true', help='the host baseline alone')
    a = p.parse_args()
    rng = np.random.default_rng(256)
    if not a.no_device:
        warm = two_phase(2048, a.ndim, rng)
        nbr, pc, _ = manifold.affinities(warm, 10.0, 31)                    # the warm-up: the library and its kernels are loaded
        manifold.gradient(nbr, pc, manifold.start(warm, a.ncomp))
    for n in ([] if a.no_device else a.npoints):
        x = two_phase(n, a.ndim, rng)
        k = min(a.k, n - 1)
        rows = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            nbr, pc, beta = manifold.affinities(x, k / 3.0, k)
            rows.append(np.append(timing(), (time.perf_counter() - t0) * 1e3))
        up, sel, gat, row, _, wall = np.min(np.array(rows), axis=0)
        show(what='affinities', npoints=n, ndim=a.ndim, k=k, upload_ms=up, select_ms=sel, gather_ms=gat, sort_search_ms=row, wall_ms=wall,
             select_pairs_per_s=64.0 * n * n / (sel * 1e-3), select_share_of_f64_rate=64.0 * n * n * (3 * a.ndim - 1) / (sel * 1e-3) / F64_RATE)
        y = 10.0 * rng.standard_normal((n, a.ncomp))
        rows = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            manifold.gradient(nbr, pc, y, 12.0)
            rows.append(np.append(timing(), (time.perf_counter() - t0) * 1e3))
        setup, att, pairs, join, _, wall = np.min(np.array(rows), axis=0)
        show(what='gradient', npoints=n, k=k, ncomp=a.ncomp, setup_ms=setup, attract_ms=att, pairs_ms=pairs, join_ms=join, wall_ms=wall,
             pairs_per_s=float(n) * n / (pairs * 1e-3), edges_per_s=2.0 * n * k / (att * 1e-3))
        up_, ga_ = np.zeros_like(y), np.ones_like(y)
        manifold.descend(nbr, pc, y, up_, ga_, 20, 12.0, 0.5, 200.0)
        ms = timing()
        show(what='descend', npoints=n, k=k, ncomp=a.ncomp, steps=20, ms_per_step=ms[4] / 20, first_step_ms=float(ms[1] + ms[2] + ms[3]))
        del nbr, pc
    pn, tn, sn = a.grid
    n = pn * tn * sn
    x = two_phase(n, a.ndim, np.random.default_rng(257))
    if not a.no_device:
        t0 = time.perf_counter()
        y, beta, trace = manifold.embed(x, a.ncomp, float(sn), 24.0, 200.0, a.iterations, min(250, a.iterations))
        wall = time.perf_counter() - t0
        show(what='stage', npoints=n, perplexity=sn, k=manifold.neighbours(n, sn), iterations=a.iterations, wall_s=wall, kl=float(trace[-1, 0]),
             trustworthiness=trust(x, y, a.sample, np.random.default_rng(258)), sample=min(a.sample, n))
    if a.host:
        from sklearn.manifold import TSNE
        t0 = time.perf_counter()
        sk = TSNE(n_components=a.ncomp, perplexity=float(sn), early_exaggeration=24.0, learning_rate=200.0, max_iter=a.iterations, init='pca',
                  method='barnes_hut', n_jobs=THREADS)
        ys = sk.fit_transform(x)
        wall = time.perf_counter() - t0
        show(what='sklearn barnes_hut', npoints=n, perplexity=sn, iterations=int(sk.n_iter_), threads=THREADS, wall_s=wall, kl=float(sk.kl_divergence_),
             trustworthiness=trust(x, ys, a.sample, np.random.default_rng(258)), sample=min(a.sample, n))
    return 0


if __name__ == '__main__':
    sys.exit(main())
