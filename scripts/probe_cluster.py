"""Where the time of the cluster stage goes: nm_cluster_dbscan on two Gaussian blobs, split by
nm_cluster_last_timing's device events into the upload and screen, the degree pass, the union pass, the numbering and the border
pass; each scan beside the float64 vector rate of the part.  eps is chosen from a sample of the distances for a mean degree of a
few hundred, and again for a few ten thousand: the dense case, where a cluster has N x degree edges for the union pass.  At the
small size only: one scan (the degrees) restated in numpy in chunks on 16 threads, and sklearn's brute-force DBSCAN where it
imports and its neighbourhoods fit the memory (the sparse case).

    python scripts/probe_cluster.py [--npoints 65536 1048576] [--ndim 2 8] [--degrees 300 30000] [--repeats 2] [--no-host]
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralmelting_amd import _lib as B  # noqa: E402
from neuralmelting_amd import cluster  # noqa: E402

ROWS = 512                                  # csrc/nm_cluster.h: CL_ROWS
F64_RATE = 256 * 4 * 16 * 2.4e9             # float64 vector operations per second: 256 CUs x 4 SIMDs x 16 lanes per clock at 2.4 GHz
#                                             (a fused multiply-add counts once: 39.3e12, the 78.6 Tflop/s of DESIGN.md §9 f-2)
HOST_N = 65536                              # the size at which the host's implementations are timed
THREADS = 16


def timing():
    ms = np.zeros(5)
    B.load().nm_cluster_last_timing(ms.ctypes.data_as(B.c_double_p))
    return ms


def two_blobs(n, nd, rng):
    x = rng.standard_normal((n, nd))
    x[n // 2:, 0] += 6.0
    return x[rng.permutation(n)]


def eps_for(x, degree, rng):
    """the radius within which a point of x has `degree` points on average, from 512 x 8192 sampled distances"""
    a, b = x[rng.choice(x.shape[0], 512, replace=False)], x[rng.choice(x.shape[0], 8192, replace=False)]
    d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2)
    return float(np.sqrt(np.quantile(d2, min(1.0, degree / x.shape[0]))))


def numpy_degrees(x, eps, rows=512):
    """one scan of the stage on the host: the degrees, THREADS chunks of rows at a time"""
    e2 = eps * eps

    def chunk(r0):
        d2 = np.zeros((min(rows, x.shape[0] - r0), x.shape[0]))
        for c in range(x.shape[1]):
            d = x[r0:r0 + rows, None, c] - x[None, :, c]
            d2 += d * d
        return (d2 <= e2).sum(axis=1)
    with ThreadPoolExecutor(THREADS) as pool:
        return np.concatenate(list(pool.map(chunk, range(0, x.shape[0], rows)))).astype(np.int32)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--npoints', type=int, nargs='+', default=[65536, 1048576])
    p.add_argument('--ndim', type=int, nargs='+', default=[2, 8])
    p.add_argument('--degrees', type=float, nargs='+', default=[300, 30000])
    p.add_argument('--min_pts', type=int, default=5)
    p.add_argument('--repeats', type=int, default=2)
    p.add_argument('--no-host', action='store_true')
    a = p.parse_args()
    rng = np.random.default_rng(256)
    cluster.dbscan(two_blobs(4096, 2, rng), 0.1, a.min_pts)                 # the warm-up: the library and its kernels are loaded
    for n in a.npoints:
        for nd in a.ndim:
            x = two_blobs(n, nd, rng)
            for want in a.degrees:
                eps = eps_for(x, want, rng)
                rows = []
                for _ in range(a.repeats):
                    t0 = time.perf_counter()
                    label, degree, ncl = cluster.dbscan(x, eps, a.min_pts)
                    rows.append(np.append(timing(), (time.perf_counter() - t0) * 1e3))
                up, deg, uni, num, bor, wall = np.min(np.array(rows), axis=0)
                ops = 2.0 * nd + 1.0
                blocks = -(-n // ROWS)
                tri = sum(min(n, (b + 1) * ROWS) for b in range(blocks)) * float(ROWS)        # the pairs of the union pass, tiles rounded away
                core = degree >= a.min_pts
                res = dict(npoints=n, ndim=nd, eps=eps, mean_degree=float(degree.mean()), nclusters=ncl, core=int(core.sum()),
                           noise=int((label < 0).sum()), repeats=a.repeats, upload_ms=up, degree_ms=deg, union_ms=uni, numbering_ms=num,
                           border_ms=bor, wall_ms=wall,
                           degree_share_of_f64_rate=ops * n * n / (deg * 1e-3) / F64_RATE,
                           union_share_of_f64_rate=ops * min(tri, float(n) * n) / (uni * 1e-3) / F64_RATE,
                           border_rows=int((~core).sum()))
                if not a.no_host and n == HOST_N:
                    t0 = time.perf_counter()
                    ref = numpy_degrees(x, eps)
                    res['numpy_degree_scan_ms'] = (time.perf_counter() - t0) * 1e3
                    res['numpy_threads'] = THREADS
                    res['degrees_differ_from_numpy'] = int((ref != degree).sum())
                    if degree.sum() * 8 < 2e9:                                  # sklearn holds every neighbourhood at once
                        try:
                            from sklearn.cluster import DBSCAN
                            t0 = time.perf_counter()
                            sk = DBSCAN(eps=eps, min_samples=a.min_pts, algorithm='brute', n_jobs=THREADS).fit(x)
                            res['sklearn_brute_ms'] = (time.perf_counter() - t0) * 1e3
                            res['labels_differ_from_sklearn'] = int((sk.labels_ != label).sum())
                        except ImportError:
                            res['sklearn_brute_ms'] = None
                    else:
                        res['sklearn_brute_ms'] = 'left out: its neighbourhoods would take %.3g GB' % (degree.sum() * 8 / 1e9)
                print(json.dumps({k: (float('%.5g' % v) if isinstance(v, float) else v) for k, v in res.items()}))
                sys.stdout.flush()
    return 0


if __name__ == '__main__':
    sys.exit(main())
