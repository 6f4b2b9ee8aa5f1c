"""Where the time of the principal component stage goes: nm_pca_moments and nm_pca_project on random float32
data of the production width, split by nm_pca_last_timing's device events into the upload, the first pass, the Gram pass and the
projection; beside it numpy's float64 a.T @ a on the host's threads, the only other implementation of this product at hand.

    python scripts/probe_pca.py [--nsamples 262144 1048576] [--nfeat 1331] [--ncomp 8] [--repeats 3] [--no-numpy]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralmelting_amd import _lib as B  # noqa: E402
from neuralmelting_amd import pca  # noqa: E402

TILE = 64       # csrc/nm_pca.h


def timing():
    ms = np.zeros(4)
    B.load().nm_pca_last_timing(ms.ctypes.data_as(B.c_double_p))
    return ms


def numpy_gram(x, rows=65536):
    """the same product in float64 on the host, 65536 rows at a time so that the float64 copy stays small"""
    m = x.mean(axis=0, dtype=np.float64)
    g = np.zeros((x.shape[1], x.shape[1]))
    for r0 in range(0, x.shape[0], rows):
        a = x[r0:r0 + rows].astype(np.float64) - m
        g += a.T @ a
    return g


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--nsamples', type=int, nargs='+', default=[262144, 1048576])
    p.add_argument('--nfeat', type=int, default=1331)
    p.add_argument('--ncomp', type=int, default=8)
    p.add_argument('--repeats', type=int, default=3)
    p.add_argument('--no-numpy', action='store_true')
    a = p.parse_args()
    d = a.nfeat
    tiles = -(-d // TILE)
    ntri = tiles * (tiles + 1) // 2
    rng = np.random.default_rng(256)
    for n in a.nsamples:
        try:
            x = rng.random((n, d), dtype=np.float32)
        except MemoryError:
            print('%d x %d: no host memory for it, left out' % (n, d))
            continue
        comp = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((d, a.ncomp)))[0].T)
        rows = []
        for rep in range(a.repeats + 1):            # the first call is the warm-up and is not counted
            t0 = time.perf_counter()
            mean, lo, hi, gram = pca.moments(x)
            wall_m = time.perf_counter() - t0
            tm = timing()
            t0 = time.perf_counter()
            z, norm2 = pca.project(x, mean, np.ones(d), comp)
            wall_p = time.perf_counter() - t0
            tp = timing()
            if rep:
                rows.append([tm[0], tm[1], tm[2], wall_m * 1e3, tp[0], tp[3], wall_p * 1e3])
        up, colsum, gramms, wall_m, up_p, proj, wall_p = np.median(np.array(rows), axis=0)
        spread = np.ptp(np.array(rows), axis=0)
        res = dict(nsamples=n, nfeat=d, ncomp=a.ncomp, repeats=a.repeats,
                   upload_ms=up, upload_GBps=n * d * 4 / up / 1e6, colsum_ms=colsum, colsum_GBps=n * d * 4 / colsum / 1e6,
                   gram_ms=gramms, gram_executed_Tflops=2.0 * n * TILE * TILE * ntri / gramms / 1e9,
                   gram_useful_Tflops=1.0 * n * d * (d + 1) / gramms / 1e9,
                   moments_wall_ms=wall_m, upload_share_of_moments=up / (up + colsum + gramms),
                   project_upload_ms=up_p, project_ms=proj, project_GBps=n * d * 4 / proj / 1e6, project_wall_ms=wall_p,
                   spread_ms=dict(upload=float('%.3g' % spread[0]), colsum=float('%.3g' % spread[1]), gram=float('%.3g' % spread[2]), project=float('%.3g' % spread[5])))
        if not a.no_numpy:
            t0 = time.perf_counter()
            ref = numpy_gram(x)
            res['numpy_gram_ms'] = (time.perf_counter() - t0) * 1e3
            res['numpy_threads'] = int(os.environ.get('OMP_NUM_THREADS', 0))
            res['gram_vs_numpy_max_rel'] = float(np.abs(gram - ref).max() / np.abs(ref).max())
        print(json.dumps({k: (float('%.5g' % v) if isinstance(v, float) else v) for k, v in res.items()}))
        sys.stdout.flush()
        del x, z, gram
    return 0


if __name__ == '__main__':
    sys.exit(main())
