"""Where the time of the spectral embedding goes: nm_cluster_spectral on two concentric rings (radii 1 and 3,
radial noise 0.05, gamma 5) of 2^13, 2^15 and 2^17 points, two wanted eigenvectors, block 16, filter degree 8, tol 1e-6.
nm_cluster_spectral_last_timing's device events split the call into the upload and screen, the degree pass, the operator passes, the
block reductions and applies, and the host's small matrices with their transfers; the wall time of the whole call stands beside
them.  A pass is npoints^2 affinities (a distance, one exp, 16 multiply-adds each), so the time of a pass over npoints^2 is the
figure to compare between sizes.  After a warm-up at 4096 points every size runs --repeats times and the fastest call is reported.
Without a GPU it fails: the library has no fallback.

    python scripts/probe_spectral.py [--npoints 8192 32768 131072] [--block 16] [--degree 8] [--tol 1e-6] [--repeats 2]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from neuralmelting_amd import _lib as B  # noqa: E402
from neuralmelting_amd import cluster  # noqa: E402

GAMMA = 5.0


def timing():
    ms = np.zeros(5)
    B.load().nm_cluster_spectral_last_timing(ms)
    return ms


def rings(n, rng):
    """two rings, the points alternating between them, evenly spaced angles jittered by a quarter of their spacing"""
    i = np.arange(n)
    inner = i % 2 == 0
    angle = 2.0 * np.pi * ((i // 2) + 0.25 * rng.uniform(-1.0, 1.0, n)) / np.where(inner, (n + 1) // 2, n // 2)
    radius = np.where(inner, 1.0, 3.0) + 0.05 * rng.standard_normal(n)
    return np.stack([radius * np.cos(angle), radius * np.sin(angle)], axis=1), inner


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--npoints', type=int, nargs='+', default=[2 ** 13, 2 ** 15, 2 ** 17])
    p.add_argument('--block', type=int, default=16)
    p.add_argument('--degree', type=int, default=8)
    p.add_argument('--tol', type=float, default=1e-6)
    p.add_argument('--max_pass', type=int, default=2000)
    p.add_argument('--repeats', type=int, default=2)
    a = p.parse_args()
    rng = np.random.default_rng(256)
    warm = rings(4096, rng)[0]
    cluster.spectral(warm, GAMMA, 2, rng.standard_normal((4096, a.block)), a.degree, 100, a.tol)      # the library and its kernels are loaded
    for n in a.npoints:
        x, inner = rings(n, rng)
        init = rng.standard_normal((n, a.block))
        rows = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            embed, eigval, resid, deg, passes, status = cluster.spectral(x, GAMMA, 2, init, a.degree, a.max_pass, a.tol)
            rows.append(np.append(timing(), (time.perf_counter() - t0) * 1e3))
        up, degree, operator, block, host, wall = np.min(np.array(rows), axis=0)
        off = embed - embed.mean(axis=0)                                    # two tight clusters: the side of the mean along the main axis
        side = off @ np.linalg.eigh(off.T @ off)[1][:, -1] > 0.0
        res = dict(npoints=n, block=a.block, degree=a.degree, tol=a.tol, repeats=a.repeats, passes=passes, status=status,
                   eigval=[float('%.8f' % v) for v in eigval[:4]], resid=float(resid[:2].max()), upload_ms=up, degree_ms=degree,
                   operator_ms=operator, block_ms=block, host_ms=host, wall_ms=wall, ms_per_pass=operator / passes,
                   ns_per_affinity_of_the_degree_pass=degree * 1e6 / n ** 2, ns_per_affinity_of_a_pass=operator / passes * 1e6 / n ** 2,
                   share_outside_the_passes=1.0 - (degree + operator) / wall, rings_found=bool((side == inner).all() or (side != inner).all()))
        print(json.dumps({k: (float('%.5g' % v) if isinstance(v, float) else v) for k, v in res.items()}))
        sys.stdout.flush()
    return 0


if __name__ == '__main__':
    sys.exit(main())
