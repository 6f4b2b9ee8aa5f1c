"""The cases and inputs of tests/golden/ref_scan.json, for its maker (tests/golden/make_golden_scan.py, run once at the commit
whose bytes the fixture pins) and for tests/test_scan_golden_gpu.py: the sizes that cross every edge of the all-pairs skeleton of
csrc/nm_scan.h, and points from a closed integer formula, so the inputs depend on no random-number library and on no version of one.

points(): a 64-bit linear congruential generator in Python integers (Knuth's MMIX constants), the top 23 bits of a state mapped to
a multiple of 2^-20 in [-4, 4).  Seven points of eight lie in two blobs, an eighth of that wide, around -1.5 and +1.5 on every
axis (even and odd index); every eighth point is scattered over the whole cube.  Every value is a dyadic rational far inside
float64, so the arrays are exact."""
import hashlib

import numpy as np

from neuralmelting_amd import _lib as B

CL_TILE, CL_ROWS = 256, 512                     # csrc/nm_cluster.h
TS_TILE, TS_ROWS = 128, 512                     # csrc/nm_tsne.h

CL_N = (1, 255, 256, 257, 511, 513, 2 * CL_ROWS + CL_TILE + 7)
CL_ND = (1, 3, 16)
CL_EPS = {1: 2.0 ** -7, 3: 0.125, 16: 1.0}      # core, border and noise points occur at every N >= 255 (the maker asserts it)
CL_MIN_PTS = 4

AF_N = (3, 127, 128, 129, 511, 513, 2 * TS_ROWS + TS_TILE + 7)
AF_ND = (1, 2, 16)

GR_N = (129, 513, 2 * TS_ROWS + TS_TILE + 7)    # on the lists of AF_ND's last
GR_NC = (1, 2, 3)
GR_EXAGGERATION, GR_STEPS, GR_MOMENTUM, GR_RATE = 12.0, 5, 0.5, 200.0

_A, _C, _M = 6364136223846793005, 1442695040888963407, (1 << 64) - 1


def points(n, nd, seed):
    """(n, nd) float64 of the formula above; `seed` picks the stream"""
    s = (seed * 0x9E3779B97F4A7C15 + 1) & _M
    vals = []
    for _ in range(n * nd):
        s = (s * _A + _C) & _M
        vals.append((s >> 41) - (1 << 22))
    u = np.array(vals, dtype=np.int64).reshape(n, nd)
    i = np.arange(n)[:, None]
    blob = np.where(i % 2 == 0, -3, 3) * (1 << 22) + u          # in units of 2^-23: centre -+1.5, u / 8
    x = np.where(i % 8 == 7, 8 * u, blob) * 2.0 ** -23
    return np.ascontiguousarray(x, dtype=np.float64)


def affinity_k(n):
    return min(n - 1, 9)


def digest(a):
    """the shape and the SHA-256 of an output's bytes"""
    assert a.dtype in (np.int32, np.float64) and a.flags.c_contiguous
    return {'shape': list(a.shape), 'sha256': hashlib.sha256(a.tobytes()).hexdigest()}


def _dp(a):
    return a.ctypes.data_as(B.c_double_p)


def _ip(a):
    return a.ctypes.data_as(B.c_int32_p)


# ---- the cases: every output by name, through the raw ABI on sentinel-filled arrays
def cluster_key(n, nd):
    return 'cluster_n%d_nd%d' % (n, nd)


def cluster_case(n, nd):
    L = B.load()
    x = points(n, nd, 1000 * nd + n)
    label, degree, ncl = np.full(n, -77, np.int32), np.full(n, -77, np.int32), np.full(1, -77, np.int32)
    rc = L.nm_cluster_dbscan(0, n, nd, _dp(x), CL_EPS[nd], CL_MIN_PTS, _ip(label), _ip(degree), _ip(ncl))
    assert rc == B.NM_OK, L.nm_cluster_last_error().decode()
    return {'label': label, 'degree': degree, 'nclusters': ncl}


def affinity_key(n, nd):
    return 'affinities_n%d_nd%d' % (n, nd)


def affinity_call(n, nd):
    """rc, the message, and the outputs of nm_tsne_affinities at k = min(n - 1, 9), perplexity k / 3"""
    L = B.load()
    x, k = points(n, nd, 2000 * nd + n), affinity_k(n)
    nbr, p, beta = np.full((n, k), -77, np.int32), np.full((n, k), -77.0), np.full(n, -77.0)
    rc = L.nm_tsne_affinities(0, n, nd, _dp(x), k / 3.0, k, _ip(nbr), _dp(p), _dp(beta))
    return rc, (L.nm_tsne_last_error().decode() if rc else ''), {'nbr': nbr, 'p': p, 'beta': beta}


def gradient_key(n, nc):
    return 'gradient_n%d_nc%d' % (n, nc)


def gradient_case(n, nc, lists):
    """one nm_tsne_gradient and GR_STEPS steps of nm_tsne_descend from points(n, nc) on `lists`, the outputs of affinity_call(n, AF_ND[-1])"""
    L = B.load()
    nbr, p, k = lists['nbr'], lists['p'], affinity_k(n)
    y0 = points(n, nc, 3000 * nc + n)
    grad, kl, z = np.full((n, nc), -77.0), np.full(1, -77.0), np.full(1, -77.0)
    rc = L.nm_tsne_gradient(0, n, k, _ip(nbr), _dp(p), nc, _dp(y0), GR_EXAGGERATION, _dp(grad), _dp(kl), _dp(z))
    assert rc == B.NM_OK, L.nm_tsne_last_error().decode()
    y, update, gains, trace = y0.copy(), np.zeros((n, nc)), np.ones((n, nc)), np.full((GR_STEPS, 3), -77.0)
    rc = L.nm_tsne_descend(0, n, k, _ip(nbr), _dp(p), nc, _dp(y), _dp(update), _dp(gains), GR_STEPS, GR_EXAGGERATION, GR_MOMENTUM, GR_RATE, _dp(trace))
    assert rc == B.NM_OK, L.nm_tsne_last_error().decode()
    return {'grad': grad, 'kl': kl, 'z': z, 'y': y, 'update': update, 'gains': gains, 'trace': trace}
