"""The sizes at which a workgroup of the all-pairs scans (csrc/nm_scan.h) walks several tiles, their inputs and their references,
for tests/test_scan_big.py (the regimes, on the CPU) and tests/test_scan_big_gpu.py (the kernels).  scan_grid() restates the host's
choice of the grid with the constants read from the headers, so a change of a GRID, a SPAN, a tile or a row block fails the
regime assertions instead of moving the cases back to one tile per workgroup without a word.

Every input lies on the dyadic grid G of tests/test_cluster_gpu.py: coordinates are integers times G, so every d2 and eps^2 is
exact, pairs exactly on the bound and ties at the k-th distance occur, and the KD-tree references decide them as the kernels do."""
import functools
import os
import re

import numpy as np

import scan_big_ref as K

G = 2.0 ** -8
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'neuralmelting_amd', 'csrc')


@functools.lru_cache(maxsize=None)
def shape(stage):
    """{'ROWS', 'TILE', 'GRID', 'SPAN'} of 'cluster' or 'tsne', read from the stage's header"""
    name, pre = {'cluster': ('nm_cluster.h', 'CL'), 'tsne': ('nm_tsne.h', 'TS')}[stage]
    src = open(os.path.join(CSRC, name)).read()
    const = {k: v for k, v in re.findall(r'constexpr int %s_(\w+) = ([^;]+);' % pre, src)}
    assert const['ROWS'] == '%s_RPT * %s_BLOCK' % (pre, pre)
    assert 'ScanShape<%s_BLOCK, %s_RPT, %s_TILE, %s_GRID, %s_SPAN>' % ((pre,) * 5) in src
    return dict(ROWS=int(const['RPT']) * int(const['BLOCK']), TILE=int(const['TILE']), GRID=int(const['GRID']), SPAN=int(const['SPAN']))


def scan_grid(stage, nrows, n):
    """csrc/nm_scan.h's scan_grid: dict(blocks, tiles, slices, limb, walk); limb names the term that set the slices ('GRID', 'SPAN',
    or 'TILES' where the cap of one slice per tile did), walk = (fewest, most) tiles that a slice walks"""
    s = shape(stage)
    blocks, tiles = -(-nrows // s['ROWS']), -(-n // s['TILE'])
    by_grid, by_span = -(-s['GRID'] // blocks), -(-tiles // s['SPAN'])
    slices, limb = (by_grid, 'GRID') if by_grid >= by_span else (by_span, 'SPAN')
    if slices >= tiles:
        slices, limb = tiles, 'TILES'
    walk = [len(range(first, tiles, slices)) for first in range(slices)]        # slice `first` walks first, first + slices, ...
    return dict(blocks=blocks, tiles=tiles, slices=slices, limb=limb, walk=(min(walk), max(walk)), last=n - (tiles - 1) * s['TILE'])


# ---- the cluster stage
# n: (row blocks, tiles, slices, limb, tiles per slice, columns of the last tile, fewest points that are not core or None)
CLUSTER_REGIME = {
    16392: (33, 65, 63, 'GRID', (1, 2), 8, None),
    40007: (79, 157, 26, 'GRID', (6, 7), 71, 6657),
    196616: (385, 769, 7, 'SPAN', (109, 110), 8, 151041),
}
# (n, nd): sigma of a blob in grid steps, eps in grid steps, min_pts
CLUSTER_CASES = {
    (16392, 1): (1200, 2, 5), (16392, 2): (40, 2, 6), (16392, 3): (10, 2, 6), (16392, 16): (40, 6, 6),
    (40007, 1): (4500, 2, 5), (40007, 2): (60, 2, 6), (40007, 3): (12, 2, 6),
    (196616, 1): (90000, 2, 4), (196616, 2): (260, 2, 4),
}
PLANE = 16          # nd = 16 is an integer plane in 16 dimensions


def cluster_key(case):
    return 'N%d-nd%d' % case


@functools.lru_cache(maxsize=None)
def cluster_points(n, nd):
    """three blobs of width sigma and a scattered tenth, in whole grid steps, shuffled; nd = 16: a 2-D set z of that kind times an
    integer matrix A (2, 16), a plane on which the KD-tree stays fast"""
    sigma, eps, min_pts = CLUSTER_CASES[(n, nd)]
    rng = np.random.default_rng(1000 * nd + n)
    zd = 2 if nd == PLANE else nd
    centre = rng.uniform(-6.0 * sigma, 6.0 * sigma, (3, zd))
    z = centre[rng.integers(0, 3, n)] + sigma * rng.standard_normal((n, zd))
    z[: n // 10] = rng.uniform(-10.0 * sigma, 10.0 * sigma, (n // 10, zd))
    z = np.round(z[rng.permutation(n)])
    if nd == PLANE:
        a = rng.integers(-1, 2, (2, PLANE)).astype(np.float64)
        a[0] = np.where(a[0] == 0.0, 1.0, a[0]) * (np.arange(PLANE) < 9)        # |a[0]| = 3: two steps along z[0] are eps = 6 exactly
        z = z @ a
    assert np.abs(z).max() < 2 ** 22                            # d2 in steps^2 stays far below 2^53
    x = np.ascontiguousarray(z * G)
    x.setflags(write=False)
    return x, eps * G, min_pts


@functools.lru_cache(maxsize=None)
def cluster_reference(n, nd):
    x, eps, min_pts = cluster_points(n, nd)
    label, degree, ncl = K.dbscan_kd(x, eps, min_pts)
    for a in (label, degree):
        a.setflags(write=False)
    return label, degree, ncl


CHAIN_N = (16392, 40007)


def chain(n, shuffled):
    """points one link of four grid steps apart along a line in the plane, eps one link: (x, eps, the position of every point)"""
    pos = np.random.default_rng(3).permutation(n) if shuffled else np.arange(n)
    return np.stack([pos * (4 * G), np.full(n, 0.5)], axis=1), 4 * G, pos


def chain_reference(n, pos, min_pts):
    """closed form: the two ends see one neighbour and themselves, the others two; at min_pts 2 and 3 one cluster holds every point
    (the ends are core at 2 and borders at 3)"""
    assert min_pts in (2, 3)
    degree = (3 - (pos == 0) - (pos == n - 1)).astype(np.int32)
    return np.zeros(n, dtype=np.int32), degree, 1


# ---- the manifold stage
# n: (row blocks, tiles, slices, limb, tiles per slice)
TSNE_REGIME = {
    12297: (25, 97, 82, 'GRID', (1, 2)),
    24583: (49, 193, 42, 'GRID', (4, 5)),
    196616: (385, 1537, 7, 'SPAN', (219, 220)),
}
AF_N, AF_ND, AF_K = (12297, 24583), (1, 2, 3), (9, 65)
AF_SIGMA = {1: 3000, 2: 40, 3: 16}         # grid steps: a point per grid location or fewer at a blob's centre, so that the ties
                                           # at one distance fit into the candidates of neighbours_kd (test_scan_big.py asserts it)
RING_N, RING_K = 196616, (1, 3)
LOCATIONS = 48


@functools.lru_cache(maxsize=None)
def affinity_points(n, nd):
    """three blobs in whole grid steps, one point in fifty a copy of another: duplicates, and ties at every distance"""
    rng = np.random.default_rng(2000 * nd + n)
    sigma = AF_SIGMA[nd]
    centre = rng.uniform(-6.0 * sigma, 6.0 * sigma, (3, nd))
    z = np.round(centre[rng.integers(0, 3, n)] + sigma * rng.standard_normal((n, nd)))
    z = z[rng.permutation(n)]
    z[rng.permutation(n)[: n // 50]] = z[rng.integers(0, n, n // 50)]
    x = np.ascontiguousarray(z * G)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def affinity_reference(n, nd, k):
    """(nbr, complete, tied): the lists, whether they may be used, and the rows whose k-th and (k + 1)-th distance are equal"""
    nbr, complete, tied = K.neighbours_kd(affinity_points(n, nd), k)
    nbr.setflags(write=False)
    return nbr, complete, tied


def grouped_embedding(n, nc, scale, seed):
    """(centres (LOCATIONS, nc), member (n,)): y = centres[member], every location taken, the members shuffled"""
    rng = np.random.default_rng(seed)
    centres = scale * rng.standard_normal((LOCATIONS, nc))
    member = np.concatenate([np.arange(LOCATIONS), rng.integers(0, LOCATIONS, n - LOCATIONS)])
    return centres, member[rng.permutation(n)]


SCALES = {'start': 1e-4, 'wide': 10.0}     # tests/test_tsne_gpu.py's embeddings()


def ring_lists(n, k, seed=3):
    """hand-made lists: row i lists i + 1 .. i + k around a ring, with random conditional probabilities"""
    nbr = np.ascontiguousarray((np.arange(n)[:, None] + np.arange(1, k + 1)[None, :]) % n, dtype=np.int32)
    p = np.random.default_rng(seed).random((n, k)) + 0.01
    return nbr, p / p.sum(axis=1, keepdims=True)
