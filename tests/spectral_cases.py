"""The inputs that tests/test_spectral.py and tests/test_spectral_gpu.py share: seeded generators of points, the cases of the GPU
tests with their references, and the raw call of nm_cluster_spectral on sentinel-filled outputs."""
import functools

import numpy as np

import spectral_ref as R
from neuralmelting_amd import _lib as B

SENT = -77
OUTPUTS = ('embed', 'eigval', 'resid', 'deg', 'info')
TILE, ROWS, GRID, SPAN = 128, 512, 2048, 1024       # csrc/nm_spectral.h: columns of a tile, rows of a workgroup, workgroups aimed at, tiles walked at most
SIZES = (2, 3, TILE - 1, TILE, TILE + 1, ROWS - 1, ROWS + 1, 2 * ROWS + TILE + 7)
WIDTHS = ((1, 1), (2, 5), (3, 8), (8, 16))         # (ncomp, nblock): the widths 1, a padded 8, 8 and 16
RINGS_GAMMA, BLOBS_GAMMA, WIDE_GAMMA = 5.0, 10.0, 1.0
RINGS_GAP, BLOBS_GAP = 0.001, 0.5


def rings(n, seed):
    """two concentric rings of radii 1 and 3 with radial noise 0.05, the points alternating between them (even: the inner one); the
    angles are evenly spaced and jittered by a quarter of their spacing, so a ring stays connected at every n.  (x (n, 2), inner (n,))"""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    inner = i % 2 == 0
    per = np.where(inner, (n + 1) // 2, max(n // 2, 1))
    angle = 2.0 * np.pi * ((i // 2) + 0.25 * rng.uniform(-1.0, 1.0, n)) / per
    radius = np.where(inner, 1.0, 3.0) + 0.05 * rng.standard_normal(n)
    return np.stack([radius * np.cos(angle), radius * np.sin(angle)], axis=1), inner


CENTRES = np.array([[0.0, 0.0], [1.0, 0.0], [0.5, 0.9]])


def blobs(n, seed):
    """three blobs of sigma 0.08 at (0, 0), (1, 0) and (0.5, 0.9), point i in blob i % 3: (x (n, 2), which (n,))"""
    rng = np.random.default_rng(seed)
    which = np.arange(n) % 3
    return CENTRES[which] + 0.08 * rng.standard_normal((n, 2)), which


def line(n, seed):
    """three blobs of sigma 0.08 at 0, 1 and 2 on a line: (x (n, 1), which (n,))"""
    rng = np.random.default_rng(seed)
    which = np.arange(n) % 3
    return (which + 0.08 * rng.standard_normal(n))[:, None], which


def lifted(x, nd, seed):
    """x (n, 2) in nd >= 2 dimensions by a map with orthonormal columns: every distance, so the whole spectrum, is kept"""
    q = np.linalg.qr(np.random.default_rng(seed).standard_normal((nd, 2)))[0]
    return x @ q.T


def blobs16(n, seed):
    """the same blobs embedded in 16 dimensions"""
    x, which = blobs(n, seed)
    return lifted(x, 16, seed + 1), which


def scan_grid(n):
    """csrc/nm_scan.h's scan_grid for the pass over n points: (row blocks, column slices)"""
    blocks, tiles = (n + ROWS - 1) // ROWS, (n + TILE - 1) // TILE
    slices = max((GRID + blocks - 1) // blocks, (tiles + SPAN - 1) // SPAN)
    return blocks, min(slices, tiles)


@functools.lru_cache(maxsize=None)
def case(n, nd, ncomp):
    """what the GPU tests run for n points in nd dimensions and ncomp wanted eigenvectors: (x, gamma, truth, the dense reference).
    Two wanted: the rings (nd 1: the line); one wanted: the blobs at a gamma that joins them, so that 1 is a simple eigenvalue
    with a gap behind it; else the blobs."""
    seed = 1000 * nd + n
    if nd == 1:
        (x, truth), gamma = line(n, seed), WIDE_GAMMA if ncomp == 1 else BLOBS_GAMMA
    elif ncomp == 2:
        (x, truth), gamma = rings(n, seed), RINGS_GAMMA
    else:
        (x, truth), gamma = blobs(n, seed), WIDE_GAMMA if ncomp == 1 else BLOBS_GAMMA
    if nd > 2:
        x = lifted(x, nd, seed + 1)
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return x, gamma, truth, R.dense(x, gamma)


def start(n, nblock, seed=7):
    """a start block of standard normals"""
    return np.random.default_rng(seed).standard_normal((n, nblock))


def outputs(n, ncomp, nblock, fill=SENT):
    return dict(embed=np.full((n, max(ncomp, 1)), float(fill)), eigval=np.full(max(nblock, 1), float(fill)), resid=np.full(max(nblock, 1), float(fill)),
                deg=np.full(n, float(fill)), info=np.full(2, fill, np.int32))


def untouched(out, fill=SENT):
    return all((v == fill).all() for v in out.values())


def raw(x, gamma, ncomp, init, degree=8, max_pass=2000, tol=1e-8, device=0, null=(), fill=SENT, **over):
    """the raw ABI on sentinel-filled outputs: rc, message, {output: array}.  `over` replaces npoints, ndim or nblock as the library
    is told them (the arrays keep their sizes); `null` names the pointers passed as null"""
    L = B.load()
    x, init = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(init, dtype=np.float64)
    (n, nd), nb = x.shape, init.shape[1]
    out = outputs(n, ncomp, nb, fill)
    rc = L.nm_cluster_spectral(device, over.get('npoints', n), over.get('ndim', nd), None if 'x' in null else x, gamma, ncomp,
                               over.get('nblock', nb), None if 'init' in null else init, degree, max_pass, tol,
                               *[None if name in null else out[name] for name in OUTPUTS])
    return rc, (L.nm_distr_last_error().decode() if rc else ''), out
