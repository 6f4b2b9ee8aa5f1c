"""The inputs that tests/test_kmeans.py and tests/test_kmeans_gpu.py share, and the raw call of nm_cluster_kmeans on sentinel-filled
outputs."""
import numpy as np

from neuralmelting_amd import _lib as B

SENT = -77
G = 2.0 ** -5               # the grid of the exact data: coordinates are multiples of it, |x| <= 64, so every d2 and every sum is exact
OUTPUTS = ('label', 'centre', 'count', 'inertia', 'iters', 'status', 'best')


def blobs(n, nd, seed, k=3):
    """tests/test_cluster_gpu.py's grid_blobs without the rounding: k blobs and a scattered tenth, continuous, |x| < 8"""
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-3.0, 3.0, (k, nd))
    x = centre[rng.integers(0, k, n)] + 0.4 * rng.standard_normal((n, nd))
    x[: n // 10] = rng.uniform(-5.0, 5.0, (n // 10, nd))
    return x[rng.permutation(n)]


def on_grid(x):
    """x rounded to the grid, every zero a +0"""
    return np.round(x / G) * G + 0.0


def drawn(x, k, seed, nrestarts=None):
    """k points of x drawn without replacement as initial centres: (k, ND), or (R, k, ND)"""
    rng = np.random.default_rng(seed)
    if nrestarts is None:
        return x[rng.choice(x.shape[0], k, replace=False)].copy()
    return np.stack([x[rng.choice(x.shape[0], k, replace=False)] for _ in range(nrestarts)])


def outputs(n, nd, k, nr):
    return dict(label=np.full(n, SENT, np.int32), centre=np.full((k, nd), float(SENT)), count=np.full(k, SENT, np.int32),
                inertia=np.full(nr, float(SENT)), iters=np.full(nr, SENT, np.int32), status=np.full(nr, SENT, np.int32),
                best=np.full(1, SENT, np.int32))


def untouched(out):
    return all((v == SENT).all() for v in out.values())


def raw(x, init, max_iter=300, tol=0.0, device=0, null=(), **over):
    """the raw ABI on sentinel-filled outputs: rc, message, {output: array}.  `over` replaces npoints, ndim, k or nrestarts as the
    library is told them (the arrays keep their sizes); `null` names the pointers passed as null"""
    L = B.load()
    x, init = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(init, dtype=np.float64)
    if init.ndim == 2:
        init = init[None]
    (n, nd), (nr, k) = x.shape, init.shape[:2]
    out = outputs(n, nd, k, nr)
    arg = dict(x=x, init=init, **out)
    rc = L.nm_cluster_kmeans(device, over.get('npoints', n), over.get('ndim', nd), None if 'x' in null else arg['x'], over.get('k', k),
                             over.get('nrestarts', nr), None if 'init' in null else arg['init'], max_iter, tol,
                             *[None if name in null else out[name] for name in OUTPUTS])
    return rc, (L.nm_distr_last_error().decode() if rc else ''), out
