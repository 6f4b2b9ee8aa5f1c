"""What the stages behind the driver share: the prefix of a run's files, and the front of the stages that work on one array over
the whole replica grid (pca, outlier, manifold, cluster): their inputs, the kept samples of every grid point, the way back, and
for `-il` the mask of the inliers that `outlier` found among them."""
import os

import numpy as np

LAT = {'Ti': 'bcc', 'Al': 'fcc', 'Ni': 'fcc', 'Cu': 'fcc', 'LJ': 'fcc'}


def prefix(name, element):
    """<cwd>/<name>.<element>.<lattice>.lammps, what every file of a run starts with"""
    return os.getcwd() + '/' + '%s.%s.%s.lammps' % (name, element.lower(), LAT[element])


def grid_inputs(stage, pre, key, tail, more_axes=False):
    """(P, T, pe, values, path): the target grid, <pre>.pe.npy (PN, TN, SN) and <pre>.<key>.npy (PN, TN, SN, one axis; with
    more_axes at least one), the two large ones as memory maps, and the latter's path.  Every input is checked before a stage
    writes anything: SystemExit in the name of `stage`, `tail` saying what follows the sample axis."""
    paths = {k: pre + '.%s.npy' % k for k in ('virial.trgt', 'temp.trgt', 'pe', key)}
    for path in paths.values():
        if not os.path.isfile(path):
            raise SystemExit('%s: %s is missing' % (stage, path))
    P, T, pe = np.load(paths['virial.trgt']), np.load(paths['temp.trgt']), np.load(paths['pe'], mmap_mode='r')
    values = np.load(paths[key], mmap_mode='r')
    if pe.ndim != 3 or pe.shape[:2] != (P.size, T.size):
        raise SystemExit('%s: %s has shape %s and does not fit the %d x %d grid' % (stage, paths['pe'], pe.shape, P.size, T.size))
    if (values.ndim < 4 if more_axes else values.ndim != 4) or values.shape[:3] != pe.shape:
        raise SystemExit('%s: %s has shape %s, not %s followed by %s' % (stage, paths[key], values.shape, pe.shape, tail))
    return P, T, pe, values, paths[key]


def kept(values, skip, stride):
    """(how many, which): the samples skip, skip + stride, ... of every grid point of values (PN, TN, SN, ...)"""
    return len(range(skip, values.shape[2], stride)), values[:, :, skip::stride]


def spread(values, shape, skip, stride, fill):
    """values (PN, TN, kept, ...) of the samples skip, skip + stride, ... in an array of `shape` (PN, TN, SN, ...) filled with `fill`"""
    out = np.full(shape, fill, dtype=np.asarray(values).dtype)
    out[:, :, skip::stride] = values
    return out


def inliers(stage, pre, feature, shape, skip, stride):
    """the keep-mask (PN, TN, kept), bool, of the samples skip, skip + stride, ... that `outlier` called inliers: <pre>.<feature>.loi.npy
    is not 0 there.  <pre>.<feature>.lof.npy must be NaN at exactly the samples that skip and stride leave out: SystemExit in the
    name of `stage` otherwise, or where a file is missing or not of `shape` (PN, TN, SN)."""
    lof, loi = (pre + '.%s.%s.npy' % (feature, key) for key in ('lof', 'loi'))
    for path in (lof, loi):
        if not os.path.isfile(path):
            raise SystemExit('%s: %s is missing: -il wants the outlier stage to have run' % (stage, path))
    factor, keep = np.load(lof), np.load(loi)
    for path, a in ((lof, factor), (loi, keep)):
        if a.shape != tuple(shape):
            raise SystemExit('%s: %s has shape %s, not %s' % (stage, path, a.shape, tuple(shape)))
    left_out = np.ones(shape[2], dtype=bool)
    left_out[skip::stride] = False
    if not np.array_equal(np.isnan(factor), np.broadcast_to(left_out, shape)):
        raise SystemExit('%s: -sk %d -sd %d are not those that %s was written with' % (stage, skip, stride, lof))
    return keep[:, :, skip::stride] != 0


def spread_kept(values, keep, shape, skip, stride, fill):
    """values (M, ...) of the M samples that keep (PN, TN, kept) marks, in their order, in an array of `shape` (PN, TN, SN, ...)
    filled with `fill`: the way back of x[keep] for x = kept(...)[1]"""
    out = np.full(shape, fill, dtype=np.asarray(values).dtype)
    out[:, :, skip::stride][keep] = values                               # (a view of out: the assignment lands in it)
    return out
