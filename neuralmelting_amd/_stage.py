"""What the stages behind the driver share: the prefix of a run's files, and the front of the stages that work on one array over
the whole replica grid (pca, manifold, cluster): their inputs, the kept samples of every grid point, and the way back."""
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
