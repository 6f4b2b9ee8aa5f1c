"""throughput of nm_distr_histograms (row f-2) next to the numpy restatement of calculate_rdf / calculate_cdf

    python scripts/bench_distr.py [ns=4096] [natoms=256]
    python scripts/bench_distr.py --angles [ns=4096] [cells=4] [cutoff=0.5] [repeats=5]
    python scripts/bench_distr.py --sfactor [ns=4096] [natoms=256] [qmax=16] [repeats=5]
    python scripts/bench_distr.py --bondorder [ns=4096] [cells=4] [cutoff=0] [repeats=5] [l ...=4 6]
    python scripts/bench_distr.py --bond-w [ns=4096] [cells=4] [cutoff=0] [repeats=5] [l ...=4 6]
    python scripts/bench_distr.py --solid [ns=4096] [cells=4] [cutoff=0] [repeats=5] [l=6] [s_min=0.5] [n_min=8]
    python scripts/bench_distr.py --cna [ns=4096] [cells=4] [cutoff=0] [repeats=5] [mode=adaptive]
    python scripts/bench_distr.py --entropy [ns=4096] [cells=4] [repeats=5] [r_m=0] [sigma=0] [nbins=0] [r_avg=0]

--angles: nm_distr_angles on displaced fcc frames of 4 cells^3 atoms (shell up to cutoff * l; the first shell is about
0.85 / cells): the time of the whole call (copies + kernel, host clock around the synchronous call, median of the repeats
after a warm-up), triplets/s, and the numpy restatement (tests/adf_ref.py) on one host core over a few centres.  The
kernel's own time comes from `rocprofv3 --kernel-trace --stats -- python scripts/bench_distr.py --angles ...` (nm_adf_kernel).

--sfactor: nm_distr_sfactor on random liquids: the time of the whole call as above and the rate in the definition's terms, one
complex multiply-add (8 flop) per atom and vector of the half space; the kernel's own time from the same rocprofv3 line
(nm_sfac_kernel).

--bondorder: nm_distr_bondorder on the frames and shapes of --angles (cutoff 0 = the first fcc shell, 0.853553 / cells), all four
outputs: the time of the whole call as above, bonds/s, the same call of nm_distr_angles on the same frames and shell next to it
(the yardstick: it pays for one scan of the candidates, the bond-order path for two plus the harmonics), and the numpy
restatement on one host core over one sample (imported from tests/bondorder_ref.py, as --angles imports tests/adf_ref.py: the
script needs the tests directory next to it).  The kernels' own times come from the same rocprofv3 line
(nm_bo_moments_kernel, nm_bo_average_kernel, nm_bo_global_kernel, nm_adf_kernel).

--bond-w: nm_distr_bondorder_w with all seven outputs on the frames and shapes of --bondorder (even l only), and next to it
nm_distr_bondorder with all four outputs on the same frames, shell and l (the yardstick: the same two scans; the new call adds the three
contractions and three more arrays to copy back): the time of each whole call as above and their ratio.  The kernels' own times come
from the same rocprofv3 line (nm_bo_moments_kernel, nm_bo_w_kernel, nm_bo_w_average_kernel, nm_bo_w_global_kernel against
nm_bo_moments_kernel, nm_bo_average_kernel, nm_bo_global_kernel).

--solid: nm_distr_solid on the frames and shapes of --bondorder, all five outputs: the time of the whole call as above, entries/s,
and next to it nm_distr_bondorder with qbar2 alone for the same single l on the same frames and shell (the yardstick: two scans
of the candidates; the solid path does three and the gather of the bond values).  The kernels' own times come from the same
rocprofv3 line (nm_bo_moments_kernel, nm_solid_connect_kernel, nm_solid_union_kernel, nm_solid_label_kernel).

--cna: nm_distr_cna (mode adaptive or fixed) on the frames of --bondorder, all four outputs (cutoff 0 = distr.cna_radius's automatic
value for the mode): the time of the whole call as above, centres/s and entries/s, the types and columns found, and next to it
nm_distr_solid (l = 6, the defaults) on the same frames and the same shell, the nearest scan-bound sibling (three scans of the
candidates and the moments against this path's one scan and the graphs).  The kernel's own time comes from the same rocprofv3 line
(nm_cna_kernel against nm_bo_moments_kernel + nm_solid_connect_kernel + nm_solid_union_kernel + nm_solid_label_kernel).

--entropy: nm_distr_entropy on the frames of --bondorder at distr -le's automatic parameters (or the fractions given), all six outputs:
the time of the whole call as above, the entries and the Gaussian terms (entries x grid points) per second.  The kernels' own times
come from the same rocprofv3 line (nm_ent_local_kernel, nm_ent_average_kernel, nm_ent_mean_kernel)."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from neuralmelting_amd import distr


def bench_angles(argv):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import adf_ref as A
    from neuralmelting_amd import _lib as B, lattice
    ns = int(argv[0]) if len(argv) > 0 else 4096
    cells = int(argv[1]) if len(argv) > 1 else 4
    cut = float(argv[2]) if len(argv) > 2 else 0.5
    reps = int(argv[3]) if len(argv) > 3 else 5
    rng = np.random.default_rng(3)
    n = 4 * cells ** 3
    a0 = lattice.lattice_constant('LJ')
    box = (cells * a0 * (1.0 + 0.05 * rng.random(ns))).astype(np.float32)
    frac = lattice.fcc_fractional(cells)
    pos = ((frac[None] + 0.08 / cells * rng.normal(size=(ns, n, 3))) % 1.0 * box[:, None, None]).astype(np.float32)
    pos = np.minimum(pos, np.nextafter(box, np.float32(0))[:, None, None])
    l = float(box.min())
    ce = np.ascontiguousarray(np.cos(np.linspace(1e-16, np.pi, 64)))
    L = B.load()
    out = np.zeros((ns, 64), dtype=np.uint64)

    def run(m):
        rc = L.nm_distr_angles(0, m, n, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), 1e-16 * l, cut * l, 64,
                               ce.ctypes.data_as(B.c_double_p), out.ctypes.data_as(B.c_uint64_p))
        if rc != 0:
            raise RuntimeError(L.nm_distr_last_error().decode())
    run(min(ns, 8))
    run(ns)                                                                   # warm-up at the timed shape
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); run(ns); ts.append(time.perf_counter() - t)
    trip = int(out.sum())
    dt = float(np.median(ts))
    print('angles: %d samples x %d atoms, cutoff %.4f l: %d triplets (%.1f neighbours per centre); call (H2D + kernel + D2H) median '
          'of %d: %.4f s (min %.4f, max %.4f) = %.2f G triplets/s' % (ns, n, cut, trip, (1 + np.sqrt(1 + 8 * trip / (ns * n))) / 2,
                                                                       reps, dt, min(ts), max(ts), trip / dt / 1e9))
    kc = min(n, 16)
    t = time.perf_counter()
    nt = 0
    for c in range(kc):
        v = A.neighbours(pos[0], box[0], c, 1e-16 * l, cut * l)
        k = A.cos_bins(ce, A.cosines(v)) if len(v) > 1 else np.zeros(0, dtype=np.int64)
        np.bincount(k[k >= 0], minlength=63)
        nt += len(v) * (len(v) - 1) // 2
    dt = time.perf_counter() - t
    print('numpy restatement, one core, %d centres of sample 0: %.4f s, %.4f G triplets/s, %.2f centres/s' % (kc, dt, nt / dt / 1e9, kc / dt))


def bench_sfactor(argv):
    from neuralmelting_amd import _lib as B
    ns = int(argv[0]) if len(argv) > 0 else 4096
    n = int(argv[1]) if len(argv) > 1 else 256
    qmax = int(argv[2]) if len(argv) > 2 else 16
    reps = int(argv[3]) if len(argv) > 3 else 5
    rng = np.random.default_rng(3)
    box = (6.0 + 0.3 * rng.random(ns)).astype(np.float32)
    pos = (rng.random((ns, n, 3)) * box[:, None, None]).astype(np.float32)
    nvec = int(distr.sfactor_shells(qmax)[1].sum()) // 2
    L = B.load()
    ssum = np.zeros((ns, qmax * qmax + 1))
    smax = np.zeros((ns, qmax * qmax + 1))

    def run(m):
        rc = L.nm_distr_sfactor(0, m, n, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), qmax,
                                ssum.ctypes.data_as(B.c_double_p), smax.ctypes.data_as(B.c_double_p))
        if rc != 0:
            raise RuntimeError(L.nm_distr_last_error().decode())
    run(min(ns, 8))
    run(ns)                                                                   # warm-up at the timed shape
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); run(ns); ts.append(time.perf_counter() - t)
    dt = float(np.median(ts))
    cma = float(ns) * n * nvec
    print('sfactor: %d samples x %d atoms, qmax %d: %d half-space vectors, %.3e complex multiply-adds; call (H2D + kernel + D2H) '
          'median of %d: %.4f s (min %.4f, max %.4f) = %.2f T flop/s at 8 flop each; mean S %.4f'
          % (ns, n, qmax, nvec, cma, reps, dt, min(ts), max(ts), 8 * cma / dt / 1e12, ssum.sum() / (2.0 * nvec * ns)))


def bench_bondorder(argv):
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import bondorder_ref as R
    from neuralmelting_amd import _lib as B, lattice
    ns = int(argv[0]) if len(argv) > 0 else 4096
    cells = int(argv[1]) if len(argv) > 1 else 4
    cut = float(argv[2]) if len(argv) > 2 else 0.0
    reps = int(argv[3]) if len(argv) > 3 else 5
    ls = np.array([int(x) for x in argv[4:]] or [4, 6], dtype=np.int32)
    rng = np.random.default_rng(3)                                            # the frames of bench_angles
    n = 4 * cells ** 3
    cut = distr.bond_cutoff(cut, n)
    a0 = lattice.lattice_constant('LJ')
    box = (cells * a0 * (1.0 + 0.05 * rng.random(ns))).astype(np.float32)
    frac = lattice.fcc_fractional(cells)
    pos = ((frac[None] + 0.08 / cells * rng.normal(size=(ns, n, 3))) % 1.0 * box[:, None, None]).astype(np.float32)
    pos = np.minimum(pos, np.nextafter(box, np.float32(0))[:, None, None])
    l = float(box.min())
    L = B.load()
    nl = len(ls)
    q2, b2, g2 = np.zeros((ns, n, nl)), np.zeros((ns, n, nl)), np.zeros((ns, nl))
    nb = np.zeros((ns, n), dtype=np.int32)
    ce = np.ascontiguousarray(np.cos(np.linspace(1e-16, np.pi, 64)))
    adf = np.zeros((ns, 64), dtype=np.uint64)

    def run(m):
        rc = L.nm_distr_bondorder(0, m, n, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), 1e-16 * l, cut * l, nl,
                                  ls.ctypes.data_as(B.c_int_p), q2.ctypes.data_as(B.c_double_p), b2.ctypes.data_as(B.c_double_p),
                                  g2.ctypes.data_as(B.c_double_p), nb.ctypes.data_as(B.c_int32_p))
        if rc != 0:
            raise RuntimeError(L.nm_distr_last_error().decode())

    def run_angles(m):
        rc = L.nm_distr_angles(0, m, n, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), 1e-16 * l, cut * l, 64,
                               ce.ctypes.data_as(B.c_double_p), adf.ctypes.data_as(B.c_uint64_p))
        if rc != 0:
            raise RuntimeError(L.nm_distr_last_error().decode())
    med = {}
    for name, f in (('bondorder', run), ('angles', run_angles)):
        f(min(ns, 8))
        f(ns)                                                                 # warm-up at the timed shape
        ts = []
        for _ in range(reps):
            t = time.perf_counter(); f(ns); ts.append(time.perf_counter() - t)
        med[name] = (float(np.median(ts)), min(ts), max(ts))
    bonds = int(nb.sum())
    dt = med['bondorder'][0]
    print('bondorder: %d samples x %d atoms, cutoff %.4f l, l = %s: %d bonds (%.1f neighbours per centre, %d at most); call (H2D + kernels '
          '+ D2H) median of %d: %.4f s (min %.4f, max %.4f) = %.2f G bonds/s, %.1f M centres/s; mean q %s, qbar %s, Q %s'
          % (ns, n, cut, ls.tolist(), bonds, bonds / (ns * n), nb.max(), reps, dt, med['bondorder'][1], med['bondorder'][2],
             bonds / dt / 1e9, ns * n / dt / 1e6, np.sqrt(q2).mean(axis=(0, 1)).round(4), np.sqrt(b2).mean(axis=(0, 1)).round(4),
             np.sqrt(g2).mean(axis=0).round(4)))
    print('angles on the same frames and shell, 64 edges: call median of %d: %.4f s (min %.4f, max %.4f); bondorder / angles = %.2f'
          % (reps, med['angles'][0], med['angles'][1], med['angles'][2], dt / med['angles'][0]))
    t = time.perf_counter()
    R.bond_order2(pos[:1], box[:1], ls.tolist(), 1e-16 * l, cut * l)
    dt = time.perf_counter() - t
    print('numpy restatement, one core, sample 0: %.3f s = %.2f samples/s, %.1f centres/s' % (dt, 1 / dt, n / dt))


def bench_bond_w(argv):
    from neuralmelting_amd import _lib as B, lattice
    ns = int(argv[0]) if len(argv) > 0 else 4096
    cells = int(argv[1]) if len(argv) > 1 else 4
    cut = float(argv[2]) if len(argv) > 2 else 0.0
    reps = int(argv[3]) if len(argv) > 3 else 5
    ls = np.array([int(x) for x in argv[4:]] or [4, 6], dtype=np.int32)
    rng = np.random.default_rng(3)                                            # the frames of bench_angles
    n = 4 * cells ** 3
    cut = distr.bond_cutoff(cut, n)
    a0 = lattice.lattice_constant('LJ')
    box = (cells * a0 * (1.0 + 0.05 * rng.random(ns))).astype(np.float32)
    frac = lattice.fcc_fractional(cells)
    pos = ((frac[None] + 0.08 / cells * rng.normal(size=(ns, n, 3))) % 1.0 * box[:, None, None]).astype(np.float32)
    pos = np.minimum(pos, np.nextafter(box, np.float32(0))[:, None, None])
    l = float(box.min())
    L = B.load()
    nl = len(ls)
    w3, wb3, q2, b2 = (np.zeros((ns, n, nl)) for _ in range(4))
    W3, g2 = np.zeros((ns, nl)), np.zeros((ns, nl))
    nb = np.zeros((ns, n), dtype=np.int32)
    P = lambda a: a.ctypes.data_as(B.c_double_p)
    head = lambda m: (0, m, n, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), 1e-16 * l, cut * l, nl,
                      ls.ctypes.data_as(B.c_int_p))

    def run_w(m):
        rc = L.nm_distr_bondorder_w(*head(m), P(w3), P(wb3), P(W3), P(q2), P(b2), P(g2), nb.ctypes.data_as(B.c_int32_p))
        if rc != 0:
            raise RuntimeError(L.nm_distr_last_error().decode())

    def run(m):
        rc = L.nm_distr_bondorder(*head(m), P(q2), P(b2), P(g2), nb.ctypes.data_as(B.c_int32_p))
        if rc != 0:
            raise RuntimeError(L.nm_distr_last_error().decode())
    med = {}
    for name, f in (('bondorder_w', run_w), ('bondorder', run)):
        f(min(ns, 8))
        f(ns)                                                                 # warm-up at the timed shape
        ts = []
        for _ in range(reps):
            t = time.perf_counter(); f(ns); ts.append(time.perf_counter() - t)
        med[name] = (float(np.median(ts)), min(ts), max(ts))
    hat = lambda w, x: np.divide(w, np.maximum(x, 0.0) ** 1.5, out=np.zeros_like(w), where=x > 0.0)
    dt = med['bondorder_w'][0]
    print('bond-w: %d samples x %d atoms, cutoff %.4f l, l = %s: %.1f neighbours per centre; nm_distr_bondorder_w, seven outputs, call (H2D '
          '+ kernels + D2H) median of %d: %.4f s (min %.4f, max %.4f) = %.1f M centres/s; mean w %s, wbar %s, W %s'
          % (ns, n, cut, ls.tolist(), nb.sum() / (ns * n), reps, dt, med['bondorder_w'][1], med['bondorder_w'][2], ns * n / dt / 1e6,
             hat(w3, q2).mean(axis=(0, 1)).round(5), hat(wb3, b2).mean(axis=(0, 1)).round(5), hat(W3, g2).mean(axis=0).round(5)))
    print('nm_distr_bondorder on the same frames, shell and l, four outputs: call median of %d: %.4f s (min %.4f, max %.4f); '
          'bondorder_w / bondorder = %.2f' % (reps, med['bondorder'][0], med['bondorder'][1], med['bondorder'][2], dt / med['bondorder'][0]))


def bench_solid(argv):
    from neuralmelting_amd import _lib as B, lattice
    ns = int(argv[0]) if len(argv) > 0 else 4096
    cells = int(argv[1]) if len(argv) > 1 else 4
    cut = float(argv[2]) if len(argv) > 2 else 0.0
    reps = int(argv[3]) if len(argv) > 3 else 5
    lv = int(argv[4]) if len(argv) > 4 else 6
    s_min = float(argv[5]) if len(argv) > 5 else 0.5
    n_min = int(argv[6]) if len(argv) > 6 else 8
    rng = np.random.default_rng(3)                                            # the frames of bench_angles
    n = 4 * cells ** 3
    cut = distr.bond_cutoff(cut, n)
    a0 = lattice.lattice_constant('LJ')
    box = (cells * a0 * (1.0 + 0.05 * rng.random(ns))).astype(np.float32)
    frac = lattice.fcc_fractional(cells)
    pos = ((frac[None] + 0.08 / cells * rng.normal(size=(ns, n, 3))) % 1.0 * box[:, None, None]).astype(np.float32)
    pos = np.minimum(pos, np.nextafter(box, np.float32(0))[:, None, None])
    l = float(box.min())
    L = B.load()
    ls = np.array([lv], dtype=np.int32)
    b2 = np.zeros((ns, n, 1))
    nb = np.zeros((ns, n), dtype=np.int32)
    nconn, label = np.zeros((ns, n), dtype=np.int32), np.zeros((ns, n), dtype=np.int32)
    nsolid, nclus, largest = np.zeros(ns, dtype=np.int32), np.zeros(ns, dtype=np.int32), np.zeros(ns, dtype=np.int32)
    ip = lambda x: x.ctypes.data_as(B.c_int32_p)

    def run(m):
        rc = L.nm_distr_solid(0, m, n, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), 1e-16 * l, cut * l, lv, s_min, n_min,
                              ip(nconn), ip(label), ip(nsolid), ip(nclus), ip(largest))
        if rc != 0:
            raise RuntimeError(L.nm_distr_last_error().decode())

    def run_qbar(m, nnb=None):
        rc = L.nm_distr_bondorder(0, m, n, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), 1e-16 * l, cut * l, 1,
                                  ls.ctypes.data_as(B.c_int_p), None, b2.ctypes.data_as(B.c_double_p), None, nnb)
        if rc != 0:
            raise RuntimeError(L.nm_distr_last_error().decode())
    med = {}
    for name, f in (('solid', run), ('qbar', run_qbar)):
        f(min(ns, 8))
        f(ns)                                                                 # warm-up at the timed shape
        ts = []
        for _ in range(reps):
            t = time.perf_counter(); f(ns); ts.append(time.perf_counter() - t)
        med[name] = (float(np.median(ts)), min(ts), max(ts))
    run_qbar(ns, ip(nb))                                                      # the entries, outside the timing
    ent = int(nb.sum())
    dt = med['solid'][0]
    print('solid: %d samples x %d atoms, cutoff %.4f l, l = %d, s_min %g, n_min %d: %d entries (%.1f per centre, %d at most), %.2f connections '
          'per atom; solid fraction %.4f, %.2f clusters per sample, largest / natoms %.4f; call (H2D + kernels + D2H) median of %d: %.4f s '
          '(min %.4f, max %.4f) = %.2f G entries/s, %.1f M centres/s'
          % (ns, n, cut, lv, s_min, n_min, ent, ent / (ns * n), nb.max(), nconn.mean(), nsolid.mean() / n, nclus.mean(), largest.mean() / n,
             reps, dt, med['solid'][1], med['solid'][2], ent / dt / 1e9, ns * n / dt / 1e6))
    print('bondorder with qbar2 alone, l = %d, on the same frames and shell: call median of %d: %.4f s (min %.4f, max %.4f); solid / bondorder = %.2f'
          % (lv, reps, med['qbar'][0], med['qbar'][1], med['qbar'][2], dt / med['qbar'][0]))


def bench_cna(argv):
    from neuralmelting_amd import _lib as B, lattice
    ns = int(argv[0]) if len(argv) > 0 else 4096
    cells = int(argv[1]) if len(argv) > 1 else 4
    cut = float(argv[2]) if len(argv) > 2 else 0.0
    reps = int(argv[3]) if len(argv) > 3 else 5
    mode = argv[4] if len(argv) > 4 else 'adaptive'
    rng = np.random.default_rng(3)                                            # the frames of bench_angles
    n = 4 * cells ** 3
    cut = distr.cna_radius(cut, n, mode)
    a0 = lattice.lattice_constant('LJ')
    box = (cells * a0 * (1.0 + 0.05 * rng.random(ns))).astype(np.float32)
    frac = lattice.fcc_fractional(cells)
    pos = ((frac[None] + 0.08 / cells * rng.normal(size=(ns, n, 3))) % 1.0 * box[:, None, None]).astype(np.float32)
    pos = np.minimum(pos, np.nextafter(box, np.float32(0))[:, None, None])
    l = float(box.min())
    L = B.load()
    typ, sig = np.zeros((ns, n), dtype=np.int32), np.zeros((ns, n, 8), dtype=np.int32)
    ntype, nsig = np.zeros((ns, 5), dtype=np.int32), np.zeros((ns, 8), dtype=np.int32)
    nconn, label = np.zeros((ns, n), dtype=np.int32), np.zeros((ns, n), dtype=np.int32)
    nsolid, nclus, largest = np.zeros(ns, dtype=np.int32), np.zeros(ns, dtype=np.int32), np.zeros(ns, dtype=np.int32)
    nb = np.zeros((ns, n), dtype=np.int32)
    ls = np.array([6], dtype=np.int32)
    ip = lambda x: x.ctypes.data_as(B.c_int32_p)

    def run(m):
        rc = L.nm_distr_cna(0, m, n, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), 1e-16 * l, cut * l,
                            distr.CNA_MODES[mode], ip(typ), ip(sig), ip(ntype), ip(nsig))
        if rc != 0:
            raise RuntimeError(L.nm_distr_last_error().decode())

    def run_solid(m):
        rc = L.nm_distr_solid(0, m, n, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), 1e-16 * l, cut * l, 6, 0.5, 8,
                              ip(nconn), ip(label), ip(nsolid), ip(nclus), ip(largest))
        if rc != 0:
            raise RuntimeError(L.nm_distr_last_error().decode())
    med = {}
    for name, f in (('cna', run), ('solid', run_solid)):
        f(min(ns, 8))
        f(ns)                                                                 # warm-up at the timed shape
        ts = []
        for _ in range(reps):
            t = time.perf_counter(); f(ns); ts.append(time.perf_counter() - t)
        med[name] = (float(np.median(ts)), min(ts), max(ts))
    rc = L.nm_distr_bondorder(0, ns, n, pos.ctypes.data_as(B.c_float_p), box.ctypes.data_as(B.c_float_p), 1e-16 * l, cut * l, 1,
                              ls.ctypes.data_as(B.c_int_p), None, None, None, ip(nb))   # the entries, outside the timing
    if rc != 0:
        raise RuntimeError(L.nm_distr_last_error().decode())
    ent = int(nb.sum())
    dt = med['cna'][0]
    print('cna %s: %d samples x %d atoms, radius %.4f l: %d entries (%.1f per centre, %d at most); types other fcc hcp bcc ico %s, '
          'columns 421 422 444 666 555 544 433 other %s; call (H2D + kernel + D2H) median of %d: %.4f s (min %.4f, max %.4f) = '
          '%.2f G entries/s, %.1f M centres/s'
          % (mode, ns, n, cut, ent, ent / (ns * n), nb.max(), (ntype.sum(axis=0) / (ns * n)).round(4).tolist(),
             (nsig.sum(axis=0) / max(1, int(nsig.sum()))).round(4).tolist(), reps, dt, med['cna'][1], med['cna'][2], ent / dt / 1e9,
             ns * n / dt / 1e6))
    print('solid (l = 6, s_min 0.5, n_min 8) on the same frames and shell: call median of %d: %.4f s (min %.4f, max %.4f); cna / solid = %.2f'
          % (reps, med['solid'][0], med['solid'][1], med['solid'][2], dt / med['solid'][0]))


def bench_entropy(argv):
    from neuralmelting_amd import lattice
    ns = int(argv[0]) if len(argv) > 0 else 4096
    cells = int(argv[1]) if len(argv) > 1 else 4
    reps = int(argv[2]) if len(argv) > 2 else 5
    flags = ['-le']
    for f, v in zip(('-lr', '-lw', '-lg', '-lv'), argv[3:7]):
        flags += [f, v]
    rng = np.random.default_rng(3)                                            # the frames of bench_angles
    n = 4 * cells ** 3
    rm, sigma, nbins, ravg = distr.entropy_params(distr.parse_args(flags), n)
    a0 = lattice.lattice_constant('LJ')
    box = (cells * a0 * (1.0 + 0.05 * rng.random(ns))).astype(np.float32)
    frac = lattice.fcc_fractional(cells)
    pos = ((frac[None] + 0.08 / cells * rng.normal(size=(ns, n, 3))) % 1.0 * box[:, None, None]).astype(np.float32)
    pos = np.minimum(pos, np.nextafter(box, np.float32(0))[:, None, None])
    l = float(box.min())
    natoms = np.full(ns, n)
    run = lambda m: distr.local_entropy(natoms[:m], box[:m], pos[:m], rm * l, sigma * l, nbins, ravg * l, -4.0)
    run(min(ns, 8))
    run(ns)                                                                   # warm-up at the timed shape
    ts = []
    for _ in range(reps):
        t = time.perf_counter(); s, sbar, nnb, smean, sbarmean, nlow = run(ns); ts.append(time.perf_counter() - t)
    dt = float(np.median(ts))
    ent = int(nnb.sum())
    print('entropy: %d samples x %d atoms, r_m %.4f l, sigma %.5f l, %d intervals, r_avg %.4f l: %d entries (%.1f per centre, %d at most), '
          '%.3e Gaussian terms on the grid; mean s %.4f, mean sbar %.4f, below -4: %.4f; call (H2D + kernels + D2H) median of %d: %.4f s '
          '(min %.4f, max %.4f) = %.2f G entries/s, %.1f M centres/s'
          % (ns, n, rm, sigma, nbins, ravg, ent, ent / (ns * n), nnb.max(), float(ent) * (nbins + 1), smean.mean(), sbarmean.mean(),
             nlow.mean() / n, reps, dt, min(ts), max(ts), ent / dt / 1e9, ns * n / dt / 1e6))


if '--entropy' in sys.argv:
    bench_entropy([x for x in sys.argv[1:] if x != '--entropy'])
    sys.exit(0)

if '--cna' in sys.argv:
    bench_cna([x for x in sys.argv[1:] if x != '--cna'])
    sys.exit(0)

if '--solid' in sys.argv:
    bench_solid([x for x in sys.argv[1:] if x != '--solid'])
    sys.exit(0)

if '--bondorder' in sys.argv:
    bench_bondorder([x for x in sys.argv[1:] if x != '--bondorder'])
    sys.exit(0)

if '--bond-w' in sys.argv:
    bench_bond_w([x for x in sys.argv[1:] if x != '--bond-w'])
    sys.exit(0)

if '--sfactor' in sys.argv:
    bench_sfactor([x for x in sys.argv[1:] if x != '--sfactor'])
    sys.exit(0)

if '--angles' in sys.argv:
    bench_angles([x for x in sys.argv[1:] if x != '--angles'])
    sys.exit(0)

from oracle import distr_oracle as D

ns, n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096, int(sys.argv[2]) if len(sys.argv) > 2 else 256
rng = np.random.default_rng(3)
box = (6.0 + 0.3 * rng.random(ns)).astype(np.float32)
pos = (rng.random((ns, n, 3)) * box[:, None, None]).astype(np.float32)
natoms = np.full(ns, n, np.uint16)
nrho, dni, r, dn, rv = distr.calculate_spatial(natoms, box, 64, 16)
distr.histograms(natoms[:8], box[:8], pos[:8], r, rv)
for rep in range(3):
    t = time.time(); rdf, cdf = distr.histograms(natoms, box, pos, r, rv); dt = time.time() - t
    print('GPU call (H2D + kernel + D2H): %d samples x %d atoms in %.3f s = %.0f samples/s, %.2f G pair-images/s'
          % (ns, n, dt, ns / dt, ns * 27 * n * n / dt / 1e9))
m = 8
t = time.time()
for s in range(m):
    D.calculate_rdf(n, box[s], pos[s], r); D.calculate_cdf(n, box[s], pos[s], rv)
dt = time.time() - t
print('numpy restatement: %.1f samples/s (one core)' % (m / dt))
