"""Diagnostic build (make prof) only: scripts/check_bounds.py for the EAM elements above 256 atoms — the 16-bit-list EAM kernels (CfgMidSC,
CfgMidSCQ4, CfgLargeSC, and their n = 9 twins for Cu and Ni; the densities of the last in the global spill).  5^3, 6^3 and 8^3 cells at 1, 2
and 4 workgroups per replica, bulk and iterative position moves, on bench's metal temperatures: every index into the spill and list arrays
checked inside the kernel, every rebuilt list row checked against exact separations.  Prints the counts; all must be 0.  --el Cu / Ni: the
n = 9 kernels; --sizes 4,5,6,8 adds the 4^3 byte-list kernels.

    NM_HIP_LIB=$PWD/build/variants/libnm_hip_prof.so python scripts/check_bounds_al.py [--el Al|Cu|Ni] [--sizes 5,6,8]
"""
import argparse
import ctypes as C
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

os.environ['NM_DBG'] = '8'   # the exact list self-check of the diagnostic build


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--el', default='Al', choices=('Al', 'Cu', 'Ni'))
    ap.add_argument('--sizes', default='5,6,8')
    a = ap.parse_args(argv)
    el, sizes = a.el, [int(s) for s in a.sizes.split(',')]
    import neuralmelting_amd as nm
    from neuralmelting_amd import lattice, _lib
    assert 'prof' in _lib.LIB_PATH, 'run with NM_HIP_LIB pointing at libnm_hip_prof.so'
    L = _lib.load()
    total = 0
    P = np.linspace(1.0, 8.0, 2, dtype=np.float32)
    T = np.linspace(256.0, 2560.0, 4, dtype=np.float32)
    for sz in sizes:
        for q in (1, 2, 4):
            for bulk in (True, False):
                os.environ['NM_CUS_PER_REPLICA'] = str(q)
                x, v, box, d = lattice.init_states(sz, P, T, 0.03125, 0.03125, el=el)
                e = nm.Engine(4 * sz ** 3, P, T, element=el, bulk=bulk, ppos=0.2, pvol=0.2)
                assert e.cus_per_replica == q
                e.set_state(x, v, box, d)
                for step in range(4):
                    e.set_step(step); e.run_block(12); e.adapt(); e.exchange(count=False)
                e.synchronize()
                st = e.stats()
                n, m = C.c_uint(0), C.c_uint(0)
                assert L.nm_prof_oob(e.h, C.byref(n)) == 0 and L.nm_prof_list_miss(e.h, C.byref(m)) == 0
                print('%s %d^3 Q=%d %-9s rebuilds %4d  evaluations %5d  longest row %3d  out-of-range indices %d  incomplete list rows %d'
                      % (el, sz, q, 'bulk' if bulk else 'iterative', st[:, 1].sum(), st[:, 0].sum(), st[:, 8].max(), n.value, m.value), flush=True)
                total += n.value + m.value
                e.close()
    print('total', total)
    return 0 if total == 0 else 1


if __name__ == '__main__':
    sys.exit(main())
