"""Longest Verlet-list row the EAM kernels build (stats column 8) on bench's metal grid — 8 x 8, P 1 .. 8 bar, T 256 .. 2560 K — over 40 cycles
from the lattice, at 5^3, 6^3 and 8^3 cells, against the 256 slots per atom of CfgMidSC / CfgLargeSC (nm_rows.hip).  Element Al, or the one
given as the first argument (Cu, Ni: the n = 9 twins)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import neuralmelting_amd as nm
from neuralmelting_amd import lattice

el = sys.argv[1] if len(sys.argv) > 1 else 'Al'

P = np.linspace(1.0, 8.0, 8, dtype=np.float32)
T = np.linspace(256.0, 2560.0, 8, dtype=np.float32)
for sz in (5, 6, 8):
    n = 4 * sz ** 3
    x, v, box, d = lattice.init_states(sz, P, T, 0.03125, 0.03125, el=el)
    e = nm.Engine(n, P, T, element=el)
    e.set_state(x, v, box, d)
    e.stats(reset=True)
    for c in range(40):
        e.set_step(c); e.run_block(8); e.adapt(); e.exchange(count=False)
    st = e.stats()
    print('%s %d^3 (%d atoms), %d workgroups per replica: longest row %d of %d slots; per temperature (K):' % (el, sz, n, e.cus_per_replica, st[:, 8].max(), st[0, 9]))
    print('   ' + '  '.join('%4.0f:%3d' % (T[j], st[j::8, 8].max()) for j in range(8)), flush=True)
    e.close()
