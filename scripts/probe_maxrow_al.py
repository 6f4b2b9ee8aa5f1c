"""Longest Verlet-list row the EAM kernels build (stats column 8) on bench's Al grid — 8 x 8, P 1 .. 8 bar, T 256 .. 2560 K — over 40 cycles
from the lattice, at 5^3, 6^3 and 8^3 cells, against the 256 slots per atom of CfgMidSC / CfgLargeSC (nm_api.hip)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import neuralmelting_amd as nm
from neuralmelting_amd import lattice

P = np.linspace(1.0, 8.0, 8, dtype=np.float32)
T = np.linspace(256.0, 2560.0, 8, dtype=np.float32)
for sz in (5, 6, 8):
    n = 4 * sz ** 3
    x, v, box, d = lattice.init_states(sz, P, T, 0.03125, 0.03125, el='Al')
    e = nm.Engine(n, P, T, element='Al')
    e.set_state(x, v, box, d)
    e.stats(reset=True)
    for c in range(40):
        e.set_step(c); e.run_block(8); e.adapt(); e.exchange(count=False)
    st = e.stats()
    print('Al %d^3 (%d atoms), %d workgroups per replica: longest row %d of %d slots; per temperature (K):' % (sz, n, e.cus_per_replica, st[:, 8].max(), st[0, 9]))
    print('   ' + '  '.join('%4.0f:%3d' % (T[j], st[j::8, 8].max()) for j in range(8)), flush=True)
    e.close()
