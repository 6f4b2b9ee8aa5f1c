"""CPU: element Al above 256 atoms.  The GPU test matrix of tests/test_eam_sizes_gpu.py names every row of nm_rows.hip's configuration
table (NM_CFG_ROWS) for Al above 256 atoms, and the oracle agrees with the exact all-pairs reference (tests/exact_ref.py) on the Al edge
states at the 5^3 and 6^3 sizes those tests use."""
import numpy as np
import pytest

import exact_ref as X
from helpers import cfg_rows


def test_the_eam_gpu_matrix_covers_every_al_row_above_256_atoms():
    import test_eam_sizes_gpu as G
    tested = {(1, 1 if n <= 864 else 2, q): G.qs(n)[q] for n, q in (c.values for c in G.CASES)}
    assert tested == {k: name for k, (name, _) in cfg_rows().items() if k[0] == 1 and k[1] > 0}


@pytest.mark.parametrize('n', [500, 864])
def test_exact_reference_against_the_oracle_al(oracle, n):
    L = X.box_for('Al', n, 0.05)
    for name, x, LL in X.edge_states('Al', n, L, seed=1) + X.box_edge_states('Al', n, seed=1):
        U, W, f, npairs, _ = X.exact('Al', x, LL)
        s = oracle.Sim(n, units=1, mass=29.982, pot=1)
        s.set_box(LL); s.set_x(x.reshape(-1)); s.setup()
        assert s.npairs == npairs, name
        assert abs(s.pe - float(U)) <= 1e-12 * abs(float(U)), (name, s.pe, float(U))
        assert abs(s.virial - float(W)) <= 1e-12 * max(abs(float(W)), 1e-300), (name, s.virial, float(W))
        assert np.all(np.abs(s.get_f().reshape(-1, 3) - f) <= X.force_bound('Al', x, LL)), name
