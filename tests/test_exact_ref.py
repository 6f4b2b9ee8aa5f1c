"""CPU: the exact all-pairs reference (tests/exact_ref.py) against the oracle's list evaluation (setup) and its direct sum
(eval_allpairs) on every edge state the GPU edge tests use.  Pins the reference, and the oracle at the edges: pairs at the cutoff
and at the list radius, through every periodic image, on the faces, unwrapped, close contacts, boxes from 2 rc to 2 (rc + skin), and
EAM atoms with nothing inside rc."""
import os
import re

import numpy as np
import pytest

import exact_ref as X
from helpers import CSRC, NM_API, cfg_rows

REL = 1e-12

CASES = [('LJ', n) for n in (2, 5, 33, 100, 257, 865)] + [('Al', n) for n in (2, 100, 256)]


def states(el, n):
    L = X.box_for(el, n, 0.5 if el == 'LJ' else 0.05)
    return X.edge_states(el, n, L, seed=1) + X.box_edge_states(el, n, seed=1)


def _sim(oracle, el, n):
    return oracle.Sim(n) if el == 'LJ' else oracle.Sim(n, units=1, mass=29.982, pot=1)


@pytest.mark.parametrize('el,n', CASES)
def test_exact_reference_against_the_oracle(oracle, el, n):
    sts = states(el, n)
    kinds = {name for name, _, _ in sts}
    assert {'fluid', 'planted_cutoff', 'half_box', 'faces', 'unwrapped'} <= kinds
    if el == 'LJ':
        assert {'contact_0.55', 'contact_0.62'} <= kinds
    else:
        assert ('al_shell_pair' if n == 2 else 'al_isolated') in kinds
    for name, x, L in sts:
        U, W, f, npairs, _ = X.exact(el, x, L)
        b = X.force_bound(el, x, L)
        s = _sim(oracle, el, n)
        s.set_box(L); s.set_x(x.reshape(-1)); s.setup()
        assert s.npairs == npairs, name
        scale = max(abs(float(U)), 1e-300)
        assert abs(s.pe - float(U)) <= REL * scale, (name, s.pe, float(U))
        assert abs(s.virial - float(W)) <= REL * max(abs(float(W)), 1e-300), (name, s.virial, float(W))
        fo = s.get_f().reshape(-1, 3)
        assert np.all(np.abs(fo - f) <= b), (name, np.abs(fo - f).max())
        if el == 'LJ':
            Ua, Wa, fa = s.eval_allpairs()
            assert abs(Ua - float(U)) <= REL * scale and abs(Wa - float(W)) <= REL * max(abs(float(W)), 1e-300), name
            assert np.all(np.abs(fa.reshape(-1, 3) - f) <= b), name
        s.close()


def test_edge_states_are_what_they_claim():
    """the planted geometry itself: pairs at rc (1 -+ 1e-12) straddle the cutoff, the Al shell atom has no neighbour inside rc"""
    L = X.box_for('LJ', 100, 0.5)
    x = dict((nm, xx) for nm, xx, _ in X.edge_states('LJ', 100, L, seed=1))['planted_cutoff']
    d = x[:, None, :] - x[None, :, :]
    d -= L * np.rint(d / L)
    r = np.sqrt((d * d).sum(-1))[np.triu_indices(len(x), 1)]
    rc, rl = X.LJ_RC, X.LJ_RC + X.skin('LJ', 100)
    assert ((r < rc) & (r > rc * (1 - 2e-12))).any() and ((r > rc) & (r < rc * (1 + 2e-12))).any()
    assert ((r < rl) & (r > rl - 2e-9)).any()
    for el, n in (('Al', 2), ('Al', 100)):
        nm, x, L = [s for s in X.edge_states(el, n, X.box_for(el, n, 0.05), seed=1) if s[0].startswith('al_')][0]
        d = x - x[0]
        d -= L * np.rint(d / L)
        r = np.sqrt((d * d).sum(-1))[1:]
        assert r.min() > X.SC_RC and r.min() <= X.SC_RC + X.skin(el, n), (nm, r.min())
    for el in ('LJ', 'Al'):
        Ls = [L for _, _, L in X.box_edge_states(el, 2)]
        rc, sk = X.RC[el], X.skin(el, 2)
        assert Ls[0] == 2 * rc and Ls[-1] > 2 * (rc + sk)


def test_the_gpu_edge_matrix_covers_every_lj_and_4cubed_al_row():
    """tests/test_eval_edges_gpu.py names a configuration for every (element, kind, workgroups per replica) of lj/cut and of Al at 4^3:
    the row of nm_rows.hip's configuration table (NM_CFG_ROWS) for each, so that a new row cannot go untested"""
    import test_eval_edges_gpu as G
    tested = {({'LJ': 0, 'Al': 1}[el], G.kind(n), q): G.qs(el, n)[q] for el, n, q in (c.values for c in G.CASES)}
    assert tested == {k: name for k, (name, _) in cfg_rows().items() if k[0] == 0 or k[:2] == (1, 0)}


def test_every_launch_finds_its_configuration_in_the_table():
    """The sampler picks the kernel configuration of a context in one place, nm_rows.hip's NM_CFG_ROWS through with_row: no launcher, occupancy
    query or kernel reference in any of its source files names a Cfg typedef, so the block launch, the occupancy query and the residency probe
    cannot disagree.  The host code (nm_api.hip) reaches the kernels through nm_rows.h alone: nothing it includes is, or includes, a kernel header.
    The rows with a fused nm_cycles_kernel and the workgroups per replica of each (potential, kind) are the measured and tested ones."""
    launcher = r'launch_block|launch_probe|blocks_per_cu|request_lds|launch_cycles(?:_rec|_form)?|launch_block_form|nm_(?:block|probe|cycles)_kernel'
    for name in ('nm_api.hip', 'nm_rows.hip', 'nm_rows.h', 'nm_params.h', 'nm_kernels.h', 'nm_device.h'):
        named = re.findall(r'\b(?:%s)\s*<\s*Cfg\w*' % launcher, open(os.path.join(CSRC, name)).read())
        assert not named, (name, named)
    seen, todo = set(), [NM_API]
    while todo:                                  # everything nm_api.hip includes from its own directory
        for inc in re.findall(r'^\s*#\s*include\s*"([^"/]+)"', open(todo.pop()).read(), flags=re.M):
            if inc not in seen:
                seen.add(inc)
                todo.append(os.path.join(CSRC, inc))
    assert 'nm_rows.h' in seen and not seen & {'nm_kernels.h', 'nm_device.h', 'nm_math.h'}, seen
    assert not re.search(r'hipLaunchKernelGGL|<<<|\bCfg\w*|\bnm_\w+_kernel\b', re.sub(r'//.*', '', open(NM_API).read()))   # (its comments may)
    rows = cfg_rows()
    fused = {k for k, (_, f) in rows.items() if f}
    assert fused == {(0, 0, 2), (0, 0, 4), (0, 0, 8), (0, 1, 8), (1, 0, 2), (1, 0, 4), (2, 0, 2), (2, 0, 4)}
    qs = {}
    for pot, kind, q in sorted(rows):
        qs.setdefault((pot, kind), []).append(q)
    assert qs == {(0, 0): [1, 2, 4, 8], (0, 1): [1, 2, 4, 8], (0, 2): [1, 2, 4], **{(p, k): [1, 2, 4] for p in (1, 2) for k in range(3)}}
