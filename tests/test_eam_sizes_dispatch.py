"""CPU: element Al above 256 atoms.  The GPU test matrix of tests/test_eam_sizes_gpu.py names every EAM instantiation nm_api.hip's
launch_kind_eam can pick, and the oracle agrees with the exact all-pairs reference (tests/exact_ref.py) on the Al edge states at the
5^3 and 6^3 sizes those tests use."""
import os
import re

import numpy as np
import pytest

import exact_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_eam_gpu_matrix_covers_every_instantiation_launch_kind_eam_can_pick():
    import test_eam_sizes_gpu as G
    src = open(os.path.join(ROOT, 'neuralmelting_amd', 'csrc', 'nm_api.hip')).read()
    body = src[src.index('hipError_t launch_kind_eam('):]
    body = body[:body.index('\n}\n')]
    launched = set(re.findall(r'launch_block<(\w+)>', body))
    tested = {G.qs(n)[q] for n, q in (c.values for c in G.CASES)}
    assert launched and tested == launched
    # launch_kind hands element Al above 256 atoms to it
    lk = src[src.index('hipError_t launch_kind('):]
    lk = lk[:lk.index('\n}\n')]
    assert 'c->pot == 1 && c->kind > 0) return launch_kind_eam(c, p)' in lk


def test_occupancy_query_and_residency_probe_name_the_configurations_launch_kind_eam_launches():
    """pick_q sizes a cluster grid by blocks_per_cu_kind and gathers it with probe_kind: for element Al above 256 atoms both must ask
    about the instantiations launch_kind_eam launches, with the same choice by kind and workgroups per replica"""
    src = open(os.path.join(ROOT, 'neuralmelting_amd', 'csrc', 'nm_api.hip')).read()

    def body(sig):
        b = src[src.index(sig):]
        return b[:b.index('\n}\n')]

    def norm(text, fn):
        # the dispatch expression with the callee and the variable names taken out: kind == 1 ? (q == 4 ? A : B) : C
        t = re.sub(r'%s<(\w+)>\([^)]*\)' % fn, r'\1', text)
        return re.sub(r'\s+', ' ', t.replace('c->', '').replace('cus', 'q')).strip()

    launch = body('hipError_t launch_kind_eam(')
    m1 = re.search(r'if \(kind == 1\) return (.*?);\s*return launch_block<(\w+)>', launch.replace('c->', ''))
    assert m1, launch
    want = 'kind == 1 ? (%s) : %s' % (norm(m1.group(1), 'launch_block'), m1.group(2))
    occ = re.search(r'if \(pot == 1 && kind > 0\) return (.*?);\n', body('int blocks_per_cu_kind('))
    prb = re.search(r'if \(c->pot == 1 && c->kind > 0\) return (.*?);\n', body('hipError_t probe_kind('))
    assert occ and prb
    assert norm(occ.group(1), 'blocks_per_cu') == want
    assert norm(prb.group(1), 'launch_probe') == want
    assert want == 'kind == 1 ? (q == 4 ? CfgMidSCQ4 : CfgMidSC) : CfgLargeSC', want


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
