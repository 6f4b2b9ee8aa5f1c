"""CPU tests: the oracle and the driver's host logic against the goldens produced by the REFERENCE's own functions
(tests/golden/make_golden.py).  These pin everything the reference itself contributes to the hot path."""
import json
import os
import re

import numpy as np
import pytest

from helpers import constants_lj
from neuralmelting_amd import lattice, remcmc

HERE = os.path.dirname(os.path.abspath(__file__))
G = json.load(open(os.path.join(HERE, 'golden', 'ref_scalars.json')))
B = np.load(os.path.join(HERE, 'golden', 'ref_blocks.npz'))
BA = np.load(os.path.join(HERE, 'golden', 'ref_blocks_al.npz'))
AL_TRACES = ['%s_%d' % (tag, sz) for sz in (4, 5) for tag in ('bulk', 'iter', 'default_mix')]


@pytest.mark.parametrize('tag', ['lj_2x2', 'lj_8x8', 'al_8x8'])
def test_G1_constants(tag):
    g = G['G1_constants'][tag]
    P, T = np.float32(g['P']), np.float32(g['T'])
    got = [remcmc.init_constant(P, T, g['el'], i, j) for i in range(len(P)) for j in range(len(T))]
    np.testing.assert_array_equal([a for a, b in got], g['et'])
    np.testing.assert_array_equal([b for a, b in got], g['pf'])
    if g['el'] == 'LJ':
        et, pf, _ = constants_lj(P, T)
        np.testing.assert_array_equal(et, g['et'])
        np.testing.assert_array_equal(pf, g['pf'])


def test_G2_adapt(oracle):
    for g in G['G2_adapt']:
        np.testing.assert_array_equal(oracle.adapt(np.float32(g['ratios']), g['steps_in']), g['steps_out'])
        assert g['tail'] == [0.0] * 9          # counters and ratios are zeroed (remcmc:745)


@pytest.mark.parametrize('idx', range(4))
def test_G3_exchange(oracle, idx):
    g = G['G3_exchange'][idx]
    etot = np.array(g['pe']) + np.array(g['ke'])
    swaps, perm, _, _, _ = oracle.exchange(g['np'], g['nt'], 0, g['np'], 256, 0, etot, g['vol'], g['et'], g['pf'],
                                           tape=g['uniforms'])
    assert list(perm) == g['perm']
    assert len(g['uniforms']) == g['np'] * g['nt'] * (g['nt'] - 1) // 2     # one draw per pair, remcmc:795


@pytest.mark.parametrize('idx', range(3))
def test_G3_exchange_al(oracle, idx):
    """the same sweep on metal-unit states (energies in eV, volumes in A^3) and the constants of init_constants() for el='Al'"""
    g = G['G3_exchange_al'][idx]
    got = [remcmc.init_constant(np.float32(g['P']), np.float32(g['T']), 'Al', i, j) for i in range(g['np']) for j in range(g['nt'])]
    np.testing.assert_array_equal([a for a, b in got], g['et'])
    np.testing.assert_array_equal([b for a, b in got], g['pf'])
    etot = np.array(g['pe']) + np.array(g['ke'])
    swaps, perm, _, _, _ = oracle.exchange(g['np'], g['nt'], 0, g['np'], 256, 0, etot, g['vol'], g['et'], g['pf'],
                                           tape=g['uniforms'])
    assert list(perm) == g['perm']
    assert list(perm) != list(range(g['np'] * g['nt']))
    assert len(g['uniforms']) == g['np'] * g['nt'] * (g['nt'] - 1) // 2


def test_G4_formats(tmp_path):
    g = G['G4_formats']
    run = remcmc.Run(['-n', 'golden', '-e', 'LJ', '-ss', '4', '-pn', '2', '-tn', '2', '-sn', '1024', '-sm', '128'],
                     cwd=str(tmp_path))
    assert run.header_text(3) == g['header_k3']
    assert os.path.basename(run.file_prefix(1, 1) + '.thrm') == g['thrm_name_k3']
    st = g['state']
    assert run.thrm_text(st['row']) == g['thrm_row']
    assert run.traj_text(st['natoms'], st['box'], st['x']) == g['traj_block']


def test_G5_command_strings():
    c = G['G5_command_strings']['bulk']
    # '%f' quantisation visible in the strings the reference sends to LAMMPS (remcmc:466,483)
    assert c[0] == 'change_box all x final 0.0 6.170386 y final 0.0 6.170386 z final 0.0 6.170386 units box'
    assert any(s.startswith('displace_atoms all random 0.035063 0.035063 0.035063 ') for s in c)


def test_G5_command_strings_al():
    """metal units: T in K, the displacement dx * 4.046 in A and the timestep in ps, each through '%f' (remcmc:466,483,604,607)"""
    c = G['G5_command_strings_al']
    assert c['bulk_4'][0] == 'change_box all x final 0.0 16.219574 y final 0.0 16.219574 z final 0.0 16.219574 units box'
    assert c['bulk_4'][2] == 'displace_atoms all random 0.016184 0.016184 0.016184 424 units box'          # 0.004 * 4.046
    assert any(s.startswith('displace_atoms all random 0.012138 0.012138 0.012138 ') for s in c['default_mix_5'])  # 0.003 * 4.046
    for name in AL_TRACES:
        hmc = [s for s in c[name] if s.startswith(('velocity all create', 'timestep'))]
        assert hmc or name.startswith('iter'), name       # iter's first 40 commands are its per-atom `run 0`
        for s in hmc:
            assert s == 'timestep 0.003906' or re.fullmatch(r'velocity all create 300\.000000 \d+ dist gaussian', s), (name, s)
    box = float(BA['bulk_4_0_scal_in'][0])
    assert c['bulk_4'][0].split()[5] == '%f' % box and float('%f' % box) != box           # the box edge is rounded


@pytest.mark.parametrize('name', AL_TRACES)
def test_G5_blocks_oracle_al(oracle, name):
    """the oracle's run_block in metal units (units=1, mass 29.982, Sutton-Chen) replays the reference's gen_sample traces for
    element Al at 4^3 and 5^3"""
    mod, ppos, pvol, nstps, bm = BA[name + '_params']
    n = 4 * int(name[-1]) ** 3
    for k in range(4):
        pre = '%s_%d_' % (name, k)
        box, dx, dv, dt, et, pf, t = BA[pre + 'scal_in']
        s = oracle.Sim(n, units=1, mass=lattice.MASS['Al'], pot=1)
        s.set_rng(256, k, 3)
        out = s.run_block(BA[pre + 'x_in'], BA[pre + 'v_in'], box, [dx, dv, dt], mod=int(mod), nstps=int(nstps), bulk=bool(bm),
                          ppos=ppos, pvol=pvol, lat=4.046, t=t, et=et, pf=pf, tape=BA[pre + 'tape'])
        s.close()
        assert out['tape_used'] == len(BA[pre + 'tape'])
        row = BA[pre + 'row_out']
        np.testing.assert_array_equal(out['counters'], row[8:14])
        np.testing.assert_array_equal(out['ratios'], row[14:17].astype(np.float32))
        np.testing.assert_allclose(out['thermo'], row[:5], rtol=1e-9)
        np.testing.assert_allclose(out['box'], BA[pre + 'box_out'][0], rtol=0, atol=0)
        np.testing.assert_allclose(out['x'], BA[pre + 'x_out'], rtol=0, atol=1e-9)
        np.testing.assert_allclose(out['v'], BA[pre + 'v_out'], rtol=0, atol=1e-9)


def test_G5_al_traces_accept_and_reject_every_move_kind():
    """over the four slots of each trace, every kind of move the tag draws was both accepted and rejected by the reference"""
    for name in AL_TRACES:
        c = np.array([BA['%s_%d_row_out' % (name, k)][8:14] for k in range(4)]).sum(0)
        for tries, acc in c.reshape(3, 2):
            assert 0 < acc < tries, (name, c)


@pytest.mark.parametrize('tag', ['bulk', 'iter', 'default_mix'])
def test_G5_blocks_oracle(oracle, tag):
    """the oracle's own run_block, fed the uniforms the reference drew, reproduces what the reference's gen_sample
    produced when it drove the same primitives one LAMMPS command at a time"""
    mod, ppos, pvol, nstps, bm = B[tag + '_params']
    for k in range(4):
        pre = '%s_%d_' % (tag, k)
        box, dx, dv, dt, et, pf, t = B[pre + 'scal_in']
        s = oracle.Sim(256)
        s.set_rng(256, k, 3)
        out = s.run_block(B[pre + 'x_in'], B[pre + 'v_in'], box, [dx, dv, dt], mod=int(mod), nstps=int(nstps), bulk=bool(bm),
                          ppos=ppos, pvol=pvol, lat=1.122, t=t, et=et, pf=pf, tape=B[pre + 'tape'])
        assert out['tape_used'] == len(B[pre + 'tape'])          # same number of draws in the same order
        row = B[pre + 'row_out']
        np.testing.assert_array_equal(out['counters'], row[8:14])
        np.testing.assert_array_equal(out['ratios'], row[14:17].astype(np.float32))
        np.testing.assert_allclose(out['thermo'], row[:5], rtol=1e-9)
        np.testing.assert_allclose(out['box'], B[pre + 'box_out'][0], rtol=0, atol=0)
        np.testing.assert_allclose(out['x'], B[pre + 'x_out'], rtol=0, atol=1e-9)
        np.testing.assert_allclose(out['v'], B[pre + 'v_out'], rtol=0, atol=1e-9)
