"""nm_eval at every lj/cut and 4^3 Al row of the configuration table (nm_rows.hip NM_CFG_ROWS), against the exact all-pairs reference
(tests/exact_ref.py), at ragged atom counts and on the edge states: pairs at the cutoff and at the list radius, through every periodic
image, at L / 2, on the faces, unwrapped, close contacts, boxes from 2 rc to just above 2 (rc + skin), EAM atoms with nothing inside rc.

Per slot: status 0, the pair count of stats() exact, U and W to 1e-11 relative, every force component within the bound derived from
the kernels' arithmetic (exact_ref.force_bound; the half-list kernels add their fixed-point quantum).  What must be refused is: a box
below 2 rc (box edge < 2*rc), and on the half-list kernels a force beyond their fixed-point range (a pair closer than 0.604 sigma)."""
import functools

import numpy as np
import pytest

import exact_ref as X
from helpers import grids

pytestmark = pytest.mark.gpu

LJ_N = (2, 5, 33, 63, 65, 100, 255, 256, 257, 499, 500, 863, 864, 865, 1372, 2047, 2048)
AL_N = (2, 100, 255, 256)


def kind(n):
    return 0 if n <= 256 else 1 if n <= 864 else 2


def qs(el, n):
    """workgroups per replica with a row in the configuration table (nm_rows.hip NM_CFG_ROWS): the names are the Cfg typedefs"""
    if el == 'Al':
        return {1: 'CfgSmallSC', 2: 'CfgSmallSCQ2', 4: 'CfgSmallSCQ4'}
    return [{1: 'CfgSmall', 2: 'CfgSmallQ2', 4: 'CfgSmallQ4', 8: 'CfgSmallQ8'},
            {1: 'CfgMidH', 2: 'CfgMid', 4: 'CfgMidQ4', 8: 'CfgMidQ8'},
            {1: 'CfgLargeH', 2: 'CfgLarge', 4: 'CfgLarge'}][kind(n)]


CASES = [pytest.param(el, n, q, id='%s-%d-%s' % (el, n, cfg)) for el, ns in (('LJ', LJ_N), ('Al', AL_N)) for n in ns
         for q, cfg in qs(el, n).items()]
# the half-list instantiations (Cfg::HALF): forces summed in 64-bit fixed point, range 2^15 force units
HALF = {'CfgMidH', 'CfgLargeH'}
R_FIX = 0.604173  # |F(r)| = 2^15 for lj/cut


@functools.lru_cache(maxsize=None)
def reference(el, n):
    """edge states of n atoms with their exact U, W, f, pair count and force bounds (computed once per (el, n))"""
    L = X.box_for(el, n, 0.9 if el == 'LJ' else 0.055)
    out = []
    for name, x, LL in X.edge_states(el, n, L, seed=3) + X.box_edge_states(el, n, seed=3):
        U, W, f, npairs, _ = X.exact(el, x, LL)
        out.append(dict(name=name, x=x, L=LL, U=float(U), W=float(W), f=f, npairs=npairs,
                        b=X.force_bound(el, x, LL), bh=X.force_bound(el, x, LL, half=True)))
    return out


def refused_on_half(st):
    return st['name'].startswith('contact_') and float(st['name'].split('_')[1]) < R_FIX


@pytest.mark.parametrize('el,n,q', CASES)
def test_eval_edges(monkeypatch, el, n, q):
    import neuralmelting_amd as nm
    from neuralmelting_amd.engine import NMError
    monkeypatch.setenv('NM_CUS_PER_REPLICA', str(q))
    cfg = qs(el, n)[q]
    half = cfg in HALF
    sts = reference(el, n)
    ok = [s for s in sts if not (half and refused_on_half(s))]
    bad = [s for s in sts if half and refused_on_half(s)]
    P, T = grids(1, len(ok))
    e = nm.Engine(n, P, T, element=el)
    try:
        assert e.cus_per_replica == q, (cfg, e.cus_per_replica, e.note())
        d = np.tile([0.03125, 0.03125, 0.00390625], (len(ok), 1))
        e.set_state(np.stack([s['x'].reshape(-1) for s in ok]), np.zeros((len(ok), 3 * n)), [s['L'] for s in ok], d)
        e.stats(reset=True)
        U, W, f = e.eval()
        assert (e.status() == 0).all()
        st = e.stats()
        for k, s in enumerate(ok):
            tag = (cfg, s['name'], s['L'])
            assert st[k, 3] == s['npairs'], tag
            assert abs(U[k] - s['U']) <= 1e-11 * abs(s['U']), (tag, U[k], s['U'])
            assert abs(W[k] - s['W']) <= 1e-11 * abs(s['W']), (tag, W[k], s['W'])
            err = np.abs(f[k].reshape(-1, 3) - s['f'])
            b = s['bh'] if half else s['b']
            assert np.all(err <= b), (tag, float(err.max()), float((err / np.maximum(b, 1e-300)).max()))
        # a force beyond the fixed-point range of the half-list kernels is reported, never returned
        for s in bad:
            e.set_state(s['x'].reshape(1, -1), None, [s['L']], None, k0=0, nk=1)
            with pytest.raises(NMError, match='fixed-point range'):
                e.eval()
            assert e.status()[0] == 64  # NM_ST_FORCE_RANGE
        # below the minimum-image limit: refused with the existing error, and the context stays usable
        s = ok[0]
        e.set_state(s['x'].reshape(1, -1), None, [2 * X.RC[el] * (1 - 1e-9)], None, k0=0, nk=1)
        with pytest.raises(NMError, match=r'box edge < 2\*rc'):
            e.eval()
        e.set_state(s['x'].reshape(1, -1), None, [s['L']], None, k0=0, nk=1)
        U2, _, _ = e.eval(forces=False)
        assert U2[0] == U[0]
    finally:
        e.close()
