"""nm_set_state / nm_get_state / nm_get_slots / nm_set_slots on every path they take (few slots, the staged whole arrays on a full and
on a partial range, slot lists) under a slot map that is not the identity.  No block is launched: a 2 x 6 grid of 5-atom replicas, the
map permuted by one exchange sweep that accepts every pair.  Every double written encodes (generation, slot, field, index), so a value
that lands in the wrong slot, array or buffer shows, and everything is compared exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NATOMS, NP, NT = 5, 2, 6
NS, N3 = NP * NT, 3 * NATOMS
FX, FV, FD = 1, 2, 4


def code(gen, slot, field, n):
    return (gen * 2.0 ** 16 + slot * 2.0 ** 10 + field * 2.0 ** 7) + np.arange(n, dtype=np.float64)


def box_of(gen, slot):
    return 1.0 + (gen * 16 + slot) / 64.0  # ten significant bits: the cube is exact in a double however it is computed


class Model:
    """what every logical slot holds"""

    def __init__(self, th):
        self.x, self.v = np.zeros((NS, N3)), np.zeros((NS, N3))
        self.box, self.d, self.th = np.zeros(NS), np.zeros((NS, 3)), np.array(th)

    def values(self, gen, slots):
        x = np.stack([code(gen, k, FX, N3) for k in slots])
        v = np.stack([code(gen, k, FV, N3) for k in slots])
        box = np.array([box_of(gen, k) for k in slots])
        d = np.stack([code(gen, k, FD, 3) for k in slots])
        return x, v, box, d

    def write(self, slots, x=None, v=None, box=None, dxdvdt=None, th=None):
        sl = np.asarray(slots, dtype=int)
        if x is not None: self.x[sl] = x
        if v is not None: self.v[sl] = v
        if box is not None:
            self.box[sl] = box
            self.th[sl, 4] = np.asarray(box) ** 3
        if dxdvdt is not None: self.d[sl] = dxdvdt
        if th is not None: self.th[sl] = th  # (behind the box: the list's thermo row wins column 4)


def fresh():
    """an engine whose slot map is a known non-identity permutation, filled with recognisable state, and its model"""
    import neuralmelting_amd as nm
    e = nm.Engine(NATOMS, np.linspace(1, 8, NP, dtype=np.float32), np.linspace(0.25, 2.5, NT, dtype=np.float32))
    assert e.nslots == NS
    th0 = np.array([[k + 0.25, -100.0 - k, 50.0 + k, 7.0 + k, 200.0 + k] for k in range(NS)])
    e.set_thermo(th0)
    e.set_exchange_tape(np.zeros(NP * NT * (NT - 1) // 2))  # a uniform of zero accepts every pair
    e.exchange()
    perm = e.perm()
    assert sorted(perm) == list(range(NS)) and list(perm) != list(range(NS)), 'the slot map must not be the identity'
    m = Model(th0[perm])  # the thermo rows went into the buffers under the identity map: slot k now reads buffer perm[k]
    x, v, box, d = m.values(0, range(NS))
    e.set_state(x, v, box, d)
    m.write(range(NS), x, v, box, d)
    return e, m


def eq(a, b):
    np.testing.assert_array_equal(np.asarray(a).reshape(np.shape(b)), b)


def check_range(e, m, k0, nk):
    for vel in (True, False):
        x, v, box, d = e.get_state(k0, nk, velocities=vel)
        sl = slice(k0, k0 + nk)
        eq(x, m.x[sl]); eq(box, m.box[sl]); eq(d, m.d[sl])
        if vel: eq(v, m.v[sl])
        else: assert v is None


def check_slots(e, m, slots):
    for vel in (True, False):
        x, v, box, d, th = e.get_slots(slots, velocities=vel)
        sl = np.asarray(slots, dtype=int)
        eq(x, m.x[sl]); eq(box, m.box[sl]); eq(d, m.d[sl]); eq(th, m.th[sl])
        if vel: eq(v, m.v[sl])
        else: assert v is None


def check_all(e, m):
    check_range(e, m, 0, NS)
    check_slots(e, m, list(range(NS)))


@pytest.fixture(scope='module')
def filled():
    e, m = fresh()
    yield e, m
    e.close()


def test_get_state_all_slots(filled):
    check_range(*filled, 0, NS)


@pytest.mark.parametrize('nk', [1, 8])
@pytest.mark.parametrize('k0', [0, 1, 3])
def test_get_state_few_slots(filled, k0, nk):
    check_range(*filled, k0, nk)


@pytest.mark.parametrize('k0,nk', [(0, 9), (1, 9), (3, 9), (0, 11), (1, 11)])
def test_get_state_partial_range_staged(filled, k0, nk):
    check_range(*filled, k0, nk)


def test_get_slots_unordered_repeated(filled):
    e, m = filled
    slots = [7, 2, 11, 2, 0, 9]
    check_slots(e, m, slots)
    th = e.get_slots(slots)[4]
    eq(th[:, 4], m.box[slots] ** 3)
    eq(th[:, :4], np.array([[k + 0.25, -100.0 - k, 50.0 + k, 7.0 + k] for k in e.perm()[slots]]))  # what nm_set_thermo wrote


SUBSETS = [('x',), ('v', 'box'), ('dxdvdt',), ('box',), ('x', 'v', 'box', 'dxdvdt')]


def subset(m, gen, slots, names):
    x, v, box, d = m.values(gen, slots)
    full = dict(x=x, v=v, box=box, dxdvdt=d)
    return {n: full[n] for n in names}


@pytest.mark.parametrize('k0,nk', [(5, 2), (1, 10)])  # the few-slots path and the merge into the staged arrays
def test_set_state_partial(k0, nk):
    e, m = fresh()
    slots = list(range(k0, k0 + nk))
    for gen, names in enumerate(SUBSETS, 1):
        kw = subset(m, gen, slots, names)
        th_before = m.th.copy()
        e.set_state(k0=k0, nk=nk, **kw)
        m.write(slots, **kw)
        check_all(e, m)  # the slots outside the range and the arrays not passed are as they were
        eq(m.th[:, :4], th_before[:, :4])
        if 'box' in names: eq(m.th[slots, 4], m.box[slots] ** 3)
    e.close()


def test_set_slots():
    e, m = fresh()
    slots = [7, 2, 9]
    gen = 0
    for names in SUBSETS:  # without th
        gen += 1
        kw = subset(m, gen, slots, names)
        e.set_slots(slots, **kw)
        m.write(slots, **kw)
        check_all(e, m)
        if 'box' in names: eq(m.th[slots, 4], m.box[slots] ** 3)
    th = np.stack([code(9, k, 5, 5) for k in slots])
    e.set_slots(slots, th=th)  # th alone
    m.write(slots, th=th)
    check_all(e, m)
    # box and th together: the box is written with its volume, then the thermo row, whose column 4 is what stays
    kw = subset(m, 10, slots, ('box', 'x'))
    th = np.stack([code(11, k, 5, 5) for k in slots])
    e.set_slots(slots, th=th, **kw)
    m.write(slots, th=th, **kw)
    eq(m.th[slots, 4], th[:, 4])
    assert not np.any(m.th[slots, 4] == m.box[slots] ** 3)
    check_all(e, m)
    e.close()


def test_refusals_keep_code_and_text(filled):
    import neuralmelting_amd as nm
    from neuralmelting_amd import _lib as B
    e, m = filled
    L, h = e.lib, e.h

    def refused(call, text):
        with pytest.raises(nm.NMError) as err:
            call()
        assert err.value.code == B.NM_ERR_ARG
        assert L.nm_last_error(h).decode() == text

    refused(lambda: e.get_state(5, 8), 'nm_get_state: slot range')
    refused(lambda: e.get_state(-1, 2), 'nm_get_state: slot range')
    refused(lambda: e.set_state(x=np.zeros((8, N3)), k0=5, nk=8), 'nm_set_state: slot range')
    refused(lambda: e.set_state(box=np.zeros(2), k0=-1, nk=2), 'nm_set_state: slot range')
    refused(lambda: e.get_slots([0, NS]), 'nm_get_slots: slot out of range')
    refused(lambda: e.set_slots([3, -1], box=np.ones(2)), 'nm_set_slots: slot out of range')
    assert L.nm_get_slots(h, 1, None, None, None, None, None, None) == B.NM_ERR_ARG
    assert L.nm_last_error(h).decode() == 'nm_get_slots: bad argument'
    assert L.nm_set_slots(h, 1, None, None, None, None, None, None) == B.NM_ERR_ARG
    assert L.nm_last_error(h).decode() == 'nm_set_slots: bad argument'
    # nothing to do is accepted
    box = np.ones(1)
    bp = box.ctypes.data_as(B.c_double_p)
    assert L.nm_get_slots(h, 0, None, None, None, bp, None, None) == B.NM_OK
    assert L.nm_set_slots(h, 0, None, None, None, bp, None, None) == B.NM_OK
    assert L.nm_get_state(h, NS, 0, None, None, bp, None) == B.NM_OK
    assert L.nm_set_state(h, NS, 0, None, None, bp, None) == B.NM_OK
    assert L.nm_set_state(h, 3, 0, None, None, bp, None) == B.NM_OK
    assert box[0] == 1.0
    assert L.nm_last_error(h) == b''  # (empty after a call that returned NM_OK)
    check_all(e, m)  # and a refused call changed nothing
