"""The VAE stage against tests/golden/ref_vae.json: every output of the cases of tests/vae_cases.py, byte for byte what the library
wrote before the network of csrc/nm_vae_api.hip was put into one table of layers (the maker: tests/golden/make_golden_vae.py).
The stage is deterministic ("the same call twice gives the same bits"), so nothing but a change of its arithmetic, of the order of
a sum, of a buffer or of a parameter's place moves a byte."""
import functools
import json
import os

import numpy as np
import pytest

import vae_cases as V

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_vae.json')) as f:
        return json.load(f)['cases']


def compare(key, out):
    want = golden()[key]['outputs']
    assert sorted(out) == sorted(want)
    for name, a in out.items():                                     # where the fixture holds the values, the difference is shown
        if 'values' in want[name]:
            np.testing.assert_array_equal(a.ravel(), np.array(want[name]['values'], dtype=a.dtype), err_msg='%s of %s' % (name, key))
    wrong = [name for name, a in out.items() if V.digest(a) != want[name]]
    assert not wrong, '%s: %s differ from the fixture' % (key, wrong)


def test_the_fixture_holds_every_case_and_no_other():
    assert sorted(key for key, _ in V.every_case()) == sorted(golden())
    assert V.MODEL_CASES == ((4, 1, 3, 2), (8, 3, 5, 2), (12, 2, 2, 2), (16, 8, 66, 3)) and V.DENSE['dout'] >= 1024


@pytest.mark.parametrize('side,latent,n,batch', V.MODEL_CASES)
def test_model(side, latent, n, batch):
    compare(V.model_key(side, latent, n, batch), V.model_case(side, latent, n, batch))


@pytest.mark.parametrize('name', V.PRIMITIVE_CASES)
def test_primitive(name):
    compare(name, V.primitive_case(name))
