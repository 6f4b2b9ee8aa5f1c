"""The all-pairs scans of the cluster and the manifold stage against tests/golden/ref_scan.json: every output of the cases of
tests/scan_cases.py, byte for byte what the library wrote before both stages' scans were put on csrc/nm_scan.h (the maker:
tests/golden/make_golden_scan.py).  Both stages are deterministic ("identical bytes on every call", labels that are "a property of
the input alone"), so nothing but a change of their arithmetic, of the order of a sum or of a tie's rule moves a byte."""
import functools
import json
import os

import numpy as np
import pytest

import scan_cases as S

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_scan.json')) as f:
        return json.load(f)['cases']


@functools.lru_cache(maxsize=None)
def affinities(n, nd):
    """computed once: the gradient's cases run on these lists"""
    rc, msg, out = S.affinity_call(n, nd)
    for a in out.values():
        a.setflags(write=False)
    return rc, msg, out


def compare(key, out):
    want = golden()[key]
    assert sorted(out) == sorted(want['outputs'])
    for name, a in out.items():                                     # where the fixture holds the arrays, the difference is shown
        if 'arrays' in want:
            np.testing.assert_array_equal(a, np.array(want['arrays'][name], dtype=a.dtype), err_msg='%s of %s' % (name, key))
    for name, a in out.items():
        assert S.digest(a) == want['outputs'][name], '%s of %s' % (name, key)


def test_the_fixture_holds_every_case_and_no_other():
    keys = ([S.cluster_key(n, nd) for n in S.CL_N for nd in S.CL_ND] + [S.affinity_key(n, nd) for n in S.AF_N for nd in S.AF_ND]
            + [S.gradient_key(n, nc) for n in S.GR_N for nc in S.GR_NC])
    assert sorted(keys) == sorted(golden())
    assert S.CL_N[-1] == 2 * S.CL_ROWS + S.CL_TILE + 7 == 1287 and S.AF_N[-1] == 2 * S.TS_ROWS + S.TS_TILE + 7 == 1159


@pytest.mark.parametrize('nd', S.CL_ND)
@pytest.mark.parametrize('n', S.CL_N)
def test_cluster(n, nd):
    compare(S.cluster_key(n, nd), S.cluster_case(n, nd))


@pytest.mark.parametrize('nd', S.AF_ND)
@pytest.mark.parametrize('n', S.AF_N)
def test_affinities(n, nd):
    rc, msg, out = affinities(n, nd)
    want = golden()[S.affinity_key(n, nd)]
    if 'rc' in want:                                                # the refusal at N = 3: the code, the message, nothing written
        assert (rc, msg) == (want['rc'], want['message']) and all((a == -77).all() for a in out.values())
        return
    assert rc == S.B.NM_OK, msg
    compare(S.affinity_key(n, nd), out)


@pytest.mark.parametrize('nc', S.GR_NC)
@pytest.mark.parametrize('n', S.GR_N)
def test_gradient_and_descent(n, nc):
    rc, msg, lists = affinities(n, S.AF_ND[-1])
    assert rc == S.B.NM_OK, msg
    compare(S.gradient_key(n, nc), S.gradient_case(n, nc, lists))
