"""CPU tests of the ctypes binding (neuralmelting_amd/_lib.py): its one prototype table against the declarations of include/*.h type by
type, the pointer types that take numpy arrays, and call(), the one way a stage raises a library error."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from neuralmelting_amd import _lib as B
from neuralmelting_amd import vae

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ('nm.h', 'nm_distr.h', 'nm_parse.h', 'nm_reweight.h', 'nm_reweight_hist.h', 'nm_reweight_boot.h', 'nm_pca.h', 'nm_cluster.h',
           'nm_tsne.h', 'nm_vae.h')
TUPLES = ('SYMBOLS', 'DISTR_SYMBOLS', 'PARSE_SYMBOLS', 'REWEIGHT_SYMBOLS', 'REWEIGHT_HIST_SYMBOLS', 'REWEIGHT_BOOT_SYMBOLS', 'PCA_SYMBOLS',
          'CLUSTER_SYMBOLS', 'TSNE_SYMBOLS', 'VAE_SYMBOLS')
CTX, CTX_P = C.c_void_p, C.POINTER(C.c_void_p)
# the C type texts of the headers and what the binding must declare for each; a text that is missing here fails the test
CTYPES = {
    'int': C.c_int, 'long': C.c_long, 'int64_t': C.c_int64, 'uint32_t': C.c_uint32, 'double': C.c_double,
    'double *': B.c_double_p, 'const double *': B.c_double_p, 'float *': B.c_float_p, 'const float *': B.c_float_p,
    'int *': B.c_int_p, 'const int *': B.c_int_p, 'int32_t *': B.c_int32_p, 'const int32_t *': B.c_int32_p,
    'int64_t *': B.c_int64_p, 'const int64_t *': B.c_int64_p, 'uint16_t *': B.c_uint16_p, 'const uint16_t *': B.c_uint16_p,
    'uint64_t *': B.c_uint64_p, 'unsigned long long *': B.c_uint64_p, 'long *': B.c_long_p,
    'char *': C.c_char_p, 'const char *': C.c_char_p, 'const char *const *': C.POINTER(C.c_char_p),
    'nm_ctx *': CTX, 'const nm_ctx *': CTX, 'nm_vae_ctx *': CTX, 'nm_ctx **': CTX_P, 'nm_vae_ctx **': CTX_P,
    'const nm_config *': C.POINTER(B.NMConfig)}


def _type(text):
    """the ctypes type of a C type text, whatever its spacing"""
    return {re.sub(r'\s*\*\s*', '*', k): v for k, v in CTYPES.items()}[re.sub(r'\s*\*\s*', '*', ' '.join(text.split()))]


def declarations(header):
    """[(name, restype, argtypes)] of a header in its order, comments stripped as test_abi.declared_symbols strips them"""
    txt = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', header)).read(), flags=re.S)
    out = []
    for ret, name, params in re.findall(r'^((?:const )?\w+ \*?)(nm_[a-z_0-9]+)\s*\(([^)]*)\)\s*;', txt, flags=re.M):
        params = [] if params.strip() == 'void' else [re.fullmatch(r'(.*?)\w+', ' '.join(p.split())).group(1) for p in params.split(',')]
        out.append((name, _type(ret), [_type(p) for p in params]))
    assert sorted(n for n, _, _ in out) == sorted(set(re.findall(r'\b(nm_[a-z_0-9]+)\s*\(', txt))), header    # no declaration slipped by
    return out


def test_every_header_has_its_entry():
    assert tuple(B.PROTOTYPES) == HEADERS == tuple(sorted(os.listdir(os.path.join(ROOT, 'include')), key=HEADERS.index))
    for header, name in zip(HEADERS, TUPLES):
        assert getattr(B, name) == tuple(B.PROTOTYPES[header][1]), name
    for header, (error, symbols) in B.PROTOTYPES.items():
        stage = 'nm_reweight' if header.startswith('nm_reweight') else header[:-2]
        assert error == (None if header == 'nm.h' else stage + '_last_error')
        assert error is None or error in B.PROTOTYPES[stage + '.h'][1]


@pytest.mark.parametrize('header', HEADERS)
def test_table_equals_header(header):
    declared = declarations(header)
    table = B.PROTOTYPES[header][1]
    assert list(table) == [name for name, _, _ in declared]
    L = B.load()
    for name, restype, argtypes in declared:
        assert table[name] == (restype, argtypes), name
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name      # and load() set what the table says


# ---- the pointer types, through library functions that need no device

def _thrm(row):
    buf = C.create_string_buffer(17 * 14 + 8)
    n = B.load().nm_format_thrm(row, buf, len(buf))
    assert n > 0
    return buf.raw[:n]


def test_an_array_is_its_pointer():
    row = np.arange(17, dtype=np.float64) * 1.25 - 3.0
    text = _thrm(row)
    assert text == _thrm(row.ctypes.data_as(B.c_double_p)) == _thrm(row.ctypes.data_as(C.POINTER(C.c_double)))
    assert text.decode() == ''.join(' %.4E' % v for v in row) + '\n'
    frozen = row.copy()
    frozen.flags.writeable = False                   # the inputs are often memory maps
    assert _thrm(frozen) == text
    assert B.load().nm_format_thrm.argtypes[0] is B.c_double_p and issubclass(B.c_double_p, C.POINTER(C.c_double))


def _angles(pos, box, ce, adf, natoms=0):
    return B.load().nm_distr_angles(0, 1, natoms, pos, box, 0.0, 1.0, 2, ce, adf)


def test_arrays_none_and_byref_reach_the_library():
    f4, f8, u8 = np.zeros(3, np.float32), np.zeros(2), np.zeros(2, np.uint64)
    assert _angles(f4, f4, f8, u8) == B.NM_ERR_ARG and B.load().nm_distr_last_error().startswith(b'nm_distr_angles:')   # natoms = 0
    assert _angles(None, f4, f8, None, natoms=1) == B.NM_ERR_ARG
    n = C.c_long(-7)
    assert B.load().nm_parse_thrm(b'/nonexistent/x.thrm', None, 0, C.byref(n), 1) == B.NM_ERR_ARG


@pytest.mark.parametrize('case', ['float32 for double', 'int64 for int32', 'strided', 'list'])
def test_a_wrong_array_never_reaches_the_library(case):
    L = B.load()
    f4, f8, u8 = np.zeros(3, np.float32), np.zeros(2), np.zeros(2, np.uint64)
    before = L.nm_distr_last_error(), L.nm_cluster_last_error()
    with pytest.raises(C.ArgumentError) as err:
        if case == 'float32 for double':
            _angles(f4, f4, f4, u8)
        elif case == 'int64 for int32':
            L.nm_cluster_dbscan(0, 2, 0, f8, 0.5, 2, np.zeros(2, np.int64), np.zeros(2, np.int32), np.zeros(1, np.int32))
        elif case == 'strided':
            _angles(f4, f4, np.zeros(4)[::2], u8)
        else:
            _angles(f4, f4, [0.0, 1.0], u8)
    assert (L.nm_distr_last_error(), L.nm_cluster_last_error()) == before        # raised before the call
    if case == 'float32 for double':
        assert 'float64' in str(err.value) and 'float32' in str(err.value)
    if case == 'int64 for int32':
        assert 'int32' in str(err.value) and 'int64' in str(err.value)


# ---- call(): one refusal of every stage, each before a device is looked for; the text of the header's own error function

def _refusals():
    d, f4, i32 = np.zeros(4), np.zeros(3, np.float32), np.zeros(4, np.int32)
    states = (0, 0, None, None, None)                # nstates = 0: the first check, no pointer is looked at
    return {
        'nm_reweight_expect': states + (None, 1, None, None, 1, None, None, 0, None, None, None, None, None, None),
        'nm_reweight_histogram': states + (None, 1, None, None, 1, None, None, 1, None, 1, None, None, None),
        'nm_reweight_boot_solve': states + (1, None, None, None, 1, None, 1e-9, 1, None, None, None, None),
        'nm_distr_angles': (0, 1, 0, f4, f4, 0.0, 1.0, 2, d, np.zeros(2, np.uint64)),
        'nm_pca_moments': (0, 1, 1, None, d, d, d, d),
        'nm_cluster_dbscan': (0, 2, 0, d, 0.5, 2, i32, i32, i32),
        'nm_tsne_affinities': (0, 6, 0, d, 2.0, 4, i32, d, d),
        'nm_vae_nparams': (7, 8)}


@pytest.mark.parametrize('name', sorted(_refusals()))
def test_call_raises_the_header_s_message(name):
    error = next(e for e, symbols in B.PROTOTYPES.values() if name in symbols)
    with pytest.raises(RuntimeError) as err:
        B.call(name, *_refusals()[name])
    message = getattr(B.load(), error)().decode()
    assert message.startswith(name + ':')
    assert str(err.value) == '%s failed (-1): ' % name + message


def test_call_returns_the_value():
    assert B.call('nm_vae_nparams', 8, 8) == vae.layout(8, 8)[-1] > 0
    with pytest.raises(RuntimeError) as err:         # parse's form of the text
        B.call('nm_parse_thrm', b'/nonexistent/x.thrm', None, 0, C.byref(C.c_long(0)), 1, form='{0}: {2}')
    assert str(err.value) == 'nm_parse_thrm: ' + B.load().nm_parse_last_error().decode()
