"""ctypes binding of libnm_hip.so (include/*.h).  There is no CPU fallback: if the HIP library is missing or cannot be loaded this
module raises, it never substitutes another implementation.

Three things, and a stage needs nothing else to reach the library:
- prototypes: PROTOTYPES holds every header's symbols with their restype and argtypes, and the header's `*_last_error`.  load() sets
  them in one loop; tests/test_binding.py compares the table with include/*.h type by type.  A new stage adds its header's entry to
  _prototypes() and nothing anywhere else.
- arrays: a pointer parameter (c_double_p, c_float_p, ...) takes the numpy array itself, provided its dtype is the element type and
  it is C-contiguous; anything else is a TypeError (ctypes.ArgumentError at the call), never a conversion or a reinterpretation.
  None, C.byref(...) and ready-made pointers pass as they do with a plain C.POINTER type.  So a wrapper coerces with
  np.ascontiguousarray(..., dtype=...) and hands the arrays over.
- errors: call(name, *args) returns the function's value, or for a negative one raises RuntimeError with the message of the
  header's error function.  (The sampler's context has a channel of its own: engine.Engine, NMError, nm_last_error(ctx).)"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('NM_HIP_LIB') or os.path.join(_HERE, 'libnm_hip.so')  # NM_HIP_LIB: dev override (diagnostic builds)


def _array_pointer(ctype):
    """C.POINTER(ctype) as a parameter type that also takes a C-contiguous numpy array of exactly that element type"""
    base, dtype = C.POINTER(ctype), np.dtype(ctype)

    class pointer(base):
        _type_ = ctype

        @classmethod
        def from_param(cls, obj):
            if not isinstance(obj, np.ndarray):
                return base.from_param(obj)           # (from_param lives on the metaclass: there is no super() to ask)
            if obj.dtype != dtype or not obj.flags.c_contiguous:
                raise TypeError('wants a C-contiguous %s array, got %s%s' % (dtype, obj.dtype, '' if obj.flags.c_contiguous else ', strided'))
            return obj.ctypes.data_as(cls)

    pointer.__name__ = pointer.__qualname__ = ctype.__name__ + '_p'
    return pointer


c_double_p, c_float_p, c_int_p, c_long_p = (_array_pointer(t) for t in (C.c_double, C.c_float, C.c_int, C.c_long))
c_int32_p, c_int64_p, c_uint16_p, c_uint64_p = (_array_pointer(t) for t in (C.c_int32, C.c_int64, C.c_uint16, C.c_uint64))

NM_OK, NM_ERR_ARG, NM_ERR_HIP, NM_ERR_STATE, NM_ERR_UNSUPPORTED = 0, -1, -2, -3, -4
NM_EL_LJ, NM_EL_AL, NM_EL_NI, NM_EL_CU = 0, 1, 2, 3
NM_THERMO_COLS, NM_TRACE_COLS, NM_STATS_COLS = 17, 4, 12
NM_VAE_ACT_NONE, NM_VAE_ACT_RELU, NM_VAE_ACT_TANH, NM_VAE_NTENSORS = 0, 1, 2, 26


class NMConfig(C.Structure):
    _fields_ = [('size', C.c_int32), ('element', C.c_int32), ('natoms', C.c_int32), ('np', C.c_int32),
                ('nt', C.c_int32), ('row0', C.c_int32), ('nrows', C.c_int32), ('nstps', C.c_int32),
                ('bulk', C.c_int32), ('iter_revert', C.c_int32), ('device', C.c_int32), ('seed', C.c_uint32),
                ('ppos', C.c_double), ('pvol', C.c_double), ('P', c_float_p), ('T', c_float_p),
                ('slot0', C.c_int32), ('nslots', C.c_int32)]


def _prototypes():
    """{header: (its error function or None, {symbol: (restype, argtypes)})}, headers and symbols in the order of include/"""
    i, l, i64, u32, d, s = C.c_int, C.c_long, C.c_int64, C.c_uint32, C.c_double, C.c_char_p
    h, hp, sp = C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_char_p)        # nm_ctx * and nm_vae_ctx *, their **, const char *const *
    D, F, I, L, I32, I64, U16, U64 = c_double_p, c_float_p, c_int_p, c_long_p, c_int32_p, c_int64_p, c_uint16_p, c_uint64_p
    frames = [i, i, i, F, F]                                                    # device, ns, natoms, pos, box
    states = [i, i, D, D, I64]                                                  # device, nstates, b, c, count
    return {
        'nm.h': (None, {                                                        # per context: Engine reads nm_last_error(ctx) itself
            'nm_create': (i, [C.POINTER(NMConfig), hp]),
            'nm_destroy': (i, [h]),
            'nm_last_error': (s, [h]),
            'nm_create_note': (s, [h]),
            'nm_nslots': (i, [h]),
            'nm_natoms': (i, [h]),
            'nm_cus_per_replica': (i, [h]),
            'nm_heal_count': (i, [h]),
            'nm_get_const': (i, [h, D, D]),
            'nm_set_state': (i, [h, i, i, D, D, D, D]),
            'nm_get_state': (i, [h, i, i, D, D, D, D]),
            'nm_get_slots': (i, [h, i, I, D, D, D, D, D]),
            'nm_set_slots': (i, [h, i, I, D, D, D, D, D]),
            'nm_init_lattice': (i, [h, d, d, i]),
            'nm_lattice_state': (i, [i, i, i, i, F, u32, i, d, i, D, D]),
            'nm_set_thermo': (i, [h, i, i, D]),
            'nm_set_step': (i, [h, u32]),
            'nm_run_md': (i, [h, i]),
            'nm_run_block': (i, [h, i]),
            'nm_run_cycles': (i, [h, i, i]),
            'nm_get_thermo': (i, [h, D]),
            'nm_snapshot': (i, [h]),
            'nm_snapshot_fetch': (i, [h, D, D, D]),
            'nm_run_cycles_recorded': (i, [h, i, i]),
            'nm_record_capacity': (i, [h]),
            'nm_snapshot_pending': (i, [h]),
            'nm_adapt': (i, [h]),
            'nm_exchange': (i, [h, I]),
            'nm_synchronize': (i, [h]),
            'nm_get_status': (i, [h, I]),
            'nm_timing_reset': (i, [h]),
            'nm_timing_get': (i, [h, I, D]),
            'nm_stats_get': (i, [h, D, i]),
            'nm_format_thrm': (i, [D, s, i]),
            'nm_format_traj': (i, [i, d, D, s, i]),
            'nm_append_outputs': (i, [i, i, sp, sp, D, D, D, i]),
            'nm_eval': (i, [h, D, D, D]),
            'nm_set_rng_tape': (i, [h, D, I]),
            'nm_set_exchange_tape': (i, [h, D, i]),
            'nm_set_trace': (i, [h, i]),
            'nm_get_trace': (i, [h, D, i]),
            'nm_set_counters': (i, [h, D, F]),
            'nm_get_perm': (i, [h, I]),
            'nm_get_exchange_crit': (i, [h, D, i])}),
        'nm_distr.h': ('nm_distr_last_error', {
            'nm_distr_histograms': (i, frames + [i, D, i, D, F, F]),
            'nm_distr_last_error': (s, []),
            'nm_distr_angles': (i, frames + [d, d, i, D, U64]),
            'nm_distr_sfactor': (i, frames + [i, D, D]),
            'nm_distr_bondorder': (i, frames + [d, d, i, I, D, D, D, I32]),
            'nm_distr_bondorder_w': (i, frames + [d, d, i, I, D, D, D, D, D, D, I32]),
            'nm_distr_solid': (i, frames + [d, d, i, d, i, I32, I32, I32, I32, I32]),
            'nm_distr_cna': (i, frames + [d, d, i, I32, I32, I32, I32]),
            'nm_distr_entropy': (i, frames + [d, d, i, d, d, D, D, I32, D, D, I32]),
            'nm_cluster_spectral': (i, [i, i64, i, D, d, i, i, D, i, i, d, D, D, D, D, I32]),
            'nm_cluster_spectral_last_timing': (i, [D]),
            'nm_cluster_kmeans': (i, [i, i64, i, D, i, i, D, i, d, I32, D, I32, D, I32, I32, I32]),
            'nm_cluster_kmeans_last_timing': (i, [D]),
            'nm_distr_lof': (i, [i, i64, i, i, D, i, D, D, D, I32]),
            'nm_distr_last_timing': (i, [D])}),
        'nm_parse.h': ('nm_parse_last_error', {
            'nm_parse_thrm': (i, [s, F, l, L, i]),
            'nm_parse_traj': (i, [s, U16, F, F, l, l, L, L, i]),
            'nm_parse_last_error': (s, [])}),
        'nm_reweight.h': ('nm_reweight_last_error', {
            'nm_reweight_solve': (i, states + [i64, D, D, d, i, D, D, I, D]),
            'nm_reweight_expect': (i, states + [D, i64, D, D, i, D, D, i, D, D, D, D, D, D]),
            'nm_reweight_last_error': (s, [])}),
        'nm_reweight_hist.h': ('nm_reweight_last_error', {
            'nm_reweight_histogram': (i, states + [D, i64, D, D, i, D, D, i, D, i, D, D, D])}),
        'nm_reweight_boot.h': ('nm_reweight_last_error', {
            'nm_reweight_boot_solve': (i, states + [i64, D, D, D, i, U16, d, i, D, I, D, I]),
            'nm_reweight_boot_expect': (i, states + [D, i64, D, D, i, U16, D, i, D, D, i, D, D, D, D, D, D])}),
        'nm_pca.h': ('nm_pca_last_error', {
            'nm_pca_moments': (i, [i, i64, i, F, D, D, D, D]),
            'nm_pca_project': (i, [i, i64, i, F, D, D, i, D, D, D]),
            'nm_pca_last_timing': (i, [D]),
            'nm_pca_last_error': (s, [])}),
        'nm_cluster.h': ('nm_cluster_last_error', {
            'nm_cluster_dbscan': (i, [i, i64, i, D, d, i, I32, I32, I32]),
            'nm_cluster_last_timing': (i, [D]),
            'nm_cluster_last_error': (s, [])}),
        'nm_tsne.h': ('nm_tsne_last_error', {
            'nm_tsne_affinities': (i, [i, i64, i, D, d, i, I32, D, D]),
            'nm_tsne_gradient': (i, [i, i64, i, I32, D, i, D, d, D, D, D]),
            'nm_tsne_descend': (i, [i, i64, i, I32, D, i, D, D, D, i, d, d, d, D]),
            'nm_tsne_last_timing': (i, [D]),
            'nm_tsne_last_error': (s, [])}),
        'nm_vae.h': ('nm_vae_last_error', {
            'nm_vae_nparams': (i64, [i, i]),
            'nm_vae_layout': (i, [i, i, I64]),
            'nm_vae_conv': (i, [i] * 8 + [F] * 4),
            'nm_vae_conv_grad': (i, [i] * 8 + [F] * 7),
            'nm_vae_dense': (i, [i] * 5 + [F] * 4),
            'nm_vae_dense_grad': (i, [i] * 5 + [F] * 7),
            'nm_vae_create': (i, [i, i, i, hp]),
            'nm_vae_destroy': (i, [h]),
            'nm_vae_set_params': (i, [h, F]),
            'nm_vae_get_params': (i, [h, F]),
            'nm_vae_data': (i, [h, i64, F]),
            'nm_vae_eval': (i, [h, i64, I64, F, F, F, F, F, F]),
            'nm_vae_grad': (i, [h, i64, I64, F, F, D]),
            'nm_vae_epoch': (i, [h, i64, I64, F, i, d, D]),
            'nm_vae_last_timing': (i, [D]),
            'nm_vae_last_error': (s, [])})}


PROTOTYPES = _prototypes()
# every symbol each header declares (tests check that the library exports all of them)
(SYMBOLS, DISTR_SYMBOLS, PARSE_SYMBOLS, REWEIGHT_SYMBOLS, REWEIGHT_HIST_SYMBOLS, REWEIGHT_BOOT_SYMBOLS, PCA_SYMBOLS, CLUSTER_SYMBOLS,
 TSNE_SYMBOLS, VAE_SYMBOLS) = (tuple(symbols) for _, symbols in PROTOTYPES.values())
_ERROR_OF = {name: error for error, symbols in PROTOTYPES.values() if error for name in symbols}

_lib = None


def load():
    """load libnm_hip.so and declare the prototypes of include/*.h"""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise ImportError('%s is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                          '(hipcc --offload-arch=gfx950); this package has no CPU fallback' % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    for _, symbols in PROTOTYPES.values():
        for name, (restype, argtypes) in symbols.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def call(name, *args, form='{} failed ({}): {}'):
    """the value of a stage's library function; negative: RuntimeError of form.format(name, value, the header's last error)"""
    L = load()
    rc = getattr(L, name)(*args)
    if rc < 0:
        raise RuntimeError(form.format(name, rc, getattr(L, _ERROR_OF[name])().decode()))
    return rc
