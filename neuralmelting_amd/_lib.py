"""ctypes binding of libnm_hip.so (include/nm.h).  There is no CPU fallback: if the HIP library is
missing or cannot be loaded this module raises, it never substitutes another implementation."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('NM_HIP_LIB') or os.path.join(_HERE, 'libnm_hip.so')  # NM_HIP_LIB: dev override (diagnostic builds)

c_double_p = C.POINTER(C.c_double)
c_float_p = C.POINTER(C.c_float)
c_int_p = C.POINTER(C.c_int)
c_uint64_p = C.POINTER(C.c_uint64)
c_int32_p = C.POINTER(C.c_int32)
c_int64_p = C.POINTER(C.c_int64)

NM_OK, NM_ERR_ARG, NM_ERR_HIP, NM_ERR_STATE, NM_ERR_UNSUPPORTED = 0, -1, -2, -3, -4
NM_EL_LJ, NM_EL_AL, NM_EL_NI, NM_EL_CU = 0, 1, 2, 3
NM_THERMO_COLS, NM_TRACE_COLS, NM_STATS_COLS = 17, 4, 12

# every symbol include/nm.h declares (tests check that the library exports all of them)
SYMBOLS = ('nm_create', 'nm_destroy', 'nm_last_error', 'nm_create_note', 'nm_nslots', 'nm_natoms', 'nm_cus_per_replica', 'nm_heal_count', 'nm_get_const',
           'nm_get_slots', 'nm_set_slots', 'nm_snapshot', 'nm_snapshot_fetch', 'nm_run_cycles_recorded', 'nm_record_capacity', 'nm_snapshot_pending',
           'nm_set_state', 'nm_get_state', 'nm_init_lattice', 'nm_lattice_state', 'nm_set_thermo', 'nm_set_step', 'nm_run_md', 'nm_run_block', 'nm_run_cycles', 'nm_get_thermo', 'nm_adapt',
           'nm_exchange', 'nm_synchronize', 'nm_get_status', 'nm_format_thrm', 'nm_format_traj', 'nm_append_outputs', 'nm_timing_reset', 'nm_timing_get', 'nm_stats_get', 'nm_eval',
           'nm_set_rng_tape', 'nm_set_exchange_tape', 'nm_set_trace', 'nm_get_trace', 'nm_get_perm', 'nm_set_counters',
           'nm_get_exchange_crit')


# include/nm_distr.h
DISTR_SYMBOLS = ('nm_distr_histograms', 'nm_distr_angles', 'nm_distr_sfactor', 'nm_distr_bondorder', 'nm_distr_solid', 'nm_distr_cna',
                 'nm_distr_entropy', 'nm_distr_last_error')
# include/nm_parse.h
PARSE_SYMBOLS = ('nm_parse_thrm', 'nm_parse_traj', 'nm_parse_last_error')
# include/nm_reweight.h
REWEIGHT_SYMBOLS = ('nm_reweight_solve', 'nm_reweight_expect', 'nm_reweight_last_error')
# include/nm_reweight_hist.h, which nm_reweight.h includes
REWEIGHT_HIST_SYMBOLS = ('nm_reweight_histogram',)
# include/nm_reweight_boot.h
REWEIGHT_BOOT_SYMBOLS = ('nm_reweight_boot_solve', 'nm_reweight_boot_expect')
# include/nm_pca.h
PCA_SYMBOLS = ('nm_pca_moments', 'nm_pca_project', 'nm_pca_last_timing', 'nm_pca_last_error')
# include/nm_cluster.h
CLUSTER_SYMBOLS = ('nm_cluster_dbscan', 'nm_cluster_last_timing', 'nm_cluster_last_error')
# include/nm_tsne.h
TSNE_SYMBOLS = ('nm_tsne_affinities', 'nm_tsne_gradient', 'nm_tsne_descend', 'nm_tsne_last_timing', 'nm_tsne_last_error')
# include/nm_vae.h
VAE_SYMBOLS = ('nm_vae_nparams', 'nm_vae_layout', 'nm_vae_conv', 'nm_vae_conv_grad', 'nm_vae_dense', 'nm_vae_dense_grad', 'nm_vae_create',
               'nm_vae_destroy', 'nm_vae_set_params', 'nm_vae_get_params', 'nm_vae_data', 'nm_vae_eval', 'nm_vae_grad', 'nm_vae_epoch',
               'nm_vae_last_timing', 'nm_vae_last_error')
NM_VAE_ACT_NONE, NM_VAE_ACT_RELU, NM_VAE_ACT_TANH, NM_VAE_NTENSORS = 0, 1, 2, 26


class NMConfig(C.Structure):
    _fields_ = [('size', C.c_int32), ('element', C.c_int32), ('natoms', C.c_int32), ('np', C.c_int32),
                ('nt', C.c_int32), ('row0', C.c_int32), ('nrows', C.c_int32), ('nstps', C.c_int32),
                ('bulk', C.c_int32), ('iter_revert', C.c_int32), ('device', C.c_int32), ('seed', C.c_uint32),
                ('ppos', C.c_double), ('pvol', C.c_double), ('P', c_float_p), ('T', c_float_p),
                ('slot0', C.c_int32), ('nslots', C.c_int32)]


_lib = None


def load():
    """load libnm_hip.so and declare the prototypes of include/nm.h"""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.isfile(LIB_PATH):
        raise ImportError('%s is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
                          '(hipcc --offload-arch=gfx950); this package has no CPU fallback' % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    L.nm_create.argtypes = [C.POINTER(NMConfig), C.POINTER(vp)]
    L.nm_destroy.argtypes = [vp]
    L.nm_last_error.restype = C.c_char_p
    L.nm_last_error.argtypes = [vp]
    L.nm_create_note.restype = C.c_char_p
    L.nm_create_note.argtypes = [vp]
    L.nm_nslots.argtypes = [vp]
    L.nm_natoms.argtypes = [vp]
    L.nm_cus_per_replica.argtypes = [vp]
    L.nm_heal_count.argtypes = [vp]
    L.nm_get_const.argtypes = [vp, c_double_p, c_double_p]
    L.nm_set_state.argtypes = [vp, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p]
    L.nm_get_state.argtypes = [vp, C.c_int, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p]
    L.nm_set_thermo.argtypes = [vp, C.c_int, C.c_int, c_double_p]
    L.nm_get_slots.argtypes = [vp, C.c_int, c_int_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]
    L.nm_set_slots.argtypes = [vp, C.c_int, c_int_p, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]
    L.nm_init_lattice.argtypes = [vp, C.c_double, C.c_double, C.c_int]
    L.nm_lattice_state.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, c_float_p, C.c_uint32, C.c_int, C.c_double, C.c_int, c_double_p, c_double_p]
    L.nm_set_step.argtypes = [vp, C.c_uint32]
    L.nm_run_block.argtypes = [vp, C.c_int]
    L.nm_run_cycles.argtypes = [vp, C.c_int, C.c_int]
    L.nm_run_md.argtypes = [vp, C.c_int]
    L.nm_get_thermo.argtypes = [vp, c_double_p]
    L.nm_adapt.argtypes = [vp]
    L.nm_snapshot.argtypes = [vp]
    L.nm_snapshot_fetch.argtypes = [vp, c_double_p, c_double_p, c_double_p]
    L.nm_run_cycles_recorded.argtypes = [vp, C.c_int, C.c_int]
    L.nm_record_capacity.argtypes = [vp]
    L.nm_snapshot_pending.argtypes = [vp]
    L.nm_exchange.argtypes = [vp, c_int_p]
    L.nm_synchronize.argtypes = [vp]
    L.nm_get_status.argtypes = [vp, c_int_p]
    L.nm_format_thrm.argtypes = [c_double_p, C.c_char_p, C.c_int]
    L.nm_format_traj.argtypes = [C.c_int, C.c_double, c_double_p, C.c_char_p, C.c_int]
    L.nm_append_outputs.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), c_double_p, c_double_p, c_double_p,
                                    C.c_int]
    L.nm_timing_reset.argtypes = [vp]
    L.nm_timing_get.argtypes = [vp, c_int_p, c_double_p]
    L.nm_stats_get.argtypes = [vp, c_double_p, C.c_int]
    L.nm_eval.argtypes = [vp, c_double_p, c_double_p, c_double_p]
    L.nm_set_rng_tape.argtypes = [vp, c_double_p, c_int_p]
    L.nm_set_exchange_tape.argtypes = [vp, c_double_p, C.c_int]
    L.nm_set_trace.argtypes = [vp, C.c_int]
    L.nm_get_trace.argtypes = [vp, c_double_p, C.c_int]
    L.nm_get_perm.argtypes = [vp, c_int_p]
    L.nm_set_counters.argtypes = [vp, c_double_p, c_float_p]
    L.nm_get_exchange_crit.argtypes = [vp, c_double_p, C.c_int]
    for s in SYMBOLS:
        if s not in ('nm_last_error', 'nm_create_note'):
            getattr(L, s).restype = C.c_int
    L.nm_distr_histograms.restype = C.c_int
    L.nm_distr_histograms.argtypes = [C.c_int, C.c_int, C.c_int, c_float_p, c_float_p, C.c_int, c_double_p, C.c_int, c_double_p,
                                      c_float_p, c_float_p]
    L.nm_distr_angles.restype = C.c_int
    L.nm_distr_angles.argtypes = [C.c_int, C.c_int, C.c_int, c_float_p, c_float_p, C.c_double, C.c_double, C.c_int, c_double_p,
                                  c_uint64_p]
    L.nm_distr_sfactor.restype = C.c_int
    L.nm_distr_sfactor.argtypes = [C.c_int, C.c_int, C.c_int, c_float_p, c_float_p, C.c_int, c_double_p, c_double_p]
    L.nm_distr_bondorder.restype = C.c_int
    L.nm_distr_bondorder.argtypes = [C.c_int, C.c_int, C.c_int, c_float_p, c_float_p, C.c_double, C.c_double, C.c_int, c_int_p,
                                     c_double_p, c_double_p, c_double_p, c_int32_p]
    L.nm_distr_solid.restype = C.c_int
    L.nm_distr_solid.argtypes = [C.c_int, C.c_int, C.c_int, c_float_p, c_float_p, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int,
                                 c_int32_p, c_int32_p, c_int32_p, c_int32_p, c_int32_p]
    L.nm_distr_cna.restype = C.c_int
    L.nm_distr_cna.argtypes = [C.c_int, C.c_int, C.c_int, c_float_p, c_float_p, C.c_double, C.c_double, C.c_int, c_int32_p, c_int32_p,
                               c_int32_p, c_int32_p]
    L.nm_distr_entropy.restype = C.c_int
    L.nm_distr_entropy.argtypes = [C.c_int, C.c_int, C.c_int, c_float_p, c_float_p, C.c_double, C.c_double, C.c_int, C.c_double, C.c_double,
                                   c_double_p, c_double_p, c_int32_p, c_double_p, c_double_p, c_int32_p]
    L.nm_distr_last_error.restype = C.c_char_p
    c_long_p = C.POINTER(C.c_long)
    L.nm_parse_thrm.restype = C.c_int
    L.nm_parse_thrm.argtypes = [C.c_char_p, c_float_p, C.c_long, c_long_p, C.c_int]
    L.nm_parse_traj.restype = C.c_int
    L.nm_parse_traj.argtypes = [C.c_char_p, C.POINTER(C.c_uint16), c_float_p, c_float_p, C.c_long, C.c_long, c_long_p, c_long_p,
                                C.c_int]
    L.nm_parse_last_error.restype = C.c_char_p
    L.nm_reweight_solve.restype = C.c_int
    L.nm_reweight_solve.argtypes = [C.c_int, C.c_int, c_double_p, c_double_p, c_int64_p, C.c_int64, c_double_p, c_double_p, C.c_double,
                                    C.c_int, c_double_p, c_double_p, c_int_p, c_double_p]
    L.nm_reweight_expect.restype = C.c_int
    L.nm_reweight_expect.argtypes = [C.c_int, C.c_int, c_double_p, c_double_p, c_int64_p, c_double_p, C.c_int64, c_double_p, c_double_p,
                                     C.c_int, c_double_p, c_double_p, C.c_int, c_double_p, c_double_p, c_double_p, c_double_p, c_double_p,
                                     c_double_p]
    L.nm_reweight_histogram.restype = C.c_int
    L.nm_reweight_histogram.argtypes = [C.c_int, C.c_int, c_double_p, c_double_p, c_int64_p, c_double_p, C.c_int64, c_double_p, c_double_p,
                                        C.c_int, c_double_p, c_double_p, C.c_int, c_double_p, C.c_int, c_double_p, c_double_p, c_double_p]
    L.nm_reweight_boot_solve.restype = C.c_int
    L.nm_reweight_boot_solve.argtypes = [C.c_int, C.c_int, c_double_p, c_double_p, c_int64_p, C.c_int64, c_double_p, c_double_p, c_double_p,
                                         C.c_int, C.POINTER(C.c_uint16), C.c_double, C.c_int, c_double_p, c_int_p, c_double_p, c_int_p]
    L.nm_reweight_boot_expect.restype = C.c_int
    L.nm_reweight_boot_expect.argtypes = [C.c_int, C.c_int, c_double_p, c_double_p, c_int64_p, c_double_p, C.c_int64, c_double_p, c_double_p,
                                          C.c_int, C.POINTER(C.c_uint16), c_double_p, C.c_int, c_double_p, c_double_p, C.c_int, c_double_p,
                                          c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]
    L.nm_reweight_last_error.restype = C.c_char_p
    L.nm_pca_moments.restype = C.c_int
    L.nm_pca_moments.argtypes = [C.c_int, C.c_int64, C.c_int, c_float_p, c_double_p, c_double_p, c_double_p, c_double_p]
    L.nm_pca_project.restype = C.c_int
    L.nm_pca_project.argtypes = [C.c_int, C.c_int64, C.c_int, c_float_p, c_double_p, c_double_p, C.c_int, c_double_p, c_double_p, c_double_p]
    L.nm_pca_last_timing.restype = C.c_int
    L.nm_pca_last_timing.argtypes = [c_double_p]
    L.nm_pca_last_error.restype = C.c_char_p
    L.nm_cluster_dbscan.restype = C.c_int
    L.nm_cluster_dbscan.argtypes = [C.c_int, C.c_int64, C.c_int, c_double_p, C.c_double, C.c_int, c_int32_p, c_int32_p, c_int32_p]
    L.nm_cluster_last_timing.restype = C.c_int
    L.nm_cluster_last_timing.argtypes = [c_double_p]
    L.nm_cluster_last_error.restype = C.c_char_p
    L.nm_tsne_affinities.restype = C.c_int
    L.nm_tsne_affinities.argtypes = [C.c_int, C.c_int64, C.c_int, c_double_p, C.c_double, C.c_int, c_int32_p, c_double_p, c_double_p]
    L.nm_tsne_gradient.restype = C.c_int
    L.nm_tsne_gradient.argtypes = [C.c_int, C.c_int64, C.c_int, c_int32_p, c_double_p, C.c_int, c_double_p, C.c_double, c_double_p,
                                   c_double_p, c_double_p]
    L.nm_tsne_descend.restype = C.c_int
    L.nm_tsne_descend.argtypes = [C.c_int, C.c_int64, C.c_int, c_int32_p, c_double_p, C.c_int, c_double_p, c_double_p, c_double_p, C.c_int,
                                  C.c_double, C.c_double, C.c_double, c_double_p]
    L.nm_tsne_last_timing.restype = C.c_int
    L.nm_tsne_last_timing.argtypes = [c_double_p]
    L.nm_tsne_last_error.restype = C.c_char_p
    i, f = C.c_int, c_float_p
    L.nm_vae_nparams.restype = C.c_int64
    L.nm_vae_nparams.argtypes = [i, i]
    L.nm_vae_layout.argtypes = [i, i, c_int64_p]
    L.nm_vae_conv.argtypes = [i, i, i, i, i, i, i, i, f, f, f, f]
    L.nm_vae_conv_grad.argtypes = [i, i, i, i, i, i, i, i, f, f, f, f, f, f, f]
    L.nm_vae_dense.argtypes = [i, i, i, i, i, f, f, f, f]
    L.nm_vae_dense_grad.argtypes = [i, i, i, i, i, f, f, f, f, f, f, f]
    L.nm_vae_create.argtypes = [i, i, i, C.POINTER(vp)]
    L.nm_vae_destroy.argtypes = [vp]
    L.nm_vae_set_params.argtypes = [vp, f]
    L.nm_vae_get_params.argtypes = [vp, f]
    L.nm_vae_data.argtypes = [vp, C.c_int64, f]
    L.nm_vae_eval.argtypes = [vp, C.c_int64, c_int64_p, f, f, f, f, f, f]
    L.nm_vae_grad.argtypes = [vp, C.c_int64, c_int64_p, f, f, c_double_p]
    L.nm_vae_epoch.argtypes = [vp, C.c_int64, c_int64_p, f, i, C.c_double, c_double_p]
    L.nm_vae_last_timing.argtypes = [c_double_p]
    for s in VAE_SYMBOLS:
        if s not in ('nm_vae_nparams', 'nm_vae_last_error'):
            getattr(L, s).restype = C.c_int
    L.nm_vae_last_error.restype = C.c_char_p
    _lib = L
    return L
