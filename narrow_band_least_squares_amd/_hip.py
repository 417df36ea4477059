"""ctypes binding of ``libnbls_hip.so`` (C ABI: ``include/nbls.h``).

There is no CPU fallback: if the library is missing or no HIP device can be opened, the
functions of this package raise.  No PyTorch is involved on this path.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# NBLS_LIB: another build of the library (tools/ use the developer build, csrc/libnbls_hip_dev.so)
LIB_PATH = os.environ.get('NBLS_LIB') or os.path.join(_HERE, 'csrc', 'libnbls_hip.so')

EXPORTS = [
    'nbls_version', 'nbls_device_count', 'nbls_create', 'nbls_destroy', 'nbls_last_error', 'nbls_set_trace',
    'nbls_set_geometry', 'nbls_plan', 'nbls_execute', 'nbls_execute_stages', 'nbls_execute_after', 'nbls_set_trace_shape', 'nbls_upload_rows', 'nbls_sync',
    'nbls_fetch', 'nbls_fetch_filtered', 'nbls_device_results', 'nbls_set_profiling',
    'nbls_get_timings', 'nbls_run', 'nbls_probe_mfma_f64', 'nbls_probe_mfma_i8', 'nbls_debug_screen_stats', 'nbls_debug_screen_records', 'nbls_set_window_ranges', 'nbls_debug_screen_stamps', 'nbls_debug_lts_stamps',
    'nbls_set_trace_rows', 'nbls_result_layout', 'nbls_fetch_packed', 'nbls_comm_init_all', 'nbls_comm_unique_id',
    'nbls_comm_init_rank', 'nbls_reserve_results', 'nbls_comm_gather', 'nbls_comm_destroy', 'nbls_set_option',
    'nbls_developer_build', 'nbls_set_trace_from', 'nbls_debug_lts_coop_breakdown', 'nbls_filter_segment',
    'nbls_set_filtered', 'nbls_load_result_block', 'nbls_stream_results', 'nbls_result_batches', 'nbls_wait_result_batch',
    'nbls_comm_set_library', 'nbls_set_uncertainty', 'nbls_fetch_uncertainty', 'nbls_expect_upload', 'nbls_abort_upload',
    'nbls_set_segments', 'nbls_route_xcorr', 'nbls_route_table', 'nbls_set_estimators', 'nbls_est_result_layout',
    'nbls_est_fetch_packed', 'nbls_est_fetch', 'nbls_est_fetch_uncertainty', 'nbls_est_wait_result_batch',
    'nbls_set_beam', 'nbls_fetch_beam', 'nbls_est_fetch_beam',
    'nbls_set_lag_refinement', 'nbls_fetch_lag_fraction', 'nbls_est_fetch_lag_fraction', 'nbls_refine_lds_bytes',
    'nbls_set_lag_limits', 'nbls_lag_limit_form', 'nbls_set_lag_seed', 'nbls_lag_seed_form',
    'nbls_set_beam_grid', 'nbls_fetch_beam_grid', 'nbls_fetch_beam_grid_map', 'nbls_fetch_beam_grid_delays',
    'nbls_beam_grid_lds_bytes',
    'nbls_set_closure', 'nbls_fetch_closure', 'nbls_est_fetch_closure',
    'nbls_set_capon', 'nbls_fetch_capon', 'nbls_fetch_capon_maps', 'nbls_fetch_capon_csdm', 'nbls_fetch_capon_tables',
    'nbls_set_capon_peaks', 'nbls_fetch_capon_peaks',
    'nbls_set_capon_clean', 'nbls_fetch_capon_clean', 'nbls_fetch_capon_clean_csdm', 'nbls_capon_clean_lds_bytes',
    'nbls_set_capon_music', 'nbls_fetch_capon_music', 'nbls_fetch_capon_music_map', 'nbls_fetch_capon_music_vectors',
    'nbls_fetch_capon_music_peaks',
    'nbls_capon_music_lds_bytes',
    'nbls_set_kept_elements', 'nbls_fetch_kept_elements',
    'nbls_set_beam_trace', 'nbls_fetch_beam_trace',
    'nbls_set_beam_interpolation', 'nbls_fetch_beam_grid_coefficients',
    'nbls_set_element_delays', 'nbls_fetch_element_delays', 'nbls_element_delay_lds_bytes',
    'nbls_set_families', 'nbls_fetch_families', 'nbls_label_families',
    'nbls_set_beam_grid_refinement', 'nbls_fetch_beam_grid_refined', 'nbls_beam_grid_refine_lds_bytes',
]
STEER_TAPS = (0, 4, 6, 8)  # taps of nbls_set_beam_interpolation (0: whole-sample delays)
GRID_REFINE_MAX_LEVELS = 12   # levels of nbls_set_beam_grid_refinement (NBLS_BEAM_GRID_REFINE_MAX_LEVELS)
BEAM_GRID_MAX = 65536    # grid points of a slowness-grid search (NBLS_BEAM_GRID_MAX)
BEAM_GRID_WAVES = 16     # waves of a workgroup of the search kernel (NBLS_BEAM_GRID_WAVES)
CAPON_GRID_MAX = 65536   # grid points of the Capon spectra (NBLS_CAPON_GRID_MAX)
CAPON_MAX_ELEMENTS = 32  # array elements of a plan with Capon spectra (NBLS_CAPON_MAX_ELEMENTS)
CAPON_THREADS = 128      # threads of a workgroup of the Capon kernel, one grid point each (NBLS_CAPON_THREADS)
CAPON_CHUNK = 32         # snapshots that go through LDS together (NBLS_CAPON_CHUNK)
CAPON_MAPS, CAPON_CSDM = 1, 2     # flags of nbls_set_capon
CAPON_PEAKS_MAX = 8      # ranks of a peak request (NBLS_CAPON_PEAKS_MAX)
CAPON_CLEAN_MAX = 32     # iterations of a CLEAN request (NBLS_CAPON_CLEAN_MAX)
CLEAN_RESIDUAL = 1       # flag of nbls_set_capon_clean (NBLS_CLEAN_RESIDUAL)
MUSIC_MAP, MUSIC_VECTORS, MUSIC_PEAKS = 1, 2, 4   # flags of nbls_set_capon_music
MUSIC_SWEEP_CAP = 24     # Jacobi sweeps of a MUSIC request at most (NBLS_MUSIC_SWEEP_CAP)
KEPT_BEAM, KEPT_CAPON = 1, 2      # flags of nbls_set_kept_elements
BEAM_TRACE_KEPT = 1      # flag of nbls_set_beam_trace
ELEMENT_DELAY_KEPT = 1   # flag of nbls_set_element_delays (NBLS_ELEMENT_DELAY_KEPT)
ELEMENT_DELAY_MAX_SHIFT = 256     # largest max_shift of a band (NBLS_ELEMENT_DELAY_MAX_SHIFT)
FAMILY_COLUMNS = 8       # columns of a family table row (NBLS_FAMILY_COLUMNS)
FAMILY_MAX_REACH = 8     # largest band_reach / time_reach of a family request (NBLS_FAMILY_MAX_REACH)
# the columns of a family table row, in order
FAMILY_FIELDS = ('count', 'first_cell', 'peak_cell', 'band_lo', 'band_hi', 'segment', 'sample_first', 'sample_end')
MAX_ESTIMATORS = 8       # further estimators of one pass beside estimator 0 (NBLS_MAX_ESTIMATORS)

NBLS_ERR_ARG, NBLS_ERR_STATE, NBLS_ERR_GEOMETRY = -1, -2, -3
NBLS_ERR_HIP, NBLS_ERR_NOMEM, NBLS_ERR_UNSUPPORTED, NBLS_ERR_COMM = -4, -5, -6, -7


class NblsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('libnbls_hip error %d: %s' % (code, msg))
        self.code = code


class LtsParams(C.Structure):
    _fields_ = [
        ('alpha', C.c_double), ('h', C.c_int32), ('nstarts', C.c_int32),
        ('starts', C.POINTER(C.c_int32)), ('csteps', C.c_int32), ('csteps2', C.c_int32),
        ('ncand', C.c_int32), ('xij_mad', C.c_double * 2), ('raw_factor', C.c_double),
        ('rew_table', C.POINTER(C.c_double)), ('quantile', C.c_double), ('zero_scale', C.c_double),
    ]


class EstimatorDesc(C.Structure):
    _fields_ = [('lts', C.POINTER(LtsParams)), ('nkept', C.c_int32), ('kept', C.POINTER(C.c_int32)),
                ('xij', C.POINTER(C.c_double)), ('pair_idx', C.POINTER(C.c_int32)), ('xpinv', C.POINTER(C.c_double)),
                ('eig6', C.POINTER(C.c_double))]


class FamilyParams(C.Structure):
    _fields_ = [('mdccm_min', C.c_double), ('vel_min', C.c_double), ('vel_max', C.c_double), ('sigma_tau_max', C.c_double),
                ('baz_tol', C.c_double), ('vel_tol', C.c_double), ('band_reach', C.c_int32), ('time_reach', C.c_int32),
                ('min_pixels', C.c_int32), ('flags', C.c_int32)]


def family_params(mdccm_min, vel_min, vel_max, sigma_tau_max, baz_tol, vel_tol, band_reach, time_reach, min_pixels):
    """The request of ``nbls_set_families`` / ``nbls_label_families`` (``sigma_tau_max`` None: that gate is off)."""
    return FamilyParams(float(mdccm_min), float(vel_min), float(vel_max), float('nan') if sigma_tau_max is None else float(sigma_tau_max),
                        float(baz_tol), float(vel_tol), int(band_reach), int(time_reach), int(min_pixels), 0)


class Timings(C.Structure):
    _fields_ = [('filter_ms', C.c_double), ('xcorr_ms', C.c_double), ('solve_ms', C.c_double),
                ('total_ms', C.c_double), ('xcorr_launches', C.c_int64), ('quantize_ms', C.c_double),
                ('screen_ms', C.c_double), ('verify_ms', C.c_double), ('xcorr_impl', C.c_int32),
                ('xcorr_fallback_bands', C.c_int32)]


# nbls_route (include/nbls.h): the correlator route of one window group
ROUTE_REJECTED, ROUTE_SCREEN, ROUTE_MFMA, ROUTE_VALU_LDS, ROUTE_VALU_GLOBAL = 0, 1, 2, 3, 4
ROUTE_QUANTIZE, ROUTE_SCREEN_STAGE, ROUTE_VERIFY, ROUTE_GENERAL = 0, 1, 2, 3
ROUTE_OPT_NC4, ROUTE_OPT_NSL1, ROUTE_OPT_TB8, ROUTE_OPT_TB4 = 1, 2, 4, 8
ROUTE_DTYPE = np.dtype([(k, np.int32) for k in ('correlator', 'impl', 'ncopy', 'G', 'S', 'nsl', 'PFB', 'CSB', 'CSA', 'WP',
                                                 'screen_inst', 'tab_lds', 'quant_inst', 'quant_waves', 'verifier',
                                                 'verify_threads')] +
                       [('lds_dyn', np.int64, (4,)), ('lds_static', np.int64, (4,))])
# the fields that name the kernels a route launches and their tiling (the LDS sizes follow from them)
ROUTE_KEYS = ('correlator', 'ncopy', 'G', 'S', 'nsl', 'screen_inst', 'tab_lds', 'quant_inst', 'quant_waves', 'verifier',
              'verify_threads')


class Route(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ROUTE_DTYPE.names[:16]] + [('lds_dyn', C.c_int64 * 4), ('lds_static', C.c_int64 * 4)]


_lib = None


def load_library(path=None):
    """Load (once) and return the ctypes library; raises ImportError if it is not built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise ImportError('%s not found: build it with `make -C %s` (or __graft_entry__.build()); '
                          'this package has no CPU fallback' % (p, os.path.dirname(p)))
    lib = C.CDLL(p)
    dp = C.POINTER(C.c_double)
    ip = C.POINTER(C.c_int32)
    u8p = C.POINTER(C.c_uint8)
    vp = C.c_void_p
    lib.nbls_version.restype = C.c_int
    lib.nbls_create.argtypes = [C.c_int, C.POINTER(vp)]
    lib.nbls_destroy.argtypes = [vp]
    lib.nbls_destroy.restype = None
    lib.nbls_last_error.argtypes = [vp]
    lib.nbls_last_error.restype = C.c_char_p
    lib.nbls_set_trace.argtypes = [vp, dp, C.c_int32, C.c_int64, C.c_double]
    lib.nbls_set_trace_rows.argtypes = [vp, C.POINTER(C.c_void_p), C.c_int32, C.c_int64, C.c_double]
    lib.nbls_result_layout.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.nbls_fetch_packed.argtypes = [vp, C.c_void_p, C.c_int64]
    lib.nbls_comm_init_all.argtypes = [C.POINTER(vp), C.c_int32]
    lib.nbls_comm_unique_id.argtypes = [C.c_void_p, C.c_int32]
    lib.nbls_comm_init_rank.argtypes = [vp, C.c_void_p, C.c_int32, C.c_int32]
    lib.nbls_reserve_results.argtypes = [vp, C.c_int64]
    lib.nbls_load_result_block.argtypes = [vp, C.c_void_p, C.c_int64]
    lib.nbls_comm_gather.argtypes = [C.POINTER(vp), C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_void_p, C.c_int64]
    lib.nbls_comm_destroy.argtypes = [vp]
    lib.nbls_expect_upload.argtypes = [vp]
    lib.nbls_abort_upload.argtypes = [vp]
    lib.nbls_comm_set_library.argtypes = [C.c_char_p, C.c_int32]
    lib.nbls_set_uncertainty.argtypes = [vp, dp]
    lib.nbls_fetch_uncertainty.argtypes = [vp, dp, dp]
    lib.nbls_stream_results.argtypes = [vp, C.c_int32]
    lib.nbls_result_batches.argtypes = [vp, C.POINTER(C.c_int32)]
    lib.nbls_wait_result_batch.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_void_p)]
    lib.nbls_set_trace_from.argtypes = [vp, vp]
    lib.nbls_filter_segment.argtypes = [vp, C.c_int32, dp, dp]
    lib.nbls_set_filtered.argtypes = [vp, C.c_int32, dp]
    lib.nbls_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    lib.nbls_set_geometry.argtypes = [vp, dp, ip, dp, C.c_int32]
    plan_args = [vp, C.c_int32, dp, C.c_int32, C.c_int32, dp, dp, C.c_int32, ip, ip, C.c_int32,
                 C.POINTER(LtsParams), C.c_int32]
    lib.nbls_plan.argtypes = plan_args
    lib.nbls_execute.argtypes = [vp]
    lib.nbls_execute_stages.argtypes = [vp, C.c_int32]
    lib.nbls_execute_after.argtypes = [vp, vp]
    lib.nbls_set_trace_shape.argtypes = [vp, C.c_int32, C.c_int64, C.c_double]
    lib.nbls_upload_rows.argtypes = [vp, C.POINTER(C.c_void_p), C.c_int32, C.c_int64]
    lib.nbls_sync.argtypes = [vp]
    fetch_args = [dp, dp, dp, dp, ip, ip, dp, u8p, dp]
    lib.nbls_fetch.argtypes = [vp] + fetch_args
    lib.nbls_set_estimators.argtypes = [vp, C.c_int32, C.POINTER(EstimatorDesc)]
    lib.nbls_est_result_layout.argtypes = [vp, C.c_int32, C.POINTER(C.c_int64)]
    lib.nbls_est_fetch_packed.argtypes = [vp, C.c_int32, C.c_void_p, C.c_int64]
    lib.nbls_est_fetch.argtypes = [vp, C.c_int32] + fetch_args
    lib.nbls_est_fetch_uncertainty.argtypes = [vp, C.c_int32, dp, dp]
    lib.nbls_est_wait_result_batch.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_void_p)]
    lib.nbls_set_beam.argtypes = [vp, C.c_int32]
    lib.nbls_fetch_beam.argtypes = [vp, dp, dp]
    lib.nbls_est_fetch_beam.argtypes = [vp, C.c_int32, dp, dp]
    lib.nbls_set_closure.argtypes = [vp, C.c_int32]
    lib.nbls_fetch_closure.argtypes = [vp, dp, dp, dp]
    lib.nbls_est_fetch_closure.argtypes = [vp, C.c_int32, dp, dp, dp]
    lib.nbls_set_lag_refinement.argtypes = [vp, C.c_int32]
    lib.nbls_fetch_lag_fraction.argtypes = [vp, dp]
    lib.nbls_refine_lds_bytes.argtypes = [C.c_int32, C.c_int32]
    lib.nbls_est_fetch_lag_fraction.argtypes = [vp, C.c_int32, dp]
    lib.nbls_set_lag_limits.argtypes = [vp, ip, C.c_int32]
    lib.nbls_lag_limit_form.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.nbls_set_lag_seed.argtypes = [vp, ip, C.c_int32]
    lib.nbls_lag_seed_form.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    lib.nbls_set_beam_grid.argtypes = [vp, dp, C.c_int32, C.c_int32]
    lib.nbls_fetch_beam_grid.argtypes = [vp, ip, dp, dp]
    lib.nbls_fetch_beam_grid_map.argtypes = [vp, dp]
    lib.nbls_fetch_beam_grid_delays.argtypes = [vp, ip]
    lib.nbls_beam_grid_lds_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.nbls_set_beam_interpolation.argtypes = [vp, C.c_int32]
    lib.nbls_set_beam_grid_refinement.argtypes = [vp, C.c_int32, dp]
    lib.nbls_fetch_beam_grid_refined.argtypes = [vp, dp, dp, dp, ip, dp]
    lib.nbls_beam_grid_refine_lds_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    lib.nbls_fetch_beam_grid_coefficients.argtypes = [vp, dp]
    lib.nbls_set_capon.argtypes = [vp, dp, C.c_int32, dp, ip, ip, C.c_int32, C.c_double, C.c_int32]
    lib.nbls_fetch_capon.argtypes = [vp, ip, dp, ip, dp]
    lib.nbls_fetch_capon_maps.argtypes = [vp, dp, dp]
    lib.nbls_fetch_capon_csdm.argtypes = [vp, dp]
    lib.nbls_fetch_capon_tables.argtypes = [vp, C.c_int32, dp, dp]
    lib.nbls_set_capon_peaks.argtypes = [vp, ip, C.c_int32, C.c_int32, C.c_double]
    lib.nbls_fetch_capon_peaks.argtypes = [vp, C.c_int32, ip, ip, dp, dp]
    lib.nbls_set_capon_clean.argtypes = [vp, C.c_int32, C.c_double, C.c_double, C.c_int32]
    lib.nbls_fetch_capon_clean.argtypes = [vp, ip, ip, dp, dp, dp]
    lib.nbls_fetch_capon_clean_csdm.argtypes = [vp, dp]
    lib.nbls_capon_clean_lds_bytes.argtypes = [C.c_int32]
    lib.nbls_set_capon_music.argtypes = [vp, C.c_int32, C.c_double, C.c_double, C.c_int32]
    lib.nbls_fetch_capon_music.argtypes = [vp, dp, ip, ip, ip, dp]
    lib.nbls_fetch_capon_music_map.argtypes = [vp, dp]
    lib.nbls_fetch_capon_music_vectors.argtypes = [vp, dp]
    lib.nbls_fetch_capon_music_peaks.argtypes = [vp, ip, ip, dp, dp]
    lib.nbls_capon_music_lds_bytes.argtypes = [C.c_int32]
    lib.nbls_set_kept_elements.argtypes = [vp, C.c_int32, C.c_int32]
    lib.nbls_fetch_kept_elements.argtypes = [vp, C.POINTER(C.c_uint32), ip]
    lib.nbls_set_beam_trace.argtypes = [vp, dp, C.c_int64, C.c_double, C.c_int32]
    lib.nbls_fetch_beam_trace.argtypes = [vp, C.c_int32, dp]
    lib.nbls_set_element_delays.argtypes = [vp, ip, C.c_int32, C.c_int32]
    lib.nbls_fetch_element_delays.argtypes = [vp, dp, dp, ip]
    lib.nbls_element_delay_lds_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32]
    i64p = C.POINTER(C.c_int64)
    lib.nbls_set_families.argtypes = [vp, C.POINTER(FamilyParams)]
    lib.nbls_fetch_families.argtypes = [vp, ip, ip, i64p, C.c_int64]
    lib.nbls_label_families.argtypes = [vp, C.POINTER(FamilyParams), C.c_int32, C.c_int32, C.c_int32, ip, ip, ip, dp, dp, dp, dp, ip, ip,
                                        i64p, C.c_int64]
    lib.nbls_fetch_filtered.argtypes = [vp, C.c_int32, dp]
    lib.nbls_device_results.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_int64)]
    lib.nbls_set_profiling.argtypes = [vp, C.c_int32]
    lib.nbls_get_timings.argtypes = [vp, C.POINTER(Timings)]
    lib.nbls_run.argtypes = plan_args + fetch_args
    lib.nbls_probe_mfma_f64.argtypes = [vp, dp, dp, dp]
    lib.nbls_probe_mfma_i8.argtypes = [vp, ip, ip, ip]
    lib.nbls_debug_screen_stats.argtypes = [vp, C.POINTER(C.c_int64)]
    lib.nbls_debug_screen_records.argtypes = [vp, ip, C.c_int64, C.POINTER(C.c_int64)]
    lib.nbls_set_window_ranges.argtypes = [vp, C.c_int32, ip, ip]
    lib.nbls_set_segments.argtypes = [vp, C.c_int32]
    lib.nbls_debug_screen_stamps.argtypes = [vp, dp]
    lib.nbls_debug_lts_stamps.argtypes = [vp, dp]
    lib.nbls_debug_lts_coop_breakdown.argtypes = [vp, dp]
    lib.nbls_route_xcorr.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                     C.POINTER(Route)]
    lib.nbls_route_table.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.c_int32,
                                     C.c_void_p]
    for name in EXPORTS:
        if name not in ('nbls_destroy', 'nbls_last_error'):
            getattr(lib, name).restype = C.c_int
    if path is None:
        _lib = lib
    return lib


def _lts_params(lts):
    """dict from planner.lts_plan() -> (LtsParams, the arrays it points into)."""
    starts = np.ascontiguousarray(lts['starts'], dtype=np.int32)
    rew = _f64(lts['rew_table'])
    p = LtsParams()
    p.alpha = float(lts['alpha'])
    p.h = int(lts['h'])
    p.nstarts = int(starts.shape[0])
    p.starts = _iptr(starts)
    p.csteps = int(lts['csteps'])
    p.csteps2 = int(lts['csteps2'])
    p.ncand = int(lts['ncand'])
    p.xij_mad[0] = float(lts['xij_mad'][0])
    p.xij_mad[1] = float(lts['xij_mad'][1])
    p.raw_factor = float(lts['raw_factor'])
    p.rew_table = _dptr(rew)
    p.quantile = float(lts['quantile'])
    p.zero_scale = float(lts['zero_scale'])
    return p, [starts, rew, p]


def estimator_descs(ests):
    """Dicts as ``Handle.set_estimators`` takes them -> (EstimatorDesc array, the arrays it points into, pair counts)."""
    descs = (EstimatorDesc * max(1, len(ests)))()
    keep, npairs = [], []
    for d, e in zip(descs, ests):
        kept = np.ascontiguousarray(e['kept'], dtype=np.int32)
        xij, xpinv = _f64(e['xij']), _f64(e['xpinv'])
        pair_idx = np.ascontiguousarray(e['pair_idx'], dtype=np.int32)
        nk = len(kept)
        if xij.shape != (nk * (nk - 1) // 2, 2) or xpinv.shape != (2, xij.shape[0]) or pair_idx.shape != xij.shape:
            raise ValueError('set_estimators: the tables do not have the pair count of the kept elements')
        d.nkept, d.kept, d.xij, d.pair_idx, d.xpinv = nk, _iptr(kept), _dptr(xij), _iptr(pair_idx), _dptr(xpinv)
        keep += [kept, xij, xpinv, pair_idx]
        if e.get('lts') is not None:
            p, held = _lts_params(e['lts'])
            d.lts = C.pointer(p)
            keep += held
        if e.get('eig6') is not None:
            eig = _f64(e['eig6'])
            d.eig6 = _dptr(eig)
            keep.append(eig)
        npairs.append(xij.shape[0])
    return descs, keep, npairs


def _dptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def _iptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _u8ptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint8))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


class Handle:
    """One GPU, one stream, one host thread at a time."""

    def __init__(self, device_id=0):
        self.lib = load_library()
        h = C.c_void_p()
        rc = self.lib.nbls_create(int(device_id), C.byref(h))
        if rc != 0:
            raise NblsError(rc, self.lib.nbls_last_error(None).decode())
        self._h = h
        self.device_id = int(device_id)
        self.nchans = self.npts = self.npairs = 0
        self.nbands = self.vector_len = 0
        self.nseg = 1
        self.est_npairs = []            # pair counts of the further estimators (set_estimators)
        self._want_grid_n = self.grid_n = 0   # grid points of set_beam_grid / of the plan
        self._want_taps = self.taps = 0       # taps of set_beam_interpolation / of the plan
        self._want_refine_levels = self.refine_levels = 0     # levels of set_beam_grid_refinement / of the plan
        self._want_capon = self.capon = None  # (G, snapshot lengths) of set_capon / of the plan
        self._want_capon_peaks = self.capon_peaks = 0     # K of set_capon_peaks / of the plan
        self._want_capon_clean = self.capon_clean = 0     # I of set_capon_clean / of the plan
        self._want_capon_music = self.capon_music = None  # (sources, maps, vectors) of set_capon_music / of the plan
        self._keep = []
        self.profiling = False
        self.resident_key = None        # engine.resident_trace: what the trace in HBM was uploaded from (any new trace clears it)

    def close(self):
        if getattr(self, '_h', None):
            self.lib.nbls_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            msg = self.lib.nbls_last_error(self._h).decode()
            if rc == NBLS_ERR_GEOMETRY:
                raise RuntimeError(msg)
            if rc in (NBLS_ERR_ARG, NBLS_ERR_UNSUPPORTED):
                err = ValueError(msg)
                err.code = rc                # (which of the two it was)
                raise err
            raise NblsError(rc, msg)

    def set_trace(self, data, fs):
        self.resident_key = None
        data = _f64(data)
        if data.ndim != 2:
            raise ValueError('trace must be (nchans, npts)')
        self._chk(self.lib.nbls_set_trace(self._h, _dptr(data), data.shape[0], data.shape[1], float(fs)))
        self.nchans, self.npts, self.fs = data.shape[0], data.shape[1], float(fs)

    def set_trace_rows(self, rows, fs):
        """rows: one 1-D float64 C-contiguous array per channel, all of the same length (uploaded
        straight from where they are: no packed host copy)."""
        self.resident_key = None
        npts = len(rows[0])
        keep = []
        for r in rows:
            r = np.asarray(r)
            if r.dtype != np.float64 or not r.flags.c_contiguous:
                r = np.ascontiguousarray(r, dtype=np.float64)
            if r.ndim != 1 or len(r) != npts:
                raise ValueError('All traces must have the same number of samples.')
            keep.append(r)
        ptrs = (C.c_void_p * len(keep))(*[r.ctypes.data for r in keep])
        self._chk(self.lib.nbls_set_trace_rows(self._h, ptrs, len(keep), npts, float(fs)))
        self.nchans, self.npts, self.fs = len(keep), npts, float(fs)

    def set_trace_shape(self, nchans, npts, fs):
        """Declare the trace (no samples yet): geometry and plan may follow while ``upload_rows`` runs on another thread."""
        self.resident_key = None
        self._chk(self.lib.nbls_set_trace_shape(self._h, int(nchans), int(npts), float(fs)))
        self.nchans, self.npts, self.fs = int(nchans), int(npts), float(fs)

    def expect_upload(self):
        """Announce (on the thread that goes on to plan and execute) that ``upload_rows`` is about to run on another
        thread: ``execute`` may then be called while the rows are still going up, the pass filters them as they land."""
        self._chk(self.lib.nbls_expect_upload(self._h))

    def upload_rows(self, rows):
        """The samples of the declared trace: one 1-D float64 C-contiguous array per channel."""
        self.resident_key = None
        try:
            keep = []
            for r in rows:
                r = np.asarray(r)
                if r.dtype != np.float64 or not r.flags.c_contiguous:
                    r = np.ascontiguousarray(r, dtype=np.float64)
                if r.ndim != 1 or len(r) != self.npts:
                    raise ValueError('All traces must have the same number of samples.')
                keep.append(r)
            if len(keep) != self.nchans:
                raise ValueError('upload_rows: %d rows for a trace declared with %d channels' % (len(keep), self.nchans))
            ptrs = (C.c_void_p * len(keep))(*[r.ctypes.data for r in keep])
        except BaseException:
            self.lib.nbls_abort_upload(self._h)        # (a pass that was queued on the announced rows fails instead of waiting)
            raise
        self._chk(self.lib.nbls_upload_rows(self._h, ptrs, len(keep), self.npts))

    def set_trace_from(self, other):
        """The trace of another handle on the same GPU, copied device-to-device."""
        self.resident_key = None
        self._chk(self.lib.nbls_set_trace_from(self._h, other._h))
        self.nchans, self.npts, self.fs = other.nchans, other.npts, other.fs

    def set_geometry(self, xij, pair_idx, xpinv):
        xij = _f64(xij)
        pair_idx = np.ascontiguousarray(pair_idx, dtype=np.int32)
        xpinv = _f64(xpinv)
        self._chk(self.lib.nbls_set_geometry(self._h, _dptr(xij), _iptr(pair_idx), _dptr(xpinv), xij.shape[0]))
        self.npairs = xij.shape[0]

    def plan(self, sos, zero_phase, taper_left, taper_right, winlen, wininc, vector_len, lts=None,
             xcorr_impl=0):
        """sos: (B, S, 6) or None (unfiltered single band).  lts: dict from planner.lts_plan()."""
        winlen = np.ascontiguousarray(winlen, dtype=np.int32)
        wininc = np.ascontiguousarray(wininc, dtype=np.int32)
        nb = len(winlen)
        if sos is None:
            sos_p, nsec = None, 0
        else:
            sos = _f64(sos)
            if sos.ndim != 3 or sos.shape[0] != nb or sos.shape[2] != 6:
                raise ValueError('sos must be (nbands, nsections, 6)')
            sos_p, nsec = _dptr(sos), sos.shape[1]
        tl = _f64(taper_left if taper_left is not None else np.zeros(0))
        tr = _f64(taper_right if taper_right is not None else np.zeros(0))
        if len(tl) != len(tr):
            raise ValueError('taper ramps must have equal length')
        lp = None
        keep = [sos, tl, tr, winlen, wininc]
        if lts is not None:
            p, held = _lts_params(lts)
            lp = C.byref(p)
            keep += held
        self._chk(self.lib.nbls_plan(self._h, nb, sos_p, nsec, int(bool(zero_phase)), _dptr(tl), _dptr(tr),
                                     len(tl), _iptr(winlen), _iptr(wininc), int(vector_len), lp,
                                     int(xcorr_impl)))
        self.nbands, self.vector_len = nb * self.nseg, int(vector_len)     # result rows: band-major, nseg per band
        self.fbands = nb
        self._nsec = nsec
        self.grid_n = self._want_grid_n
        self.taps = self._want_taps
        self.refine_levels = self._want_refine_levels
        self.capon = self._want_capon
        self.capon_peaks = self._want_capon_peaks
        self.capon_clean = self._want_capon_clean if self.capon else 0
        self.capon_music = self._want_capon_music if self.capon else None

    def set_option(self, key, value):
        """Per-handle implementation switch (``nbls_set_option``; identical results unless the library is the
        developer build and the key is one of its timing switches)."""
        self._chk(self.lib.nbls_set_option(self._h, key.encode(), int(value)))

    def reserve_results(self, nbytes):
        """Minimum allocation of the result block for the next plans (equal-sized gather blocks)."""
        self._chk(self.lib.nbls_reserve_results(self._h, int(nbytes)))

    def load_result_block(self, block):
        """Put a result block assembled on the host (several HBM rounds of one rank's share) back where the gather
        sends from.  ``block``: contiguous uint8 array in the layout of ``nbls_result_layout`` for all of the rank's bands."""
        block = np.ascontiguousarray(block, dtype=np.uint8)
        self._chk(self.lib.nbls_load_result_block(self._h, block.ctypes.data, block.nbytes))

    def set_segments(self, nseg):
        """The next plans treat the trace's rows as ``nseg`` recordings of one array (``nbls_set_segments``): nseg
        consecutive blocks of nchans / nseg rows; a plan of B bands then gives B * nseg result rows, row b * nseg + s."""
        self._chk(self.lib.nbls_set_segments(self._h, int(nseg)))
        self.nseg = int(nseg)

    def set_estimators(self, estimators=()):
        """Further estimators of the next plans (``nbls_set_estimators``), beside estimator 0 = what ``set_geometry`` /
        ``plan`` describe: a sequence of dicts with ``kept`` (0-based element indices, ascending), ``xij``, ``pair_idx``,
        ``xpinv`` of THAT array, ``lts`` (``planner.lts_plan`` dict, None for OLS) and ``eig6`` (``planner.uncertainty_frame``,
        None: no confidence intervals).  Empty: reset to the plain pass."""
        ests = list(estimators)
        descs, keep, npairs = estimator_descs(ests)
        self._chk(self.lib.nbls_set_estimators(self._h, len(ests), descs if ests else None))
        self.est_npairs = npairs

    def set_window_ranges(self, first=None, count=None):
        """Per-band window slices for the next plan(s); None resets to "all windows"."""
        if first is None:
            self._chk(self.lib.nbls_set_window_ranges(self._h, 0, None, None))
            return
        first = np.ascontiguousarray(first, dtype=np.int32)
        count = np.ascontiguousarray(count, dtype=np.int32)
        self._chk(self.lib.nbls_set_window_ranges(self._h, len(first), _iptr(first), _iptr(count)))

    def execute(self, stages=7, after=None):
        """Queue the pass.  ``after``: another handle of the same GPU whose pass was queued before — this pass's
        correlation stage then starts when that one's is through (``nbls_execute_after``)."""
        if after is not None:
            self._chk(self.lib.nbls_execute_after(self._h, after._h))
        else:
            self._chk(self.lib.nbls_execute_stages(self._h, int(stages)))

    def sync(self):
        self._chk(self.lib.nbls_sync(self._h))

    def _est_pairs(self, est):
        return self.npairs if est == 0 else self.est_npairs[est - 1]

    def fetch(self, want_lag=False, want_cmax=False, want_weights=False, want_z=False, grids=True, est=0):
        """``est``: the estimator whose results are fetched (0: the plan's own; its lag / cmax / weights are (B, VL, P'))."""
        B, VL, P = self.nbands, self.vector_len, self._est_pairs(est)
        if grids:
            g = np.empty((4, B, VL))               # one block: nbls_fetch moves the four grids in one copy
            out = dict(vel=g[0], baz=g[1], mdccm=g[2], sigma_tau=g[3], nwin=np.empty(B, dtype=np.int32))
        else:
            out = dict(vel=None, baz=None, mdccm=None, sigma_tau=None, nwin=np.empty(B, dtype=np.int32))
        lag = np.empty((B, VL, P), dtype=np.int32) if want_lag else None
        cmax = np.empty((B, VL, P)) if want_cmax else None
        wts = np.empty((B, VL, P), dtype=np.uint8) if want_weights else None
        z = np.empty((B, VL, 2)) if want_z else None
        args = (_dptr(out['vel']), _dptr(out['baz']), _dptr(out['mdccm']), _dptr(out['sigma_tau']), _iptr(out['nwin']),
                _iptr(lag), _dptr(cmax), _u8ptr(wts), _dptr(z))
        if est == 0:
            self._chk(self.lib.nbls_fetch(self._h, *args))
        else:
            self._chk(self.lib.nbls_est_fetch(self._h, int(est), *args))
        out.update(lag=lag, cmax=cmax, weights=wts, z=z)
        return out

    def fetch_packed(self, est=0):
        """One D2H copy of the result block (of estimator ``est``) -> dict(vel, baz, mdccm, sigma_tau (B, VL) float64 views
        of one buffer, mask (B, VL, ceil(P/8)) uint8: bit k & 7 of byte k >> 3 = LTS weight of pair k)."""
        lay = (C.c_int64 * 4)()
        if est == 0:
            self._chk(self.lib.nbls_result_layout(self._h, lay))
        else:
            self._chk(self.lib.nbls_est_result_layout(self._h, int(est), lay))
        cells, mb, total, moff = lay[0], lay[1], lay[2], lay[3]
        buf = np.empty(total // 8 + 1, dtype=np.float64)       # 8-byte aligned
        if est == 0:
            self._chk(self.lib.nbls_fetch_packed(self._h, buf.ctypes.data, total))
        else:
            self._chk(self.lib.nbls_est_fetch_packed(self._h, int(est), buf.ctypes.data, total))
        B, VL = self.nbands, self.vector_len
        grids = buf[:4 * cells].reshape(4, B, VL)
        mask = buf.view(np.uint8)[moff:moff + cells * mb].reshape(B, VL, mb)
        return dict(vel=grids[0], baz=grids[1], mdccm=grids[2], sigma_tau=grids[3], mask=mask)

    def set_uncertainty(self, eig6=None):
        """``eig6`` = (lambda_0, lambda_1, R00, R01, R10, R11) of the co-array (``planner.uncertainty_frame``): the
        next plans also compute ltsva's confidence intervals on the GPU; None switches that off."""
        e = None if eig6 is None else _f64(eig6)
        self._chk(self.lib.nbls_set_uncertainty(self._h, _dptr(e)))

    def fetch_uncertainty(self, est=0):
        """-> (vel_uncert, baz_uncert), each (nbands, vector_len)."""
        out = np.empty((2, self.nbands, self.vector_len))
        if est == 0:
            self._chk(self.lib.nbls_fetch_uncertainty(self._h, _dptr(out[0]), _dptr(out[1])))
        else:
            self._chk(self.lib.nbls_est_fetch_uncertainty(self._h, int(est), _dptr(out[0]), _dptr(out[1])))
        return out[0], out[1]

    def set_beam(self, on=True):
        """The next plans also compute, behind every unit's solve, the power and Fisher F-statistic of the delay-and-sum
        beam at the solved slowness (``nbls_set_beam``); False switches that off."""
        self._chk(self.lib.nbls_set_beam(self._h, int(bool(on))))

    def fetch_beam(self, e=0):
        """-> (beam_power, fstat) of estimator ``e``, each (rows, vector_len)."""
        out = np.empty((2, self.nbands, self.vector_len))
        if e == 0:
            self._chk(self.lib.nbls_fetch_beam(self._h, _dptr(out[0]), _dptr(out[1])))
        else:
            self._chk(self.lib.nbls_est_fetch_beam(self._h, int(e), _dptr(out[0]), _dptr(out[1])))
        return out[0], out[1]

    def set_closure(self, on=True):
        """The next plans also compute, behind every unit's solve, the closure of the picked lags per window and per
        element (``nbls_set_closure``); False switches that off."""
        self._chk(self.lib.nbls_set_closure(self._h, int(bool(on))))

    def _est_elements(self, e):
        if e == 0:
            return self.nchans // self.nseg
        return int(round((1.0 + (1.0 + 8.0 * self.est_npairs[e - 1]) ** 0.5) / 2.0))      # P' = n (n - 1) / 2

    def fetch_closure(self, e=0):
        """-> (consistency, closure_max, element_consistency) of estimator ``e``: (rows, vector_len) twice and
        (rows, vector_len, N), N that estimator's element count; seconds."""
        out = np.empty((2, self.nbands, self.vector_len))
        el = np.empty((self.nbands, self.vector_len, max(self._est_elements(e), 1)))
        if e == 0:
            self._chk(self.lib.nbls_fetch_closure(self._h, _dptr(out[0]), _dptr(out[1]), _dptr(el)))
        else:
            self._chk(self.lib.nbls_est_fetch_closure(self._h, int(e), _dptr(out[0]), _dptr(out[1]), _dptr(el)))
        return out[0], out[1], el

    def set_kept_elements(self, min_pairs=0, beam=False, capon=False):
        """The next plans also work out, behind every unit's solve, which elements LTS has dropped — those with at least
        ``min_pairs`` pairs of weight 0 — and, with ``beam`` / ``capon``, form the plan's beam results / Capon spectra over
        the elements it kept (``nbls_set_kept_elements``); 0 switches that off."""
        flags = (KEPT_BEAM if beam else 0) | (KEPT_CAPON if capon else 0)
        self._chk(self.lib.nbls_set_kept_elements(self._h, int(min_pairs), flags))

    def fetch_kept_elements(self):
        """-> (dropped_mask uint32, kept_count int32), (rows, vector_len) each: bit m of the mask is set where element m
        is dropped; the count is that of the elements the beam and the spectra are formed over."""
        mask = np.empty((self.nbands, self.vector_len), dtype=np.uint32)
        count = np.empty((self.nbands, self.vector_len), dtype=np.int32)
        self._chk(self.lib.nbls_fetch_kept_elements(self._h, mask.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                    count.ctypes.data_as(C.POINTER(C.c_int32))))
        return mask, count

    def set_beam_trace(self, window=None, mdccm_min=None, kept=False):
        """The next plans also form, behind the pass's last solve, the beam trace of every result row: the delay-and-sum
        beam at each window's solved slowness, the windows stitched with the synthesis windows ``window`` — those of the
        plan's bands one after the other, sum of the window lengths entries (``planner.beam_trace_window`` makes one) —
        using only the windows with MdCCM >= ``mdccm_min`` (None: all) and, with ``kept``, the elements LTS kept in each
        (``nbls_set_beam_trace``); None switches that off."""
        if window is None:
            self._chk(self.lib.nbls_set_beam_trace(self._h, None, 0, float('nan'), 0))
            return
        w = _f64(np.asarray(window, dtype=np.float64).reshape(-1))
        self._chk(self.lib.nbls_set_beam_trace(self._h, _dptr(w), w.size, float('nan') if mdccm_min is None else float(mdccm_min),
                                               BEAM_TRACE_KEPT if kept else 0))

    def fetch_beam_trace(self, row):
        """-> the beam trace (npts,) of result row ``row``."""
        out = np.empty(self.npts)
        self._chk(self.lib.nbls_fetch_beam_trace(self._h, int(row), _dptr(out)))
        return out

    def set_families(self, params=None):
        """The next plans also group, behind the pass's last solve, the cells of estimator 0's result grids into families:
        connected components of the eligible cells under the link of ``params`` (a ``FamilyParams``, see ``family_params``;
        ``nbls_set_families``); None switches that off."""
        self._chk(self.lib.nbls_set_families(self._h, None if params is None else C.byref(params)))

    def _family_results(self, call, cells_shape, capacity):
        family = np.empty(cells_shape, dtype=np.int32)
        nfam = C.c_int32(0)
        cap = family.size if capacity is None else int(capacity)
        if cap < 0:
            raise ValueError('capacity must not be negative')
        table = np.zeros((cap, FAMILY_COLUMNS), dtype=np.int64)
        self._chk(call(_iptr(family), C.byref(nfam), table.ctypes.data_as(C.POINTER(C.c_int64)), cap))
        return family, int(nfam.value), table[:min(int(nfam.value), cap)]

    def fetch_families(self, capacity=None):
        """-> (family int32 (rows, vector_len), nfamilies, table int64 (min(nfamilies, capacity), 8)); the columns of the
        table are ``FAMILY_FIELDS``.  ``capacity`` None: every family."""
        if capacity is None:                   # (one round trip for the count, then a table of that size)
            nfam = C.c_int32(0)
            self._chk(self.lib.nbls_fetch_families(self._h, None, C.byref(nfam), None, 0))
            capacity = int(nfam.value)
        return self._family_results(lambda f, n, t, c: self.lib.nbls_fetch_families(self._h, f, n, t, c),
                                    (self.nbands, self.vector_len), capacity)

    def label_families(self, params, nseg, winlen, wininc, nwin, vel, baz, mdccm, sigma_tau=None, capacity=None):
        """The families of grids the caller has (``nbls_label_families``): ``winlen`` / ``wininc`` (nbands,), ``nwin``
        (nbands * nseg,), the grids (nbands * nseg, vector_len), ``sigma_tau`` None exactly when ``params`` has no gate.
        The same kernels as a plan with ``set_families``; needs no plan and changes none.  -> as ``fetch_families``
        (``capacity`` None: room for every family the lattice can hold)."""
        winlen = np.ascontiguousarray(winlen, dtype=np.int32).reshape(-1)
        wininc = np.ascontiguousarray(wininc, dtype=np.int32).reshape(-1)
        nwin = np.ascontiguousarray(nwin, dtype=np.int32).reshape(-1)
        vel, baz, mdccm = _f64(vel), _f64(baz), _f64(mdccm)
        sig = None if sigma_tau is None else _f64(sigma_tau)
        rows = winlen.size * int(nseg)
        if vel.ndim != 2 or vel.shape[0] != rows or wininc.size != winlen.size or nwin.size != rows:
            raise ValueError('label_families: the grids must be (nbands * nseg, vector_len), nwin one entry per row')
        for g in (baz, mdccm, sig):
            if g is not None and g.shape != vel.shape:
                raise ValueError('label_families: the grids must have one shape')
        if capacity is None:
            capacity = vel.size // max(int(params.min_pixels), 1)
        return self._family_results(
            lambda f, n, t, c: self.lib.nbls_label_families(self._h, C.byref(params), winlen.size, int(nseg), vel.shape[1], _iptr(winlen),
                                                            _iptr(wininc), _iptr(nwin), _dptr(vel), _dptr(baz), _dptr(mdccm), _dptr(sig),
                                                            f, n, t, c), vel.shape, capacity)

    def set_element_delays(self, max_shift=None, kept=False):
        """The next plans also measure, behind every unit's solve, each element's delay against the beam of the others:
        the shift within +-``max_shift[b]`` samples (one entry per band of the plan, 0..256) of the delay the solved
        slowness predicts at which the element correlates best with the sum of the other elements — with ``kept`` of
        those LTS kept (needs ``set_kept_elements``) — (``nbls_set_element_delays``); None switches
        that off."""
        if max_shift is None:
            self._chk(self.lib.nbls_set_element_delays(self._h, None, 0, 0))
            return
        k = np.ascontiguousarray(np.asarray(max_shift).reshape(-1), dtype=np.int32)
        self._chk(self.lib.nbls_set_element_delays(self._h, k.ctypes.data_as(C.POINTER(C.c_int32)), k.size,
                                                   ELEMENT_DELAY_KEPT if kept else 0))

    def fetch_element_delays(self):
        """-> (delay, cc, shift), (rows, vector_len, N) each: seconds, the normalised correlation at the picked shift, and
        the shift (int32, samples)."""
        n = max(self._est_elements(0), 1)
        delay = np.empty((self.nbands, self.vector_len, n))
        cc = np.empty((self.nbands, self.vector_len, n))
        shift = np.empty((self.nbands, self.vector_len, n), dtype=np.int32)
        self._chk(self.lib.nbls_fetch_element_delays(self._h, _dptr(delay), _dptr(cc), shift.ctypes.data_as(C.POINTER(C.c_int32))))
        return delay, cc, shift

    def set_beam_grid(self, grid=None, want_map=False):
        """The next plans also search, per window, the beam F-statistic of the full array over the slowness vectors
        ``grid`` (G, 2) in s/km (``nbls_set_beam_grid``; ``planner.slowness_grid`` makes one);
        ``want_map``: they keep every F(g) too.  None switches that off."""
        if grid is None:
            self._chk(self.lib.nbls_set_beam_grid(self._h, None, 0, 0))
            self._want_grid_n = 0
            return
        g = _f64(grid)
        if g.ndim != 2 or g.shape[1] != 2:
            raise ValueError('the slowness grid must be (G, 2), not %r' % (g.shape,))
        self._chk(self.lib.nbls_set_beam_grid(self._h, _dptr(g), g.shape[0], int(bool(want_map))))
        self._want_grid_n = g.shape[0]

    def set_capon(self, grid=None, freqs=None, snap_len=None, snap_hop=None, loading=0.01, want_maps=False, want_csdm=False):
        """The next plans also compute, per window, the Capon and Bartlett slowness spectra of the narrow band's
        cross-spectral matrix over the slowness vectors ``grid`` (G, 2) in s/km (``nbls_set_capon``):
        per band a frequency (Hz), a snapshot length and a hop (samples), one diagonal ``loading``; ``want_maps`` keeps
        both spectra, ``want_csdm`` the matrix.  ``grid=None`` switches it off again."""
        if grid is None:
            self._chk(self.lib.nbls_set_capon(self._h, None, 0, None, None, None, 0, 0.0, 0))
            self._want_capon = None
            return
        g, f = _f64(grid), _f64(freqs)
        ls = np.ascontiguousarray(snap_len, dtype=np.int32)
        hs = np.ascontiguousarray(snap_hop, dtype=np.int32)
        if g.ndim != 2 or g.shape[1] != 2 or g.shape[0] < 1:
            raise ValueError('the slowness grid must be (G, 2) with G >= 1, not %r' % (g.shape,))
        if f.ndim != 1 or ls.shape != f.shape or hs.shape != f.shape:
            raise ValueError('one frequency, snapshot length and hop per band')
        flags = (CAPON_MAPS if want_maps else 0) | (CAPON_CSDM if want_csdm else 0)
        self._chk(self.lib.nbls_set_capon(self._h, _dptr(g), g.shape[0], _dptr(f), _iptr(ls), _iptr(hs), len(f), float(loading),
                                          flags))
        self._want_capon = (g.shape[0], ls.copy())

    def fetch_capon(self):
        """-> (capon_index int32, capon_power, bartlett_index int32, bartlett_power), each (rows, vector_len)."""
        idx = np.empty((2, self.nbands, self.vector_len), dtype=np.int32)
        out = np.empty((2, self.nbands, self.vector_len))
        self._chk(self.lib.nbls_fetch_capon(self._h, _iptr(idx[0]), _dptr(out[0]), _iptr(idx[1]), _dptr(out[1])))
        return idx[0], out[0], idx[1], out[1]

    def set_capon_peaks(self, cells=None, K=0, floor=0.25):
        """The next plans (with ``set_capon``) also pick, per window and spectrum, the ``K`` strongest local maxima on the
        lattice ``cells`` (G, 2) int32 that are no lower than ``floor`` times the maximum (``nbls_set_capon_peaks``, DESIGN.md
        section 19).  ``cells=None`` or ``K=0`` switches it off again."""
        if cells is None or not K:
            self._chk(self.lib.nbls_set_capon_peaks(self._h, None, 0, 0, 0.0))
            self._want_capon_peaks = 0
            return
        c = np.ascontiguousarray(cells, dtype=np.int32)
        if c.ndim != 2 or c.shape[1] != 2 or c.shape[0] < 1:
            raise ValueError('the cells must be (G, 2) with G >= 1, not %r' % (c.shape,))
        self._chk(self.lib.nbls_set_capon_peaks(self._h, _iptr(c), c.shape[0], int(K), float(floor)))
        self._want_capon_peaks = int(K)

    def fetch_capon_peaks(self, which):
        """The peaks of the Capon (``which`` 0) or Bartlett (1) spectrum -> (count int32 (rows, vector_len), index int32
        (rows, vector_len, K), power (rows, vector_len, K), offset (rows, vector_len, K, 2))."""
        K = max(self.capon_peaks, 1)
        cnt = np.empty((self.nbands, self.vector_len), dtype=np.int32)
        idx = np.empty((self.nbands, self.vector_len, K), dtype=np.int32)
        pw = np.empty((self.nbands, self.vector_len, K))
        off = np.empty((self.nbands, self.vector_len, K, 2))
        self._chk(self.lib.nbls_fetch_capon_peaks(self._h, int(which), _iptr(cnt), _iptr(idx), _dptr(pw), _dptr(off)))
        return cnt, idx, pw, off

    def set_capon_clean(self, iterations, gain=0.5, floor=0.02, residual=False):
        """The next plans (with ``set_capon``) also resolve every window's arrivals by CLEAN-SC: up to ``iterations`` (1..32)
        times the Bartlett maximum of the cross-spectral matrix is taken and ``gain`` in (0, 1] of everything coherent with
        that beam removed from the matrix, until the maximum falls below ``floor`` in [0, 1) times the first one
        (``nbls_set_capon_clean``); ``residual``: the plan also keeps the matrix that is left.
        ``iterations=0`` switches it off again."""
        if not iterations:
            self._chk(self.lib.nbls_set_capon_clean(self._h, 0, 0.0, 0.0, 0))
            self._want_capon_clean = 0
            return
        self._chk(self.lib.nbls_set_capon_clean(self._h, int(iterations), float(gain), float(floor), CLEAN_RESIDUAL if residual else 0))
        self._want_capon_clean = int(iterations)

    def fetch_capon_clean(self):
        """The CLEAN-SC components -> (count int32 (rows, vector_len), index int32 (rows, vector_len, I), power (rows,
        vector_len, I), total (rows, vector_len), residual (rows, vector_len))."""
        n = max(self.capon_clean, 1)
        cnt = np.empty((self.nbands, self.vector_len), dtype=np.int32)
        idx = np.empty((self.nbands, self.vector_len, n), dtype=np.int32)
        pw = np.empty((self.nbands, self.vector_len, n))
        tr = np.empty((2, self.nbands, self.vector_len))
        self._chk(self.lib.nbls_fetch_capon_clean(self._h, _iptr(cnt), _iptr(idx), _dptr(pw), _dptr(tr[0]), _dptr(tr[1])))
        return cnt, idx, pw, tr[0], tr[1]

    def fetch_capon_clean_csdm(self):
        """-> the matrix CLEAN-SC has left of every window, complex128 (rows, vector_len, N, N) (a plan made with ``residual``)."""
        N = self.nchans // self.nseg
        out = np.empty((self.nbands, self.vector_len, N, N), dtype=np.complex128)
        self._chk(self.lib.nbls_fetch_capon_clean_csdm(self._h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def set_capon_music(self, sources=0, eig_floor=0.05, maps=False, vectors=False, peaks=False, peak_floor=0.0):
        """The next plans (with ``set_capon``) also decompose every window's cross-spectral matrix: its eigenvalues, and the
        MUSIC pseudo-spectrum over the grid with ``sources`` = M in 1..N-1 signal eigenvectors, or (``sources=0``) as many
        as there are eigenvalues of at least ``eig_floor`` in (0, 1) times the largest (``nbls_set_capon_music``, DESIGN.md
        section 25); ``maps``: the plan keeps the spectrum of every window, ``vectors``: the eigenvectors, ``peaks``: the K
        strongest local maxima of the spectrum, K and the cells those of ``set_capon_peaks`` (which the plan needs), kept from
        ``peak_floor`` in [0, 1) times the maximum.  ``sources=None`` switches it off again."""
        if sources is None:
            self._chk(self.lib.nbls_set_capon_music(self._h, -1, 0.0, 0.0, 0))
            self._want_capon_music = None
            return
        flags = (MUSIC_MAP if maps else 0) | (MUSIC_VECTORS if vectors else 0) | (MUSIC_PEAKS if peaks else 0)
        self._chk(self.lib.nbls_set_capon_music(self._h, int(sources), float(eig_floor), float(peak_floor), flags))
        self._want_capon_music = (int(sources), bool(maps), bool(vectors), bool(peaks))

    def fetch_capon_music(self):
        """-> (eigenvalues (rows, vector_len, N) descending, sources int32 (rows, vector_len), sweeps int32, index int32 and
        power (rows, vector_len)) of a plan made with ``set_capon_music``."""
        N = self.nchans // self.nseg
        ev = np.empty((self.nbands, self.vector_len, N))
        ints = np.empty((3, self.nbands, self.vector_len), dtype=np.int32)
        pw = np.empty((self.nbands, self.vector_len))
        self._chk(self.lib.nbls_fetch_capon_music(self._h, _dptr(ev), _iptr(ints[0]), _iptr(ints[1]), _iptr(ints[2]), _dptr(pw)))
        return ev, ints[0], ints[1], ints[2], pw

    def fetch_capon_music_peaks(self):
        """The K strongest peaks of the MUSIC spectrum -> (count int32 (rows, vector_len), index int32 (rows, vector_len, K),
        power (rows, vector_len, K), offset (rows, vector_len, K, 2)), as ``fetch_capon_peaks`` returns a spectrum's (a plan made
        with ``peaks``)."""
        K = max(self.capon_peaks, 1)
        cnt = np.empty((self.nbands, self.vector_len), dtype=np.int32)
        idx = np.empty((self.nbands, self.vector_len, K), dtype=np.int32)
        pw = np.empty((self.nbands, self.vector_len, K))
        off = np.empty((self.nbands, self.vector_len, K, 2))
        self._chk(self.lib.nbls_fetch_capon_music_peaks(self._h, _iptr(cnt), _iptr(idx), _dptr(pw), _dptr(off)))
        return cnt, idx, pw, off

    def fetch_capon_music_map(self):
        """-> the MUSIC pseudo-spectrum of every window, (rows, vector_len, G) (a plan made with ``maps``)."""
        G = self.capon[0] if self.capon else 1
        out = np.empty((self.nbands, self.vector_len, G))
        self._chk(self.lib.nbls_fetch_capon_music_map(self._h, _dptr(out)))
        return out

    def fetch_capon_music_vectors(self):
        """-> the eigenvectors of every window, complex128 (rows, vector_len, N, N), column k beside eigenvalue k (a plan made
        with ``vectors``)."""
        N = self.nchans // self.nseg
        out = np.empty((self.nbands, self.vector_len, N, N), dtype=np.complex128)
        self._chk(self.lib.nbls_fetch_capon_music_vectors(self._h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def fetch_capon_maps(self):
        """-> (capon_map, bartlett_map), each (rows, vector_len, G) (a plan made with ``want_maps``)."""
        G = self.capon[0] if self.capon else 1
        out = np.empty((2, self.nbands, self.vector_len, G))
        self._chk(self.lib.nbls_fetch_capon_maps(self._h, _dptr(out[0]), _dptr(out[1])))
        return out[0], out[1]

    def fetch_capon_csdm(self):
        """-> the cross-spectral matrix of every window, complex128 (rows, vector_len, N, N) (a plan made with ``want_csdm``)."""
        N = self.nchans // self.nseg
        out = np.empty((self.nbands, self.vector_len, N, N), dtype=np.complex128)
        self._chk(self.lib.nbls_fetch_capon_csdm(self._h, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def fetch_capon_tables(self, band):
        """-> (snapshot coefficients complex128 (Ls,), steering vectors complex128 (G, N)) of band ``band`` of the plan."""
        G, ls = self.capon if self.capon else (1, np.ones(max(1, self.fbands), dtype=np.int32))
        coef = np.empty(int(ls[band]) if 0 <= band < len(ls) else 1, dtype=np.complex128)
        steer = np.empty((G, self.nchans // self.nseg), dtype=np.complex128)
        cd = C.POINTER(C.c_double)
        self._chk(self.lib.nbls_fetch_capon_tables(self._h, int(band), coef.ctypes.data_as(cd), steer.ctypes.data_as(cd)))
        return coef, steer

    def fetch_beam_grid(self):
        """-> (grid_index int32, grid_fstat, grid_power) of the plan's slowness-grid search, each (rows, vector_len)."""
        idx = np.empty((self.nbands, self.vector_len), dtype=np.int32)
        out = np.empty((2, self.nbands, self.vector_len))
        self._chk(self.lib.nbls_fetch_beam_grid(self._h, _iptr(idx), _dptr(out[0]), _dptr(out[1])))
        return idx, out[0], out[1]

    def fetch_beam_grid_map(self):
        """-> F of every grid point, (rows, vector_len, G) (a plan made with ``want_map``)."""
        out = np.empty((self.nbands, self.vector_len, max(self.grid_n, 1)))
        self._chk(self.lib.nbls_fetch_beam_grid_map(self._h, _dptr(out)))
        return out

    def fetch_beam_grid_delays(self):
        """-> the plan's delay table, (G, nelem) int32."""
        out = np.empty((max(self.grid_n, 1), self.nchans // self.nseg), dtype=np.int32)
        self._chk(self.lib.nbls_fetch_beam_grid_delays(self._h, _iptr(out)))
        return out

    def set_beam_interpolation(self, taps=8):
        """The next plans steer their beam (``set_beam``) and their slowness grid (``set_beam_grid``) at fractional-sample
        delays through a Lagrange interpolator of ``taps`` samples, 4, 6 or 8 (``nbls_set_beam_interpolation``, DESIGN.md
        section 22; ``planner.steering_error`` has its error); 0 switches that off."""
        self._chk(self.lib.nbls_set_beam_interpolation(self._h, int(taps)))
        self._want_taps = int(taps)

    def set_beam_grid_refinement(self, levels, step):
        """The next plans — plans with a slowness grid (``set_beam_grid``) steered at fractional-sample delays
        (``set_beam_interpolation``) — refine every window's grid maximum between the grid points: ``levels`` (1..12) times
        the best of the centre and its eight neighbours at ``step`` (h0, h1) s/km halved per level
        (``nbls_set_beam_grid_refinement``; ``planner.check_grid_refinement`` makes the step from the
        grid).  ``levels=0`` or ``step=None`` switches that off; both arguments are required."""
        if not levels or step is None:
            self._chk(self.lib.nbls_set_beam_grid_refinement(self._h, 0, None))
            self._want_refine_levels = 0
            return
        s = _f64(step).reshape(-1)
        if s.shape != (2,):
            raise ValueError('the refinement step must be two values (h0, h1), not %r' % (np.shape(step),))
        self._chk(self.lib.nbls_set_beam_grid_refinement(self._h, int(levels), _dptr(s)))
        self._want_refine_levels = int(levels)

    def fetch_beam_grid_refined(self):
        """-> (grid_refined_slowness (rows, vector_len, 2), grid_refined_fstat, grid_refined_power (rows, vector_len),
        grid_refined_path (rows, vector_len, R) int32, grid_refined_stencil (rows, vector_len, 9)) of a plan that refines its
        grid maximum."""
        cells = (self.nbands, self.vector_len)
        slow, fstat, power = np.empty(cells + (2,)), np.empty(cells), np.empty(cells)
        path = np.empty(cells + (max(self.refine_levels, 1),), dtype=np.int32)
        stencil = np.empty(cells + (9,))
        self._chk(self.lib.nbls_fetch_beam_grid_refined(self._h, _dptr(slow), _dptr(fstat), _dptr(power), _iptr(path), _dptr(stencil)))
        return slow, fstat, power, path, stencil

    def fetch_beam_grid_coefficients(self):
        """-> the Lagrange coefficients of an interpolated grid plan, (G, nelem, taps); ``fetch_beam_grid_delays`` then
        returns ``floor`` of the delays."""
        out = np.empty((max(self.grid_n, 1), self.nchans // self.nseg, max(self.taps, 1)))
        self._chk(self.lib.nbls_fetch_beam_grid_coefficients(self._h, _dptr(out)))
        return out

    def set_lag_refinement(self, on=True):
        """The next plans also refine every picked lag to sub-sample precision behind its verifier, and their solves read
        ``tau = (lag + frac) / fs`` (``nbls_set_lag_refinement``); False switches that off."""
        self._chk(self.lib.nbls_set_lag_refinement(self._h, int(bool(on))))

    def fetch_lag_fraction(self, e=0):
        """-> the sub-sample fractions of estimator ``e``'s lags, (rows, vector_len, pairs of that estimator)."""
        out = np.empty((self.nbands, self.vector_len, self._est_pairs(e)))
        if e == 0:
            self._chk(self.lib.nbls_fetch_lag_fraction(self._h, _dptr(out)))
        else:
            self._chk(self.lib.nbls_est_fetch_lag_fraction(self._h, int(e), _dptr(out)))
        return out

    def set_lag_limits(self, max_lag=None):
        """The next plans search the lag of pair k only within ``|lag| <= max_lag[k]`` samples (``nbls_set_lag_limits``,
        DESIGN.md section 14; ``planner.lag_limits`` makes the table); None switches that off."""
        if max_lag is None:
            self._chk(self.lib.nbls_set_lag_limits(self._h, None, 0))
            return
        t = np.ascontiguousarray(max_lag, dtype=np.int32).ravel()
        self._chk(self.lib.nbls_set_lag_limits(self._h, _iptr(t), len(t)))

    def set_lag_seed(self, halfwidth=None):
        """The next plans — plans with a slowness grid (``set_beam_grid``) — search every pair's lag only within
        ``halfwidth[b]`` samples of the delay the unit's grid maximum predicts for the pair (``nbls_set_lag_seed``,
        DESIGN.md section 16; ``planner.seed_halfwidths`` makes the table, one entry per band); None switches that off."""
        if halfwidth is None:
            self._chk(self.lib.nbls_set_lag_seed(self._h, None, 0))
            return
        t = np.ascontiguousarray(halfwidth, dtype=np.int32).ravel()
        self._chk(self.lib.nbls_set_lag_seed(self._h, _iptr(t), len(t)))

    def stream_results(self, on=True):
        """The next passes deliver their rows batch by batch into a pinned host mirror of the result block
        (``nbls_stream_results``); see ``result_batches`` / ``wait_result_batch``."""
        self._chk(self.lib.nbls_stream_results(self._h, int(bool(on))))

    def result_batches(self):
        n = C.c_int32()
        self._chk(self.lib.nbls_result_batches(self._h, C.byref(n)))
        return n.value

    def wait_result_batch(self, k, est=0):
        """Wait for batch ``k`` of the queued pass -> (u0, u1, c0, c1, grids (4, B*VL) float64, mask (B*VL, MB) uint8):
        the batch's units [u0, u1) own the cells [c0, c1) of the two VIEWS of the library's pinned mirror (valid until
        the handle's next pass; cells of batches not yet waited for are undefined)."""
        out = (C.c_int64 * 4)()
        blk = C.c_void_p()
        if est == 0:
            self._chk(self.lib.nbls_wait_result_batch(self._h, int(k), out, C.byref(blk)))
        else:
            self._chk(self.lib.nbls_est_wait_result_batch(self._h, int(est), int(k), out, C.byref(blk)))
        cells = self.nbands * self.vector_len
        mb = (self._est_pairs(est) + 7) // 8
        raw = (C.c_uint8 * (cells * (32 + mb))).from_address(blk.value)
        buf = np.frombuffer(raw, dtype=np.uint8)
        grids = buf[:32 * cells].view(np.float64).reshape(4, cells)
        mask = buf[32 * cells:].reshape(cells, mb)
        return out[0], out[1], out[2], out[3], grids, mask

    def fetch_filtered(self, band):
        out = np.empty((self.nchans, self.npts))
        self._chk(self.lib.nbls_fetch_filtered(self._h, int(band), _dptr(out)))
        return out

    def filter_segment(self, reverse=False, state_in=None, want_state=False):
        """One causal filter pass over the resident segment continuing from ``state_in`` (nbands, nchans, 2*nsections)
        -> the state leaving the segment (or None).  See ``nbls_filter_segment``."""
        si = None if state_in is None else _f64(state_in)
        so = np.empty((self.fbands, self.nchans, 2 * self._nsec)) if want_state else None
        self._chk(self.lib.nbls_filter_segment(self._h, int(bool(reverse)), _dptr(si), _dptr(so)))
        return so

    def set_filtered(self, band, data):
        data = _f64(data)
        if data.shape != (self.nchans, self.npts):
            raise ValueError('filtered band must be (nchans, npts)')
        self._chk(self.lib.nbls_set_filtered(self._h, int(band), _dptr(data)))

    def device_results(self):
        ptrs = (C.c_void_p * 5)()
        nbytes = C.c_int64()
        self._chk(self.lib.nbls_device_results(self._h, ptrs, C.byref(nbytes)))
        return [p or 0 for p in ptrs], nbytes.value

    def set_profiling(self, on=True):
        self._chk(self.lib.nbls_set_profiling(self._h, int(bool(on))))
        self.profiling = bool(on)

    def timings(self):
        t = Timings()
        self._chk(self.lib.nbls_get_timings(self._h, C.byref(t)))
        return dict(filter_ms=t.filter_ms, xcorr_ms=t.xcorr_ms, solve_ms=t.solve_ms,
                    total_ms=t.total_ms, xcorr_launches=t.xcorr_launches, quantize_ms=t.quantize_ms,
                    screen_ms=t.screen_ms, verify_ms=t.verify_ms, xcorr_impl=t.xcorr_impl,
                    xcorr_fallback_bands=t.xcorr_fallback_bands)

    def screen_stamps(self):
        out = np.zeros(10)
        self._chk(self.lib.nbls_debug_screen_stamps(self._h, _dptr(out)))
        return dict(zip(('stage_issue', 'stage_wait', 'compute_wave0', 'wait_other_waves', 'merge_write', 'total',
                         'kloop_cycles_wave0', 'epilogue_cycles_wave0', 'epi_convert', 'epi_lds_roundtrip'), out))

    def lts_stamps(self):
        out = np.zeros(8)
        self._chk(self.lib.nbls_debug_lts_stamps(self._h, _dptr(out)))
        return dict(zip(('setup_medians', 'elemental_starts', 'csteps', 'peel', 'refine', 'finish', 'nfin', 'total'), out))

    def lts_coop_breakdown(self):
        out = np.zeros(8)
        self._chk(self.lib.nbls_debug_lts_coop_breakdown(self._h, _dptr(out)))
        return dict(zip(('groups', 'merge', 'compact', 'live_entries_total', 'w0_passes', 'w0_select', 'w0_sums', 'w0_groups'), out))

    def screen_stats(self):
        out = (C.c_int64 * 8)()
        self._chk(self.lib.nbls_debug_screen_stats(self._h, out))
        return dict(pairs=out[0], overflow=out[1], candidates=out[2], max_candidates=out[3], lag_runs=out[4],
                    lags_in_runs_of_2_or_more=out[5])

    def screen_records(self):
        """The candidate records of the last screened unit batch (``nbls_debug_screen_records``) -> (units, N, N, 32)
        int32, N the elements of one recording: record [u, i, j] of sliding channel i and partner j = count, flags
        (1 interval, 2 list overflow), kk_lo, kk_hi, screening maximum and theta (f32 bits), up to 26 np.correlate
        indices.  The diagonal, which the kernel does not write, comes back as zeros."""
        units = C.c_int64()
        self._chk(self.lib.nbls_debug_screen_records(self._h, None, 0, C.byref(units)))
        n = self.nchans // self.nseg
        out = np.zeros((units.value, n, n, 32), dtype=np.int32)
        self._chk(self.lib.nbls_debug_screen_records(self._h, _iptr(out), out.size, C.byref(units)))
        out[:, np.arange(n), np.arange(n)] = 0
        return out

    def probe_mfma_i8(self, a, b):
        """a, b: (64, 16) int8 per-lane fragments -> (64, 4) int32 accumulators."""
        a = np.ascontiguousarray(a, dtype=np.int8).view(np.int32).reshape(64, 4)
        b = np.ascontiguousarray(b, dtype=np.int8).view(np.int32).reshape(64, 4)
        out = np.empty((64, 4), dtype=np.int32)
        self._chk(self.lib.nbls_probe_mfma_i8(self._h, _iptr(a), _iptr(b), _iptr(out)))
        return out

    def probe_mfma_f64(self, a, b):
        a = _f64(a); b = _f64(b)
        out = np.empty(256)
        self._chk(self.lib.nbls_probe_mfma_f64(self._h, _dptr(a), _dptr(b), _dptr(out)))
        return out.reshape(64, 4)


def refine_lds_bytes(nelem, W):
    """Dynamic LDS bytes of the form ``refine_lag_kernel`` takes for windows of W samples of ``nelem`` elements; 0: the
    form that reads global memory (``nbls_refine_lds_bytes``)."""
    rc = load_library().nbls_refine_lds_bytes(int(nelem), int(W))
    if rc < 0:
        raise ValueError('nbls_refine_lds_bytes: bad arguments')
    return int(rc)


def lag_limit_form(nelem, W, min_limit):
    """The form a window group of W-sample windows of ``nelem`` elements takes under lag limits whose smallest is
    ``min_limit`` (``nbls_lag_limit_form``): 0 the plan's ordinary route, 1 the matrix-core form, 2 the general form."""
    rc = load_library().nbls_lag_limit_form(int(nelem), int(W), int(min(int(min_limit), 2 ** 31 - 1)))
    if rc < 0:
        raise ValueError('nbls_lag_limit_form: arguments out of range')
    return int(rc)


def lag_seed_form(nelem, W, max_halfwidth=0, halo=0):
    """The form a window group of W-sample windows of ``nelem`` elements takes in a seeded plan (``nbls_lag_seed_form``):
    1 the staged form, 2 the general form."""
    rc = load_library().nbls_lag_seed_form(int(nelem), int(W), int(min(int(max_halfwidth), 2 ** 31 - 1)), int(halo))
    if rc < 0:
        raise ValueError('nbls_lag_seed_form: arguments out of range')
    return int(rc)


def _route_args(nelem, npairs):
    return int(nelem), int(nelem * (nelem - 1) // 2 if npairs is None else npairs)


def route(nelem, W, npairs=None, vrows=1, npts_pad=64, xcorr_impl=0, flags=0):
    """The correlator route of windows of W samples (nbls_route_xcorr; host only, no device) -> dict of the
    nbls_route fields.  npairs None: every pair of the array."""
    nelem, npairs = _route_args(nelem, npairs)
    r = Route()
    rc = load_library().nbls_route_xcorr(nelem, int(W), npairs, int(vrows), int(npts_pad), int(xcorr_impl), int(flags),
                                         C.byref(r))
    if rc != 0:
        raise ValueError('nbls_route_xcorr: arguments out of range')
    return {k: (list(getattr(r, k)) if k.startswith('lds') else getattr(r, k)) for k in ROUTE_DTYPE.names}


def route_table(nelem, W0, W1, npairs=None, vrows=1, npts_pad=64, xcorr_impl=0, flags=0):
    """The routes of W = W0..W1 (nbls_route_table: the scan runs in the library) -> structured array, row W - W0."""
    nelem, npairs = _route_args(nelem, npairs)
    out = np.zeros(int(W1) - int(W0) + 1, dtype=ROUTE_DTYPE)
    rc = load_library().nbls_route_table(nelem, int(W0), int(W1), npairs, int(vrows), int(npts_pad), int(xcorr_impl),
                                         int(flags), out.ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise ValueError('nbls_route_table: arguments out of range')
    return out


def route_boundaries(nelem, W0=2, W1=16384, npairs=None, vrows=1, npts_pad=64, xcorr_impl=0, flags=0):
    """Every pair (W_last, W_first) of adjacent window lengths in W0..W1 where any field of the route (kernels,
    tiling, LDS) changes: the window lengths where a correlator can go wrong without its neighbours noticing."""
    t = route_table(nelem, W0, W1, npairs, vrows, npts_pad, xcorr_impl, flags)
    same = np.ones(len(t) - 1, dtype=bool)
    for k in ROUTE_KEYS:
        same &= t[k][1:] == t[k][:-1]
    w = np.flatnonzero(~same) + int(W0)
    return [(int(a), int(a) + 1) for a in w]
