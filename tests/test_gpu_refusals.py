"""What ``nbls_plan`` refuses of a plan's opt-in requests, and when the opt-in results of a plan are there.

The table has one row per refusal of ``plan_check_args`` (csrc/api.hip) from the segment checks to the lag-seed checks: the
calls that provoke it, the error code and the whole message, which is compared for equality.  Each row plans on a handle of
its own, at the smallest shapes that reach the refusal: 4 or 5 elements (8 rows as 2 segments), 256 samples, 1 or 2 bands,
windows of 32 samples, a 3 x 3 slowness grid.  Rows that carry two faults pin which of them is reported.

Left out, 10 of the 55:
- the 8 refusals that only a handle with an RCCL communicator reaches (a communicator lives as long as its process; the
  tests of the features start a child process for theirs): segments, beam, closure, slowness grid, Capon spectra, kept
  elements, beam trace, element delays.  The ninth that names the communicator, the one of the further estimators, is
  reached through window ranges and through segments;
- "Capon spectra (nbls_set_capon) support up to 32 elements": the spectra need the geometry of the trace's array first,
  and ``nbls_set_geometry`` takes no array of 33 elements (528 pairs);
- "a MUSIC request (nbls_set_capon_music) needs at least 3 elements": likewise, no geometry has fewer than 3 elements.

The second part plans everything that can coexist and checks the one rule of the opt-in fetches: zeros until a pass of the
plan has run the stage that writes the result, afterwards what that pass left, whatever later passes run, and zeros again
after the next plan; the grid search of a plan with a lag seed belongs to the correlation stage."""
import numpy as np
import pytest

from narrow_band_least_squares_amd import _hip, planner, synthetic

pytestmark = pytest.mark.gpu

FS, NPTS, W, INC = 20.0, 256, 32, 16
VL = 14                                   # len(arange(0, NPTS - W, INC))
ARG, STATE, GEOMETRY, UNSUPPORTED = _hip.NBLS_ERR_ARG, _hip.NBLS_ERR_STATE, _hip.NBLS_ERR_GEOMETRY, _hip.NBLS_ERR_UNSUPPORTED
GRID = np.array([[sx, sy] for sx in (-0.3, 0.0, 0.3) for sy in (-0.3, 0.0, 0.3)])     # 3 x 3, s/km
CELLS = planner.grid_cells(GRID)[0]
HANN = planner.beam_trace_window(W)


def _trace(rows, seed=5):
    return np.random.default_rng(seed).standard_normal((rows, NPTS))


def _geometry(h, N, order=None):
    """The co-array of N elements; ``order``: a permutation of its pairs."""
    xij, pairs, xpinv = planner.co_array(synthetic.array_geometry(N, 1.0))
    p = np.arange(len(xij)) if order is None else np.asarray(order)
    h.set_geometry(xij[p], np.asarray(pairs)[p], xpinv[:, p])
    return xij


def _swapped(N, i, j):
    p = np.arange(N * (N - 1) // 2)
    p[[i, j]] = [j, i]
    return p


def _rig(h, rows=5, geometry=True, order=None, nseg=1):
    h.set_trace(_trace(rows), FS)
    if nseg > 1:
        h.set_segments(nseg)
    if geometry:
        _geometry(h, rows // nseg, order)


def _sub_estimator(N=5, kept=(0, 1, 2, 3)):
    xs, ps, xp = planner.co_array(synthetic.array_geometry(N, 1.0)[:, list(kept)])
    return [dict(kept=list(kept), xij=xs, pair_idx=ps, xpinv=xp, lts=None, eig6=None)]


def _capon(h, nbands=1, grid=GRID, ls=16, hs=4, loading=0.01, **kw):
    h.set_capon(grid, [2.0] * nbands, [ls] * nbands, [hs] * nbands, loading=loading, **kw)


def _plan(h, nbands=1, winlen=W, xcorr_impl=0, lts=None):
    sos = None if nbands == 1 else np.tile(np.array([1.0, 0, 0, 1, 0, 0]), (nbands, 1, 1))      # (the identity filter)
    h.plan(sos, False, None, None, [winlen] * nbands, [INC] * nbands, VL, lts=lts, xcorr_impl=xcorr_impl)


def _refused(h, **kw):
    """-> (code, message) of the plan's refusal."""
    try:
        _plan(h, **kw)
    except _hip.NblsError as e:
        code = e.code
    except ValueError as e:
        code = e.code
    except RuntimeError:
        code = GEOMETRY
    else:
        pytest.fail('the plan was not refused')
    return code, h.lib.nbls_last_error(h._h).decode()


# ---- the rows: (id, code, message, what to do to a fresh handle -> the plan's arguments) ----

def _segments_do_not_divide(h):
    _rig(h, rows=8, geometry=False)
    h.set_segments(3)


def _segments_with_window_ranges(h):
    _rig(h, rows=8, nseg=2)
    h.set_window_ranges([0], [5])


def _estimators_then_window_ranges(h):
    _rig(h)
    h.set_estimators(_sub_estimator())
    h.set_window_ranges([0], [5])


def _estimators_then_segments(h):
    _rig(h, rows=8, geometry=False)
    _geometry(h, 8)
    h.set_estimators(_sub_estimator(8))
    h.set_segments(2)


def _closure_out_of_order(h):
    _rig(h, order=_swapped(5, 8, 9))
    h.set_closure(True)


def _steering_alone(h):
    _rig(h)
    h.set_beam_interpolation(4)


def _grid_without_geometry(h):
    _rig(h, geometry=False)
    h.set_beam_grid(GRID)


def _grid_delay_too_long(h):
    _rig(h)
    h.set_beam_grid(np.array([[1e12, 0.0]]))


def _capon_without_geometry(h):
    _rig(h, geometry=False)
    _capon(h)


def _capon_band_count(h):
    _rig(h)
    _capon(h, nbands=1)
    return dict(nbands=2)


def _capon_snapshot_too_long(h):
    _rig(h)
    _capon(h, ls=33)


def _capon_singular(h):
    _rig(h)
    _capon(h, ls=32, hs=8, loading=0.0)


def _capon_steering_table(h):
    _rig(h)
    side = np.arange(256) * 1e-3
    _capon(h, nbands=205, grid=np.array([[a, b] for a in side for b in side]))          # 205 * 65536 * 5 * 16 bytes > 1 GiB
    return dict(nbands=205)


def _clean_without_capon(h):
    _rig(h)
    h.set_capon_clean(2)


def _music_without_capon(h):
    _rig(h)
    h.set_capon_music(sources=1)


def _music_with_estimators(h):
    _rig(h)
    _capon(h)
    h.set_capon_music(sources=1)
    h.set_estimators(_sub_estimator())


def _music_with_kept_capon(h):
    _rig(h)
    _capon(h)
    h.set_capon_music(sources=1)
    h.set_kept_elements(2, capon=True)


def _music_too_many_sources(h):
    _rig(h)
    _capon(h)
    h.set_capon_music(sources=5)


def _music_peaks_without_peaks(h):
    _rig(h)
    _capon(h)
    h.set_capon_music(sources=1, peaks=True)


def _peaks_without_capon(h):
    _rig(h)
    h.set_capon_peaks(CELLS, K=2)


def _peaks_cell_count(h):
    _rig(h)
    _capon(h, grid=GRID[:4])
    h.set_capon_peaks(CELLS, K=2)


def _peaks_route_does_not_fit(h):
    _rig(h)
    side = np.arange(100) * 1e-2
    grid = np.array([[a, b] for a in side for b in side])                               # 2 * 10000 * 8 bytes beside 11088: over 160 KiB
    _capon(h, grid=grid)
    h.set_capon_peaks(planner.grid_cells(grid)[0], K=2)
    h.set_option('capon_peak_route', 1)


def _kept_with_estimators(h):
    _rig(h)
    h.set_kept_elements(2)
    h.set_estimators(_sub_estimator())


def _kept_out_of_order(h):
    _rig(h, order=_swapped(5, 8, 9))
    h.set_kept_elements(2)


def _kept_min_pairs(h):
    _rig(h)
    h.set_kept_elements(5)


def _kept_beam_without_beam(h):
    _rig(h)
    h.set_kept_elements(2, beam=True)


def _kept_capon_without_capon(h):
    _rig(h)
    h.set_kept_elements(2, capon=True)


def _trace_with_window_ranges(h):
    _rig(h)
    h.set_beam_trace(HANN)
    h.set_window_ranges([0], [5])


def _trace_with_estimators(h):
    _rig(h)
    h.set_beam_trace(HANN)
    h.set_estimators(_sub_estimator())


def _trace_first_rows(h):
    _rig(h, order=_swapped(5, 0, 1))
    h.set_beam_trace(HANN)


def _trace_kept_without_kept(h):
    _rig(h)
    h.set_beam_trace(HANN, kept=True)


def _trace_window_count(h):
    _rig(h)
    h.set_beam_trace(HANN[:31])


def _trace_window_negative(h):
    _rig(h)
    w = np.tile(HANN, 2)
    w[W + 3] = -1.0
    h.set_beam_trace(w)
    return dict(nbands=2)


def _trace_window_zero(h):
    _rig(h)
    h.set_beam_trace(np.zeros(W))


def _delays_band_count(h):
    _rig(h)
    h.set_element_delays([3, 3])


def _delays_too_many_elements(h):
    _rig(h, rows=33, geometry=False)
    h.set_element_delays([3])


def _delays_with_estimators(h):
    _rig(h)
    h.set_element_delays([3])
    h.set_estimators(_sub_estimator())


def _delays_first_rows(h):
    _rig(h, order=_swapped(5, 0, 1))
    h.set_element_delays([3])


def _delays_kept_without_kept(h):
    _rig(h)
    h.set_element_delays([3], kept=True)


def _delays_staged_does_not_fit(h):
    _rig(h)
    assert h.lib.nbls_element_delay_lds_bytes(5, 8192, 3) == 0
    h.set_element_delays([3])
    h.set_option('element_delay_form', 1)
    return dict(winlen=8192)


def _limits_pair_count(h):
    _rig(h)
    h.set_lag_limits([5] * 9)


def _limits_forced_correlator(h):
    _rig(h)
    h.set_lag_limits([5] * 10)
    return dict(xcorr_impl=1)


def _seed_band_count(h):
    _rig(h)
    h.set_beam_grid(GRID)
    h.set_lag_seed([2, 2])


def _seed_without_grid(h):
    _rig(h)
    h.set_lag_seed([2])


def _seed_with_limits(h):
    _rig(h)
    h.set_beam_grid(GRID)
    h.set_lag_seed([2])
    h.set_lag_limits([5] * 10)


def _seed_forced_correlator(h):
    _rig(h)
    h.set_beam_grid(GRID)
    h.set_lag_seed([2])
    return dict(xcorr_impl=2)


# two faults each: the one that is tested first is the one reported
def _two_closure_before_kept(h):
    _rig(h, order=_swapped(5, 8, 9))
    h.set_closure(True)
    h.set_kept_elements(5)


def _two_clean_before_music(h):
    _rig(h)
    h.set_capon_clean(2)
    h.set_capon_music(sources=1)


def _two_kept_before_trace(h):
    _rig(h)
    h.set_kept_elements(2, beam=True)
    h.set_beam_trace(HANN[:31])


def _two_delays_before_limits(h):
    _rig(h)
    h.set_element_delays([3, 3])
    h.set_lag_limits([5] * 9)


def _two_steering_before_seed(h):
    _rig(h)
    h.set_beam_interpolation(4)
    h.set_lag_seed([2])


ROWS = [
    (_segments_do_not_divide, ARG, "nbls_plan: 8 trace rows do not divide into 3 segments"),
    (_segments_with_window_ranges, UNSUPPORTED, "nbls_plan: window ranges (nbls_set_window_ranges) are not supported with several segments"),
    (_estimators_then_window_ranges, UNSUPPORTED, "nbls_plan: further estimators (nbls_set_estimators) are not supported with several segments, window ranges or the RCCL gather"),
    (_estimators_then_segments, UNSUPPORTED, "nbls_plan: further estimators (nbls_set_estimators) are not supported with several segments, window ranges or the RCCL gather"),
    (_closure_out_of_order, STATE, "nbls_plan: closure results (nbls_set_closure) need the geometry of the trace's array, every pair in lexicographic order"),
    (_steering_alone, STATE, "nbls_plan: fractional-sample steering (nbls_set_beam_interpolation) needs beam results (nbls_set_beam) or a slowness grid (nbls_set_beam_grid)"),
    (_grid_without_geometry, STATE, "nbls_plan: the slowness-grid search (nbls_set_beam_grid) needs the geometry of the trace's array"),
    (_grid_delay_too_long, ARG, "nbls_plan: a delay of the slowness grid (nbls_set_beam_grid) reaches 2^30 samples"),
    (_capon_without_geometry, STATE, "nbls_plan: Capon spectra (nbls_set_capon) need the geometry of the trace's array"),
    (_capon_band_count, ARG, "nbls_plan: Capon tables (nbls_set_capon) of 1 bands for a plan of 2 bands"),
    (_capon_snapshot_too_long, ARG, "nbls_plan: the Capon snapshot of band 0 (33 samples) is longer than its window (32)"),
    (_capon_singular, ARG, "nbls_plan: band 0 has fewer Capon snapshots than elements and no loading: its matrix is singular by construction"),
    (_capon_steering_table, UNSUPPORTED, "nbls_plan: the Capon steering table (nbands * G * N * 16 bytes) exceeds 1 GiB"),
    (_clean_without_capon, STATE, "nbls_plan: a CLEAN request (nbls_set_capon_clean) needs Capon spectra (nbls_set_capon)"),
    (_music_without_capon, STATE, "nbls_plan: a MUSIC request (nbls_set_capon_music) needs Capon spectra (nbls_set_capon)"),
    (_music_with_estimators, UNSUPPORTED, "nbls_plan: a MUSIC request (nbls_set_capon_music) is not supported with further estimators (nbls_set_estimators)"),
    (_music_with_kept_capon, UNSUPPORTED, "nbls_plan: a MUSIC request (nbls_set_capon_music) is not supported with NBLS_KEPT_CAPON (nbls_set_kept_elements): it works on the full array"),
    (_music_too_many_sources, ARG, "nbls_plan: 5 sources (nbls_set_capon_music) for an array of 5 elements (1..4)"),
    (_music_peaks_without_peaks, STATE, "nbls_plan: NBLS_MUSIC_PEAKS (nbls_set_capon_music) needs K and the cells of a peak request (nbls_set_capon_peaks)"),
    (_peaks_without_capon, ARG, "nbls_plan: a peak request (nbls_set_capon_peaks) needs Capon spectra (nbls_set_capon)"),
    (_peaks_cell_count, ARG, "nbls_plan: the peak request (nbls_set_capon_peaks) has 9 cells for Capon spectra of 4 points"),
    (_peaks_route_does_not_fit, UNSUPPORTED, "nbls_plan: option capon_peak_route 1: the two maps of 10000 points do not fit the LDS of a workgroup beside the kernel's 11088 bytes"),
    (_kept_with_estimators, UNSUPPORTED, "nbls_plan: the kept elements (nbls_set_kept_elements) are not supported with further estimators (nbls_set_estimators)"),
    (_kept_out_of_order, STATE, "nbls_plan: the kept elements (nbls_set_kept_elements) need the geometry of the trace's array, every pair in lexicographic order"),
    (_kept_min_pairs, ARG, "nbls_plan: min_pairs (nbls_set_kept_elements) is 5 for an array of 5 elements (1..4, at most 32 elements)"),
    (_kept_beam_without_beam, STATE, "nbls_plan: NBLS_KEPT_BEAM (nbls_set_kept_elements) needs beam results (nbls_set_beam)"),
    (_kept_capon_without_capon, STATE, "nbls_plan: NBLS_KEPT_CAPON (nbls_set_kept_elements) needs Capon spectra (nbls_set_capon)"),
    (_trace_with_window_ranges, UNSUPPORTED, "nbls_plan: the beam trace (nbls_set_beam_trace) is not supported with window ranges (nbls_set_window_ranges): a slice of the windows does not cover the trace"),
    (_trace_with_estimators, UNSUPPORTED, "nbls_plan: the beam trace (nbls_set_beam_trace) is not supported with further estimators (nbls_set_estimators)"),
    (_trace_first_rows, STATE, "nbls_plan: the beam trace (nbls_set_beam_trace) needs the geometry of the trace's array, its first rows the pairs (0, m)"),
    (_trace_kept_without_kept, STATE, "nbls_plan: NBLS_BEAM_TRACE_KEPT (nbls_set_beam_trace) needs the kept elements (nbls_set_kept_elements)"),
    (_trace_window_count, ARG, "nbls_plan: a synthesis window table (nbls_set_beam_trace) of 31 entries for bands whose window lengths add up to 32"),
    (_trace_window_negative, ARG, "nbls_plan: the synthesis window (nbls_set_beam_trace) of band 1 has a negative or non-finite entry"),
    (_trace_window_zero, ARG, "nbls_plan: the synthesis window (nbls_set_beam_trace) of band 0 is all zero"),
    (_delays_band_count, ARG, "nbls_plan: 2 shift ranges (nbls_set_element_delays) for a plan of 1 bands"),
    (_delays_too_many_elements, ARG, "nbls_plan: the element delays (nbls_set_element_delays) take at most 32 elements, not 33"),
    (_delays_with_estimators, UNSUPPORTED, "nbls_plan: the element delays (nbls_set_element_delays) are not supported with further estimators (nbls_set_estimators)"),
    (_delays_first_rows, STATE, "nbls_plan: the element delays (nbls_set_element_delays) need the geometry of the trace's array, its first rows the pairs (0, m)"),
    (_delays_kept_without_kept, STATE, "nbls_plan: NBLS_ELEMENT_DELAY_KEPT (nbls_set_element_delays) needs the kept elements (nbls_set_kept_elements)"),
    (_delays_staged_does_not_fit, UNSUPPORTED, "nbls_plan: option element_delay_form 1: the rows of a band's windows do not fit the LDS of a workgroup"),
    (_limits_pair_count, ARG, "nbls_plan: 9 lag limits (nbls_set_lag_limits) for a geometry of 10 pairs"),
    (_limits_forced_correlator, UNSUPPORTED, "nbls_plan: lag limits (nbls_set_lag_limits) need xcorr_impl 0: the forced correlators search every lag"),
    (_seed_band_count, ARG, "nbls_plan: 2 seed half-widths (nbls_set_lag_seed) for a plan of 1 bands"),
    (_seed_without_grid, STATE, "nbls_plan: the lag seed (nbls_set_lag_seed) needs a slowness grid (nbls_set_beam_grid)"),
    (_seed_with_limits, UNSUPPORTED, "nbls_plan: the lag seed (nbls_set_lag_seed) is not supported together with lag limits (nbls_set_lag_limits): the grid's extent bounds the slowness, one restriction at a time"),
    (_seed_forced_correlator, UNSUPPORTED, "nbls_plan: the lag seed (nbls_set_lag_seed) needs xcorr_impl 0: the forced correlators search every lag"),
    (_two_closure_before_kept, STATE, "nbls_plan: closure results (nbls_set_closure) need the geometry of the trace's array, every pair in lexicographic order"),
    (_two_clean_before_music, STATE, "nbls_plan: a CLEAN request (nbls_set_capon_clean) needs Capon spectra (nbls_set_capon)"),
    (_two_kept_before_trace, STATE, "nbls_plan: NBLS_KEPT_BEAM (nbls_set_kept_elements) needs beam results (nbls_set_beam)"),
    (_two_delays_before_limits, ARG, "nbls_plan: 2 shift ranges (nbls_set_element_delays) for a plan of 1 bands"),
    (_two_steering_before_seed, STATE, "nbls_plan: fractional-sample steering (nbls_set_beam_interpolation) needs beam results (nbls_set_beam) or a slowness grid (nbls_set_beam_grid)"),
]


@pytest.mark.parametrize('arrange,code,message', ROWS, ids=[r[0].__name__.lstrip('_') for r in ROWS])
def test_refusal(arrange, code, message):
    h = _hip.Handle(0)
    try:
        got = _refused(h, **(arrange(h) or {}))
        assert got == (code, message)
    finally:
        h.close()


def test_the_table_is_complete():
    """45 of the 55 refusals of the stretch, the further estimators' through both of its two doors, and five plans with two faults."""
    single = [r for r in ROWS if not r[0].__name__.startswith('_two_')]
    assert len({r[2] for r in single}) == 45 and len(single) == 46 and len(ROWS) - len(single) >= 3


# ---- when the opt-in results are there ----

def _fetch_all(h, full):
    """Every opt-in result of the plan -> {name: array}."""
    out = {}
    out.update(zip(('grid_index', 'grid_fstat', 'grid_power'), h.fetch_beam_grid()))
    out['grid_map'] = h.fetch_beam_grid_map()
    out.update(zip(('beam_power', 'fstat'), h.fetch_beam()))
    if full:
        _fetch_rest(h, out)
    return {k: np.array(v) for k, v in out.items()}


def _fetch_rest(h, out):
    out.update(zip(('consistency', 'closure_max', 'element_consistency'), h.fetch_closure()))
    out.update(zip(('dropped_mask', 'kept_count'), h.fetch_kept_elements()))
    out.update(zip(('element_delay', 'element_cc', 'element_shift'), h.fetch_element_delays()))
    out['beam_trace'] = h.fetch_beam_trace(0)
    out.update(zip(('capon_index', 'capon_power', 'bartlett_index', 'bartlett_power'), h.fetch_capon()))
    out.update(zip(('capon_map', 'bartlett_map'), h.fetch_capon_maps()))
    out['capon_csdm'] = h.fetch_capon_csdm()
    for which in (0, 1):
        out.update(zip(('peak_count%d' % which, 'peak_index%d' % which, 'peak_power%d' % which, 'peak_offset%d' % which),
                       h.fetch_capon_peaks(which)))
    out.update(zip(('clean_count', 'clean_index', 'clean_power', 'clean_total', 'clean_residual'), h.fetch_capon_clean()))
    out.update(zip(('music_eigenvalues', 'music_sources', 'music_sweeps', 'music_index', 'music_power'), h.fetch_capon_music()))
    out['music_map'] = h.fetch_capon_music_map()
    out['music_vectors'] = h.fetch_capon_music_vectors()


def _all_zero(res):
    return not any(v.view(np.uint8).any() for v in res.values())


def test_results_are_there_once_their_stage_has_run():
    h = _hip.Handle(0)
    try:
        h.set_trace(_trace(5, seed=11), FS)
        xij = _geometry(h, 5)
        h.set_beam(True)
        h.set_closure(True)
        h.set_kept_elements(2, beam=True)
        h.set_element_delays([3])
        h.set_beam_trace(HANN)
        h.set_beam_grid(GRID, want_map=True)
        _capon(h, want_maps=True, want_csdm=True)
        h.set_capon_peaks(CELLS, K=2)
        h.set_capon_clean(2)
        h.set_capon_music(sources=1, maps=True, vectors=True)
        lts = planner.lts_plan(xij, 0.5)
        _plan(h, lts=lts)
        assert _all_zero(_fetch_all(h, True))                  # no pass yet
        h.execute(stages=3)
        assert _all_zero(_fetch_all(h, True))                  # 1. filter and correlation alone write none of them
        h.execute(stages=7)
        full = _fetch_all(h, True)                             # 2.
        for k in ('beam_power', 'kept_count', 'element_cc', 'beam_trace', 'grid_fstat', 'grid_map', 'capon_power', 'capon_map',
                  'capon_csdm', 'clean_total', 'music_eigenvalues', 'music_map', 'music_vectors'):
            assert full[k].view(np.uint8).any(), k
        h.execute(stages=3)
        again = _fetch_all(h, True)                            # 3. a pass without the solve stage leaves them as they are
        assert sorted(again) == sorted(full)
        for k, v in full.items():
            assert again[k].dtype == v.dtype and again[k].tobytes() == v.tobytes(), k
        _plan(h, lts=lts)
        assert _all_zero(_fetch_all(h, True))                  # 4. they were the last plan's
    finally:
        h.close()


def test_a_lag_seed_moves_the_grid_search_to_the_correlation_stage():
    h = _hip.Handle(0)
    try:
        h.set_trace(_trace(5, seed=12), FS)
        _geometry(h, 5)
        h.set_beam(True)
        h.set_beam_grid(GRID, want_map=True)
        h.set_lag_seed([4])
        _plan(h)
        assert _all_zero(_fetch_all(h, False))
        h.execute(stages=3)
        early = _fetch_all(h, False)
        assert early['grid_fstat'].any() and early['grid_map'].any()
        assert not early['beam_power'].any() and not early['fstat'].any()      # the beam grids are the solve stage's
        h.execute(stages=7)
        full = _fetch_all(h, False)
        for k in ('grid_index', 'grid_fstat', 'grid_power', 'grid_map'):
            assert early[k].tobytes() == full[k].tobytes(), k
        assert full['beam_power'].any()
    finally:
        h.close()
