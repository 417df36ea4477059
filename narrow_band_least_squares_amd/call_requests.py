"""The opt-in requests of one call of the host driver (``engine.py``), held the way the library holds a plan's
(``nbls_requests``): ONE record, ``Requests``, that ``process`` / ``process_batch`` / ``process_multi``
check once (``Requests.check``), hand down to ``launch`` — which sets and unsets them on the handle through
``Requests.applied`` — and that says which results a pass has (``RESULT_GROUPS``: one row per fetch, read by
``engine.new_result`` to allocate and by ``engine.fetch_groups`` to fetch and scatter).  Nothing here opens the GPU library.
"""
import collections
import contextlib
import inspect
import types

import numpy as np

from . import _hip, planner


# ---- what a pass can return ------------------------------------------------------------------------------------------
F8, I4, U4, C16 = np.float64, np.int32, np.uint32, np.complex128

# One fetch of a pass: ``applies(w)`` — w carries the keywords of ``engine.new_result`` (``Requests.wants``) —, the ``Handle``
# method, whether it takes an estimator index, whether it is called once per result row (rows (nbands, ...)) instead of once
# per pass (rows (nbands, vector_len, ...)), and per call its arguments and its fields in the order the method returns them
# (a method with one field returns the bare array).  A field is (name, trailing shape, dtype); N elements, P pairs, G grid
# points of the beam grid, R levels of its refinement, C of the Capon grid, K peaks, I CLEAN-SC iterations, T samples of the
# trace.
# ``sparse``: a result carries the fields only where the group applies (the others are None there).
Group = collections.namedtuple('Group', 'applies method est per_row calls sparse', defaults=(False,))


def _group(applies, method, *fields, est=False, per_row=False, args=((),), sparse=False):
    if len(args) == 1:
        fields = (fields,)
    return Group(applies, method, est, per_row, tuple(zip(args, fields)), sparse)


def _peaks(which):
    return tuple((which + f, t, d) for f, t, d in (('_peak_count', (), I4), ('_peak_index', ('K',), I4),
                                                   ('_peak_power', ('K',), F8), ('_peak_offset', ('K', 2), F8)))


# the planes of ``Handle.fetch(grids=False, want_<name>=True)``: one call for those a call wants
EXTRA_FIELDS = (('lag', ('P',), I4), ('cmax', ('P',), F8), ('z', (2,), F8))

RESULT_GROUPS = (
    _group(lambda w: w.want_uncert, 'fetch_uncertainty', ('vel_uncert', (), F8), ('baz_uncert', (), F8), est=True),
    _group(lambda w: w.want_beam, 'fetch_beam', ('beam_power', (), F8), ('fstat', (), F8), est=True),
    _group(lambda w: w.want_consistency, 'fetch_closure', ('consistency', (), F8), ('closure_max', (), F8),
           ('element_consistency', ('N',), F8), est=True),
    _group(lambda w: w.want_lag and w.want_subsample, 'fetch_lag_fraction', ('lag_frac', ('P',), F8), est=True),
    _group(lambda w: w.grid_points, 'fetch_beam_grid', ('grid_index', (), I4), ('grid_fstat', (), F8), ('grid_power', (), F8)),
    _group(lambda w: w.grid_points and w.want_grid_map, 'fetch_beam_grid_map', ('grid_map', ('G',), F8)),
    _group(lambda w: w.grid_points and w.grid_refine_levels, 'fetch_beam_grid_refined', ('grid_refined_slowness', (2,), F8),
           ('grid_refined_fstat', (), F8), ('grid_refined_power', (), F8), ('grid_refined_path', ('R',), I4),
           ('grid_refined_stencil', (9,), F8), sparse=True),
    _group(lambda w: w.capon_points, 'fetch_capon', ('capon_index', (), I4), ('capon_power', (), F8),
           ('bartlett_index', (), I4), ('bartlett_power', (), F8)),
    _group(lambda w: w.capon_points and w.want_capon_maps, 'fetch_capon_maps', ('capon_map', ('C',), F8),
           ('bartlett_map', ('C',), F8)),
    _group(lambda w: w.capon_points and w.want_capon_csdm, 'fetch_capon_csdm', ('capon_csdm', ('N', 'N'), C16)),
    _group(lambda w: w.capon_points and w.capon_peaks, 'fetch_capon_peaks', _peaks('capon'), _peaks('bartlett'),
           args=((0,), (1,))),
    _group(lambda w: w.capon_points and w.clean_iterations, 'fetch_capon_clean', ('clean_count', (), I4),
           ('clean_index', ('I',), I4), ('clean_power', ('I',), F8), ('clean_total', (), F8), ('clean_residual', (), F8)),
    _group(lambda w: w.capon_points and w.clean_iterations and w.want_clean_csdm, 'fetch_capon_clean_csdm',
           ('clean_csdm', ('N', 'N'), C16)),
    _group(lambda w: w.capon_points and w.want_music, 'fetch_capon_music', ('music_eigenvalues', ('N',), F8),
           ('music_sources', (), I4), ('music_sweeps', (), I4), ('music_index', (), I4), ('music_power', (), F8)),
    _group(lambda w: w.capon_points and w.want_music and w.want_music_maps, 'fetch_capon_music_map', ('music_map', ('C',), F8)),
    _group(lambda w: w.capon_points and w.want_music and w.want_music_vectors, 'fetch_capon_music_vectors',
           ('music_vectors', ('N', 'N'), C16)),
    _group(lambda w: w.capon_points and w.capon_peaks and w.want_music and w.want_music_peaks, 'fetch_capon_music_peaks',
           *_peaks('music')),
    _group(lambda w: w.want_kept, 'fetch_kept_elements', ('dropped_mask', (), U4), ('kept_count', (), I4)),
    _group(lambda w: w.want_element_delays, 'fetch_element_delays', ('element_delay', ('N',), F8), ('element_cc', ('N',), F8),
           ('element_shift', ('N',), I4)),
    _group(lambda w: w.beam_trace_npts, 'fetch_beam_trace', ('beam_trace', ('T',), F8), per_row=True),
)


def _names(method, call=0):
    return tuple(f[0] for g in RESULT_GROUPS if g.method == method for f in g.calls[call][1])


CLEAN_FIELDS = _names('fetch_capon_clean')                         # what ``Handle.fetch_capon_clean`` returns, in order
MUSIC_FIELDS = _names('fetch_capon_music')                         # what ``Handle.fetch_capon_music`` returns, in order
PEAK_FIELDS = tuple(n[len('capon'):] for n in _names('fetch_capon_peaks'))     # ... ``fetch_capon_peaks``, behind the spectrum's name


# ---- the checks of the raw keywords ----------------------------------------------------------------------------------
def _check_seed(seed_halfwidths, nbands, sgrid, min_velocity):
    """``seed_halfwidths`` -> int32 (nbands,) or None."""
    if seed_halfwidths is None:
        return None
    seeds = planner.check_seed_halfwidths(seed_halfwidths, nbands)
    if sgrid is None:
        raise ValueError('seed_halfwidths needs slowness_grid: the lag search is seeded by the grid maximum')
    if min_velocity is not None:
        raise ValueError('seed_halfwidths does not combine with min_velocity: the grid\'s own extent bounds the slowness, '
                         'one restriction of the lag search at a time')
    return seeds


def _check_grid_refine(grid_refine, sgrid, beam_taps, seeds):
    """``grid_refine`` — None, a number of levels or ``(levels, step)`` — -> the ``grid_refine`` tuple of the record or None
    (``planner.check_grid_refinement``)."""
    if grid_refine is None:
        return None
    args = tuple(grid_refine) if isinstance(grid_refine, (tuple, list)) else (grid_refine,)
    if not 1 <= len(args) <= 2:
        raise ValueError('grid_refine must be levels or (levels, step), not %r' % (grid_refine,))
    return planner.check_grid_refinement(args[0], args[1] if len(args) == 2 else None, sgrid, beam_taps, has_seed=seeds is not None)


def _check_capon(nchans, capon_grid, capon_freqs, capon_snapshots, capon_loading, want_capon_maps, want_capon_csdm, W,
                 capon_peaks=0, capon_peak_floor=0.25, capon_cells=None):
    """The Capon keywords -> the ``capon`` dict of the record or None (``planner.check_capon``, ``planner.check_capon_peaks``).
    ``W``: a function that returns the window length of every band."""
    wants_peaks = not (isinstance(capon_peaks, (int, np.integer)) and not isinstance(capon_peaks, (bool, np.bool_)) and capon_peaks == 0)
    if capon_grid is None:
        if capon_freqs is not None or capon_snapshots is not None or want_capon_maps or want_capon_csdm:
            raise ValueError('capon_freqs, capon_snapshots, want_capon_maps and want_capon_csdm need capon_grid')
        if wants_peaks or capon_cells is not None:
            raise ValueError('capon_peaks and capon_cells need capon_grid')
        return None
    W = W()                         # (ahead of the checks of the tables, which are checked against it)
    if capon_freqs is None or capon_snapshots is None:
        raise ValueError('capon_grid needs capon_freqs (planner.capon_frequencies) and capon_snapshots (planner.capon_snapshots)')
    g, f, ls, hs, delta = planner.check_capon(nchans, capon_grid, capon_freqs, capon_snapshots, capon_loading, W,
                                              want_capon_maps, want_capon_csdm)
    out = dict(grid=g, freqs=f, snap_len=ls, snap_hop=hs, loading=delta, want_maps=bool(want_capon_maps),
               want_csdm=bool(want_capon_csdm))
    if wants_peaks:
        cells, K, floor = planner.check_capon_peaks(len(g), planner.grid_cells(g)[0] if capon_cells is None else capon_cells,
                                                    capon_peaks, capon_peak_floor)
        out.update(peaks=K, peak_cells=cells, peak_floor=floor)
    elif capon_cells is not None:
        raise ValueError('capon_cells needs capon_peaks')
    return out


def _check_capon_clean(capon_clean, capon):
    """``capon_clean`` — None, an iteration count or ``(iterations[, gain[, floor[, residual]]])`` — -> the ``capon_clean`` tuple
    of the record or None (``planner.check_capon_clean``)."""
    if capon_clean is None:
        return None
    args = tuple(capon_clean) if isinstance(capon_clean, (tuple, list)) else (capon_clean,)
    if not 1 <= len(args) <= 4:
        raise ValueError('capon_clean must be (iterations[, gain[, floor[, residual]]]), not %r' % (capon_clean,))
    return planner.check_capon_clean(*args, has_capon=capon is not None)


def _check_capon_music(nchans, capon_music, capon, kept):
    """``capon_music`` — None, a number of sources or ``(sources[, eig_floor[, maps[, vectors[, peaks[, peak_floor]]]]])`` — -> the
    ``capon_music`` tuple of the record or None (``planner.check_capon_music``).  ``kept``: the checked ``kept`` tuple."""
    if capon_music is None:
        return None
    args = tuple(capon_music) if isinstance(capon_music, (tuple, list)) else (capon_music,)
    if not 1 <= len(args) <= 6:
        raise ValueError('capon_music must be (sources[, eig_floor[, maps[, vectors[, peaks[, peak_floor]]]]]), not %r' % (capon_music,))
    return planner.check_capon_music(nchans, *args, has_capon=capon is not None, has_peaks=capon is not None and bool(capon.get('peaks', 0)),
                                     kept_capon=kept is not None and bool(kept[2]))


def _check_kept(nchans, kept, want_beam, capon):
    """``kept`` — None or ``(min_pairs, beam, capon)`` — -> the ``kept`` tuple of the record or None (``planner.check_kept``, and
    a flag whose results the call does not ask for)."""
    if kept is None:
        return None
    try:
        q, kb, kc = kept
    except (TypeError, ValueError):
        raise ValueError('kept must be (min_pairs, beam, capon), not %r' % (kept,))
    q, kb, kc = planner.check_kept(nchans, q, kb, kc)
    if kb and not want_beam:
        raise ValueError('kept: the beam of the kept elements needs want_beam')
    if kc and capon is None:
        raise ValueError('kept: the Capon spectra of the kept elements need capon_grid')
    return q, kb, kc


def _check_element_delays(max_shift, delays_kept, nbands, nchans, kept):
    """``element_max_shift`` / ``element_delays_kept`` -> the int32 shift range of every band, or None
    (``planner.check_element_shifts``).  ``kept``: the call's checked ``kept`` tuple or None."""
    if not isinstance(delays_kept, (bool, np.bool_)):
        raise ValueError('element_delays_kept must be True or False, not %r' % (delays_kept,))
    if max_shift is None:
        if delays_kept:
            raise ValueError('element_delays_kept needs element_max_shift')
        return None
    shifts = planner.check_element_shifts(max_shift, nbands)
    if nchans > 32:
        raise ValueError('the element delays take at most 32 array elements, not %d' % nchans)
    if delays_kept and kept is None:
        raise ValueError('element_delays_kept: the beam of the kept elements needs a plan that names them (kept=, '
                         'planner.check_kept)')
    return shifts


def _check_beam_trace(want, W, kept, window_slice=None):
    """``want_beam_trace`` — None / False, True, a window kind or a dict of ``window``, ``mdccm_min``, ``kept`` — -> the
    ``beam_trace`` tuple of the record (one synthesis window per band, the gate, the kept flag) or None
    (``planner.check_beam_trace``).  ``W``: the window length of every band, or a function that returns it; ``kept``: the call's
    checked ``kept`` tuple or None."""
    if want is None or want is False:
        return None
    if callable(W):
        W = W()
    if want is True:
        want = {}
    elif isinstance(want, str):
        want = dict(window=want)
    if not isinstance(want, dict) or set(want) - {'window', 'mdccm_min', 'kept'}:
        raise ValueError('want_beam_trace must be True, a window kind or a dict of window, mdccm_min and kept, not %r' % (want,))
    table, gate, bt_kept = planner.check_beam_trace(np.asarray(W, dtype=np.int64), has_kept=kept is not None,
                                                    window_slice=window_slice, **want)
    cuts = np.cumsum(np.asarray(W, dtype=np.int64))[:-1]
    return list(np.split(table, cuts)), gate, bt_kept


def _check_families(families, window_slice=None):
    """``families`` — None or a dict of ``planner.check_families``' arguments — -> the checked request or None."""
    if families is None:
        return None
    if not isinstance(families, dict):
        raise ValueError('families must be a dict of mdccm_min, baz_tol, vel_tol, vel_min, vel_max [, sigma_tau_max, band_reach, '
                         'time_reach, min_pixels], not %r' % (families,))
    try:
        return planner.check_families(window_slice=window_slice, **families)
    except TypeError as e:
        raise ValueError('families: %s' % e)


# ---- how a request goes onto a handle and comes off it ---------------------------------------------------------------
# (attribute that is on, Handle setter, its arguments from the record, the arguments that switch it off, unset behind the
# others), in the order the setters are called; ``on``: None, False and 0 are off.
Step = collections.namedtuple('Step', 'on method set_args unset_args late')

STEPS = (
    Step('beam', 'set_beam', lambda r: (True,), (False,), False),
    Step('closure', 'set_closure', lambda r: (True,), (False,), False),
    Step('subsample', 'set_lag_refinement', lambda r: (True,), (False,), False),
    Step('lag_limits', 'set_lag_limits', lambda r: (r.lag_limits,), (None,), False),
    Step('beam_grid', 'set_beam_grid', lambda r: (r.beam_grid, r.beam_grid_map), (None,), False),
    Step('lag_seed', 'set_lag_seed', lambda r: (r.lag_seed,), (None,), False),
    Step('beam_taps', 'set_beam_interpolation', lambda r: (r.beam_taps,), (0,), False),
    Step('grid_refine', 'set_beam_grid_refinement', lambda r: tuple(r.grid_refine), (0, None), False),
    Step('kept', 'set_kept_elements', lambda r: tuple(r.kept), (0,), True),
    Step('element_delays', 'set_element_delays', lambda r: (r.element_delays, r.element_delays_kept), (None,), True),
    Step('beam_trace', 'set_beam_trace', lambda r: (np.concatenate(r.beam_trace[0]),
                                                    None if r.beam_trace[1] != r.beam_trace[1] else r.beam_trace[1],
                                                    r.beam_trace[2]), (None,), True),
    Step('capon', 'set_capon', lambda r: {k: v for k, v in r.capon.items() if not k.startswith('peak')}, (None,), False),
    Step('capon_peaks', 'set_capon_peaks', lambda r: (r.capon['peak_cells'], r.capon['peaks'], r.capon.get('peak_floor', 0.25)),
         (None,), False),
    Step('capon_clean', 'set_capon_clean', lambda r: tuple(r.capon_clean), (0,), False),
    Step('capon_music', 'set_capon_music', lambda r: tuple(r.capon_music), (None,), False),
    Step('families', 'set_families', lambda r: (_hip.family_params(**r.families),), (None,), False),
)

# Why the time-segmented path refuses a request: (keyword of ``process``, attribute of the record, is a flag — None, False
# and 0 are off; else only None is —, what that path does instead, what is not available there), in the order of precedence.
_ON_HOST = ', which keeps the filtered band on the host'
_BY_SLICE = ', which correlates the band slice by slice'
SEGMENTED_REFUSALS = (
    ('kept', 'kept', False, '', 'the kept elements are'),
    ('capon_grid', 'capon', False, _ON_HOST, 'the Capon spectra are'),
    ('element_max_shift', 'element_delays', False, _ON_HOST, 'the element delays are'),
    ('beam_taps', 'beam_taps', True, _ON_HOST, 'fractional-sample steering is'),
    ('want_beam_trace', 'beam_trace', False, _ON_HOST, 'the beam trace is'),
    ('want_consistency', 'closure', True, _BY_SLICE, 'closure results are'),
    ('seed_halfwidths', 'lag_seed', False, _ON_HOST, 'the seeded lag search is'),
    ('slowness_grid', 'beam_grid', False, _ON_HOST, 'the slowness-grid search is'),
    ('min_velocity', 'lag_limits', False, _BY_SLICE, 'the bounded lag search is'),
    ('want_subsample', 'subsample', True, _ON_HOST, 'sub-sample lag refinement is'),
    ('want_beam', 'beam', True, _ON_HOST, 'beam results are'),
)


def _cut(table, sel):
    if isinstance(table, list):                   # (the synthesis windows: one array per band)
        return table[sel] if isinstance(sel, slice) else [table[int(i)] for i in sel]
    return np.asarray(table)[sel]


class Requests:
    """The opt-in requests of one call, checked, in the form ``Handle``'s setters take them.  Every attribute is off by
    default (``DEFAULTS``); a request holds for the plans of this call only (``applied``).

    ``uncert``: the plan also computes ltsva's confidence intervals behind every solve (``Handle.set_uncertainty`` with
    ``planner.uncertainty_frame``).  ``beam``: beam power and F-statistic behind every solve (``Handle.set_beam``).
    ``subsample``: the picked lags are refined to sub-sample precision before the solve (``Handle.set_lag_refinement``).
    ``lag_limits``: the lag of pair k is searched only within ``|lag| <= lag_limits[k]`` samples (``Handle.set_lag_limits``,
    ``planner.lag_limits``).  ``beam_grid`` (G, 2): the beam F-statistic of the full array is searched over these slowness
    vectors, ``beam_grid_map``: and every F(g) kept (``Handle.set_beam_grid``).  ``lag_seed``: one half-width in samples per
    band: every pair's lag is searched only that near the delay the grid maximum predicts (``Handle.set_lag_seed``,
    ``planner.seed_halfwidths``; needs ``beam_grid``).  ``closure``: the closure of the picked lags behind every solve
    (``Handle.set_closure``).  ``capon``: a dict of ``Handle.set_capon``'s arguments, ``freqs`` / ``snap_len`` / ``snap_hop`` one
    per band: the Capon spectra of the bands; with ``peaks`` = K > 0 in it also their K strongest peaks on the lattice
    ``peak_cells`` above ``peak_floor`` (``Handle.set_capon_peaks``).  ``kept``: ``(min_pairs, beam, capon)`` of
    ``Handle.set_kept_elements``: the plan names the elements LTS dropped and forms its beam results / Capon spectra over the
    kept ones.  ``capon_clean``: ``(iterations, gain, floor, residual)`` of ``Handle.set_capon_clean``: every window's arrivals
    by CLEAN-SC (needs ``capon``).  ``capon_music``: ``(sources, eig_floor, maps, vectors, peaks, peak_floor)`` of
    ``Handle.set_capon_music``: every window's eigenvalues and MUSIC spectrum (needs ``capon``).  ``families``: the request dict
    of ``planner.check_families``: the cells of the pass's rows grouped into families behind its last solve
    (``Handle.set_families``) — only in a record whose pass covers every band of the call.  ``element_delays``: one shift range
    in samples per band: each element's delay against the beam of the others behind every solve, with
    ``element_delays_kept`` against the beam of the elements LTS kept, which needs ``kept`` (``Handle.set_element_delays``,
    ``planner.element_shifts``).  ``beam_trace``: ``(windows, mdccm_min, kept)`` — one synthesis window per band, the MdCCM gate
    (NaN: off) and the kept flag of ``Handle.set_beam_trace``: the beam trace of the pass's rows behind its last solve.
    ``beam_taps`` 4, 6 or 8: beam and slowness grid are steered at fractional-sample delays with that many Lagrange taps
    (``Handle.set_beam_interpolation``; needs ``beam`` or ``beam_grid``); 0: whole-sample delays.  ``grid_refine``: ``(levels,
    step)`` of ``Handle.set_beam_grid_refinement``: every window's grid maximum is refined between the grid points (needs
    ``beam_grid`` and ``beam_taps``; not with ``lag_seed``).  ``want_lag``, ``want_cmax``,
    ``want_z``: nothing for the plan; the call fetches these planes (``Handle.fetch``).

    The per-band tables (``lag_seed``, the three of ``capon``, the windows of ``beam_trace``, ``element_delays``) have one
    entry per band of whatever the record describes: ``check`` makes them for the bands of the call, ``for_bands`` cuts them
    to the bands of a plan."""

    DEFAULTS = dict(uncert=False, beam=False, subsample=False, lag_limits=None, beam_grid=None, beam_grid_map=False,
                    lag_seed=None, closure=False, capon=None, kept=None, capon_clean=None, capon_music=None, families=None,
                    element_delays=None, element_delays_kept=False, beam_trace=None, beam_taps=0, grid_refine=None,
                    want_lag=False, want_cmax=False, want_z=False)

    def __init__(self, **kw):
        unknown = set(kw) - set(self.DEFAULTS)
        if unknown:
            raise TypeError('Requests: unknown request %s' % ', '.join(sorted(unknown)))
        self.__dict__.update(self.DEFAULTS, **kw)

    def replace(self, **kw):
        return Requests(**dict(self.__dict__, **kw))

    @classmethod
    def check(cls, nchans, nbands, fs, W, window_slice=None, rij=None, xij=None, want_lag=False, want_cmax=False,
              want_z=False, want_uncert=False, want_beam=False, want_subsample=False, min_velocity=None, slowness_grid=None,
              want_grid_map=False, seed_halfwidths=None, want_consistency=False, capon_grid=None, capon_freqs=None,
              capon_snapshots=None, capon_loading=0.01, want_capon_maps=False, want_capon_csdm=False, capon_peaks=0,
              capon_peak_floor=0.25, capon_cells=None, kept=None, capon_clean=None, capon_music=None, families=None,
              grid_refine=None, element_max_shift=None, element_delays_kept=False, want_beam_trace=None, beam_taps=0):
        """The opt-in keywords of ``process`` / ``process_batch`` (``KEYWORDS``) -> the record; ``ValueError`` for whatever the
        library would refuse, before any GPU work.  ``nbands`` bands of ``nchans`` elements; ``W``: the window length of every
        band, or a function that returns it (called only for a request that is checked against it); ``window_slice`` of the
        call; ``xij`` the co-array or ``rij`` the geometry (``min_velocity`` reads it).  Every result is (nbands, vector_len)
        float64 unless stated.

        want_lag, want_cmax, want_z: also ``res.lag`` (.., P) int32, ``res.cmax`` (.., P), ``res.z`` (.., 2).
        want_uncert=True: also ``res.vel_uncert`` / ``res.baz_uncert``, the confidence intervals of the slowness estimate,
        computed on the GPU behind each unit's solve (``nbls_set_uncertainty``).
        want_beam=True: also ``res.beam_power`` / ``res.fstat``, power and Fisher F-statistic of the delay-and-sum beam at the
        solved slowness, computed on the GPU behind each unit's solve (``nbls_set_beam``).
        want_subsample=True: every picked lag is refined to sub-sample precision behind its verifier and the solve reads
        ``tau = (lag + frac) / fs`` (``nbls_set_lag_refinement``); with ``want_lag`` also ``res.lag_frac``
        (.., P) beside ``res.lag``.
        min_velocity (km/s): every pair's lag is searched only within the range a plane wave no slower than that can delay
        the pair (``planner.lag_limits``, ``nbls_set_lag_limits``); a finite real > 0.
        slowness_grid (G, 2) s/km: also ``res.grid_index`` (int32) / ``res.grid_fstat`` / ``res.grid_power``, per window the grid
        point at which the Fisher ratio of the full array's delay-and-sum beam is largest and the ratio and beam power
        there, searched on the GPU behind each unit's solve (``nbls_set_beam_grid``, DESIGN.md section 15;
        ``planner.check_slowness_grid``); want_grid_map=True: also ``res.grid_map`` (.., G), the ratio at every grid point.
        seed_halfwidths (samples; one integer or one per band; needs ``slowness_grid``): every pair's lag is searched only
        within that many samples of the delay the window's grid maximum predicts for the pair, and the grid search runs in
        the correlation stage, ahead of the lag pick (``planner.seed_halfwidths``, ``nbls_set_lag_seed``, DESIGN.md section 16;
        ``planner.check_seed_halfwidths``); it does not combine with ``min_velocity``.
        want_consistency=True: also ``res.consistency`` / ``res.closure_max`` and ``res.element_consistency`` (.., N), seconds:
        the rms and the largest closure ``l_ij + l_jk - l_ik`` of the picked lags over the element triplets of each window,
        and per element the rms over the triplets that hold it, computed on the GPU behind each unit's solve
        (``nbls_set_closure``); they follow whatever picks the call makes (refined, bounded, seeded).
        capon_grid (G, 2) s/km with capon_freqs (Hz per band, ``planner.capon_frequencies``) and capon_snapshots ((Ls, Hs) in
        samples, ``planner.capon_snapshots``): also ``res.capon_index`` / ``res.bartlett_index`` (int32) and ``res.capon_power`` /
        ``res.bartlett_power``, per window the maxima of the Capon (MVDR) and Bartlett slowness spectra of the band's
        cross-spectral matrix under the diagonal loading ``capon_loading``, computed on the GPU behind each unit's solve
        (``nbls_set_capon``; ``planner.check_capon``); want_capon_maps=True: also ``res.capon_map`` /
        ``res.bartlett_map`` (.., G); want_capon_csdm=True: also ``res.capon_csdm`` (.., N, N) complex.
        capon_peaks = K in 1..8 (needs ``capon_grid``): also ``res.capon_peak_count`` int32, ``res.capon_peak_index`` (.., K)
        int32, ``res.capon_peak_power`` (.., K) and ``res.capon_peak_offset`` (.., K, 2), and the same four with ``bartlett_``: per
        window the K strongest local maxima of either spectrum that reach ``capon_peak_floor`` times its maximum, with a
        sub-grid offset in lattice steps, picked on the GPU where the map is complete (``nbls_set_capon_peaks``, DESIGN.md
        section 19; ``planner.check_capon_peaks``).  ``capon_cells`` (G, 2) int: the lattice coordinates of the grid points, by
        default ``planner.grid_cells(capon_grid)[0]``.
        kept = (min_pairs, beam, capon): also ``res.dropped_mask`` uint32, bit m set where FAST-LTS has taken the weight of at
        least ``min_pairs`` (None: all N - 1) of element m's pairs in that window, and ``res.kept_count`` int32; with ``beam``
        (needs ``want_beam``) ``res.beam_power`` / ``res.fstat`` and with ``capon`` (needs ``capon_grid``) the spectra, their
        maxima, maps and peaks are those of the elements that are not dropped — the whole array where fewer than 3 would
        remain (``nbls_set_kept_elements``; ``planner.check_kept``).
        want_beam_trace = True, ``'hann'`` / ``'boxcar'`` or a dict of ``window``, ``mdccm_min``, ``kept``: also ``res.beam_trace``
        (nbands, npts), per band the delay-and-sum beam at every window's solved slowness, the overlapping windows stitched
        with the synthesis window; only windows with MdCCM >= ``mdccm_min`` enter, with ``kept`` (needs ``kept=``) each over
        the elements LTS kept in it (``nbls_set_beam_trace``; ``planner.check_beam_trace``).  Formed on
        the GPU behind the last solve of every pass, fetched per HBM round; not with a ``window_slice``.
        element_max_shift = K, one integer in 0..256 or one per band: also ``res.element_delay`` / ``res.element_cc`` /
        ``res.element_shift`` (.., N; the last int32): per window and element the delay in seconds, the normalised correlation
        and the whole-sample shift, within +-K samples of the delay the solved slowness predicts, at which the element
        correlates best with the sum of the other elements; with ``element_delays_kept`` (needs ``kept=``) with the sum of
        those LTS kept (``nbls_set_element_delays``; ``planner.element_shifts`` makes K).
        capon_clean = iterations or (iterations, gain, floor, residual) (needs ``capon_grid``): also ``res.clean_count`` int32,
        ``res.clean_index`` (.., I) int32, ``res.clean_power`` (.., I), ``res.clean_total`` and ``res.clean_residual``: per window
        the CLEAN-SC components of the band's cross-spectral matrix — the Bartlett maximum, ``gain`` of everything coherent
        with it removed, again on what is left, until a maximum falls below ``floor`` times the first — with the mean
        element power before and after; ``residual``: also ``res.clean_csdm`` (.., N, N) complex (``nbls_set_capon_clean``,
        DESIGN.md section 24; ``planner.check_capon_clean``).
        capon_music = sources or (sources, eig_floor, maps, vectors, peaks, peak_floor) (needs ``capon_grid``): also
        ``res.music_eigenvalues`` (.., N), the eigenvalues of every window's cross-spectral matrix in descending order,
        ``res.music_sources`` (the number M of signal eigenvectors: ``sources``, or with 0 the eigenvalues of at least
        ``eig_floor`` times the largest), ``res.music_sweeps`` (Jacobi sweeps), ``res.music_index`` (all three int32) and
        ``res.music_power``, the maximum of the MUSIC pseudo-spectrum over the grid; ``maps``: also ``res.music_map`` (.., G);
        ``vectors``: also ``res.music_vectors`` (.., N, N) complex; ``peaks`` (needs ``capon_peaks``): also
        ``res.music_peak_count`` / ``_index`` / ``_power`` / ``_offset``, the K strongest local maxima of the MUSIC spectrum as
        ``capon_peaks`` returns a spectrum's, kept from ``peak_floor`` times its maximum (``nbls_set_capon_music``, DESIGN.md
        section 25; ``planner.check_capon_music``); not with ``kept=(.., .., True)``.
        families = a dict of ``planner.check_families``' arguments: also ``res.family`` int32 and ``res.family_table`` (F, 8)
        int64, the cells grouped into families (``nbls_set_families``): labelled on the GPU behind the
        last solve where one pass covers every band, else by the same kernels on the assembled grids
        (``engine.label_result``) — the same arrays either way.
        beam_taps = 4, 6 or 8 (needs ``want_beam`` or ``slowness_grid``): beam and grid are steered at fractional-sample delays
        (``nbls_set_beam_interpolation``; ``planner.check_steering``).
        grid_refine = levels or (levels, step) (needs ``slowness_grid`` and ``beam_taps``; not with ``seed_halfwidths``): also
        ``res.grid_refined_slowness`` (.., 2) s/km, ``res.grid_refined_fstat``, ``res.grid_refined_power``,
        ``res.grid_refined_path`` (.., levels) int32 and ``res.grid_refined_stencil`` (.., 9): per window the grid maximum
        refined between the grid points — ``levels`` (1..12) times the best of the centre and its eight neighbours at
        ``step`` (h0, h1) s/km (default: the grid's lattice step) halved per level —, the Fisher ratio and beam power there,
        the candidate chosen on every level and the nine ratios of the last one; NaN and -1 where ``grid_index`` is -1
        (``nbls_set_beam_grid_refinement``; ``planner.check_grid_refinement``).  The coarse step must not
        exceed the width of the array's main lobe.

        The time-segmented path refuses every request but ``want_lag`` / ``want_cmax`` / ``want_z`` and ``families``
        (``segmented_refusal``)."""
        if not callable(W):
            table = W
            W = lambda: table
        limits = None
        if min_velocity is not None:
            limits = planner.lag_limits(planner.co_array(rij)[0] if xij is None else xij, fs, min_velocity)
        sgrid = None if slowness_grid is None else planner.check_slowness_grid(slowness_grid)
        seeds = _check_seed(seed_halfwidths, nbands, sgrid, min_velocity)
        capon = _check_capon(nchans, capon_grid, capon_freqs, capon_snapshots, capon_loading, want_capon_maps, want_capon_csdm,
                             W, capon_peaks, capon_peak_floor, capon_cells)
        planner.check_steering(beam_taps)
        if beam_taps and not want_beam and sgrid is None:
            raise ValueError('beam_taps: fractional-sample steering needs want_beam or slowness_grid')
        refine = _check_grid_refine(grid_refine, sgrid, beam_taps, seeds)
        kept = _check_kept(nchans, kept, want_beam, capon)
        clean = _check_capon_clean(capon_clean, capon)
        music = _check_capon_music(nchans, capon_music, capon, kept)
        fam = _check_families(families, window_slice)
        shifts = _check_element_delays(element_max_shift, element_delays_kept, nbands, nchans, kept)
        trace = _check_beam_trace(want_beam_trace, W, kept, window_slice)
        return cls(uncert=bool(want_uncert), beam=bool(want_beam), subsample=bool(want_subsample), lag_limits=limits,
                   beam_grid=sgrid, beam_grid_map=bool(want_grid_map), lag_seed=seeds, closure=bool(want_consistency),
                   capon=capon, kept=kept, capon_clean=clean, capon_music=music, families=fam, element_delays=shifts,
                   element_delays_kept=bool(element_delays_kept), beam_trace=trace, beam_taps=beam_taps,
                   grid_refine=refine,
                   want_lag=bool(want_lag), want_cmax=bool(want_cmax), want_z=bool(want_z))

    @classmethod
    def keywords_of(cls, namespace):
        """The opt-in keywords (``KEYWORDS``) a caller of ``check`` holds, e.g. in its ``locals()``."""
        return {k: namespace[k] for k in cls.KEYWORDS if k in namespace}

    def on(self, name, flag=True):
        """Whether request ``name`` is on: not None — and, for a ``flag``, neither False nor 0."""
        if name == 'capon_peaks':
            return self.capon is not None and bool(self.capon.get('peaks', 0))
        v = getattr(self, name)
        return v is not None and not (flag and isinstance(v, (bool, int, np.bool_, np.integer)) and not v)

    def for_bands(self, sel):
        """The record of a plan over the bands ``sel`` (a slice or an index array) of those this one describes: the per-band
        tables cut to them, everything else shared."""
        cut = {}
        if self.lag_seed is not None:
            cut['lag_seed'] = _cut(self.lag_seed, sel)
        if self.capon is not None:
            cut['capon'] = dict(self.capon, **{k: _cut(self.capon[k], sel) for k in ('freqs', 'snap_len', 'snap_hop')})
        if self.beam_trace is not None:
            cut['beam_trace'] = (_cut(self.beam_trace[0], sel),) + tuple(self.beam_trace[1:])
        if self.element_delays is not None:
            cut['element_delays'] = _cut(self.element_delays, sel)
        return self.replace(**cut) if cut else self

    @contextlib.contextmanager
    def applied(self, h, xij):
        """``with req.applied(h, xij): h.plan(...)``: the requests are on handle ``h`` inside the block and off it behind
        it, on every way out — a setter that refuses, a plan that does, success — for the handle is shared with calls that
        plan for themselves.  What this call did not set is not touched; ``Handle.set_uncertainty`` is called either way
        (the next call sets it again)."""
        h.set_uncertainty(planner.uncertainty_frame(xij) if self.uncert else None)
        done = []
        try:
            for step in STEPS:
                if self.on(step.on):
                    args = step.set_args(self)
                    if isinstance(args, dict):
                        getattr(h, step.method)(**args)
                    else:
                        getattr(h, step.method)(*args)
                    done.append(step)
            yield
        finally:
            for step in sorted(done, key=lambda s: s.late):        # (stable: in the order they were set, the late ones last)
                getattr(h, step.method)(*step.unset_args)

    def segmented_refusal(self, nchans, npts, keywords=None):
        """``ValueError`` for the first request that the time-segmented path of a trace of ``nchans`` x ``npts`` samples
        cannot serve (``SEGMENTED_REFUSALS``; ``keywords``: only those of them)."""
        for keyword, name, flag, why, what in SEGMENTED_REFUSALS:
            if (keywords is None or keyword in keywords) and self.on(name, flag):
                raise ValueError('%s: a trace of %d x %d samples takes the time-segmented path (not even one filtered band fits '
                                 'the HBM budget of a pass, NBLS_MAX_FILTERED_GB)%s: %s not available there'
                                 % (keyword, nchans, npts, why, what))

    def result_keywords(self, npts=0):
        """The keywords of ``engine.new_result`` for the results of a call with these requests on a trace of ``npts``
        samples."""
        capon, clean, music = self.capon or {}, self.capon_clean, self.capon_music or (0, 0, False, False, False)
        return dict(want_lag=self.want_lag, want_cmax=self.want_cmax, want_z=self.want_z, want_uncert=self.uncert,
                    want_beam=self.beam, want_subsample=self.subsample,
                    grid_points=0 if self.beam_grid is None else len(self.beam_grid), want_grid_map=self.beam_grid_map,
                    grid_refine_levels=0 if self.grid_refine is None else self.grid_refine[0],
                    want_consistency=self.closure, capon_points=len(capon.get('grid', ())),
                    want_capon_maps=capon.get('want_maps', False), want_capon_csdm=capon.get('want_csdm', False),
                    capon_peaks=capon.get('peaks', 0), want_kept=self.kept is not None,
                    beam_trace_npts=npts if self.beam_trace is not None else 0, want_element_delays=self.element_delays is not None,
                    clean_iterations=0 if clean is None else clean[0], want_clean_csdm=clean is not None and bool(clean[3]),
                    want_music=self.capon_music is not None, want_music_maps=bool(music[2]), want_music_vectors=bool(music[3]),
                    want_music_peaks=bool(music[4]))

    def wants(self):
        """``result_keywords`` as attributes: what the rows of ``RESULT_GROUPS`` ask (trace length 1: only whether there is a
        beam trace matters there)."""
        return types.SimpleNamespace(**self.result_keywords(1))


Requests.KEYWORDS = tuple(inspect.signature(Requests.check).parameters)[7:]      # the opt-in keywords, from want_lag on
