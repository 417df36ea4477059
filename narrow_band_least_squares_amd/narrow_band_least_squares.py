"""Drop-in mirror of the reference's ``narrow_band_least_squares.py``: same three functions,
same positional signatures and return tuples, but the (frequency band x time window) double
loop and the solver inside it run as ONE batched pass on the GPU.

Reference: narrow_band_least_squares.py:8-127 (serial), :134-218 (``narrow_band_loop``),
:223-323 (``..._parallel``, joblib over bands).  Here the "parallel" variant shards bands over
the GPUs of a node and collects the result blocks with one RCCL gather inside the library
(``dist.py``); with one GPU it equals the serial call.
"""
import functools
import os

import numpy as np
from scipy import signal

from . import dist, engine, planner
from .helpers import get_rij
from .lts_array import grid_slowness, _returns_capon, _peak_keywords, _returns_kept, _returns_clean, _returns_music, _check_flag, \
    _check_elements_strict, _check_clean_sources, _kept_request, refined_slowness


def _vector_len(WINLEN_list, WINOVER, st):
    """Result row length.  Reference: narrow_band_least_squares.py:41-47 (note: the hop is taken
    in SECONDS there, then divided by Fs — reproduced as is)."""
    max_WINLEN = WINLEN_list[-1]
    sampinc = int((1 - WINOVER) * max_WINLEN)
    npts = len(st[0].data)
    its = np.arange(0, npts, sampinc)
    nits = len(its) - 1
    Fs = st[0].stats.sampling_rate
    return int(nits / Fs)


def _band_edges(freqlist, FREQ_BAND_TYPE, bands):
    """narrow_band_least_squares.py:69-75."""
    step = 2 if FREQ_BAND_TYPE == '2_octave_over' else 1
    return [(freqlist[ii], freqlist[ii + step]) for ii in bands]


def _bt_caution(winlen, fmin, fmax):
    """narrow_band_least_squares.py:83-87."""
    temp_BT = winlen * (fmax - fmin)
    if temp_BT < 5.0:
        print('CAUTION: BT < 5! Band between ' + str(fmin) + ' Hz and ' + str(fmax) + ' Hz has BT = ' + str(temp_BT))


def _bt_cautions(winlens, edges):
    for winlen, (fmin, fmax) in zip(winlens, edges):
        _bt_caution(winlen, fmin, fmax)


def filter_responses(sos_list, freq_resp_list, fs):
    """``sosfreqz`` of every band (narrow_band_least_squares.py:78-80) -> (w rows, h rows), each (nbands, F) complex."""
    w_rows = np.zeros((len(sos_list), len(freq_resp_list)), dtype=complex)
    h_rows = np.zeros((len(sos_list), len(freq_resp_list)), dtype=complex)
    fast = planner.sosfreqz_bands(sos_list, freq_resp_list, fs)         # SciPy's values (bit for bit), all bands at once
    for n, sos in enumerate(sos_list):
        w_rows[n, :], h_rows[n, :] = signal.sosfreqz(sos, freq_resp_list, fs=fs) if fast is None else (fast[0], fast[1][n])
    return w_rows, h_rows


def _check_response_rows(w, h, freq_resp_list):
    if len(w) != len(freq_resp_list) or len(h) != len(freq_resp_list):
        raise ValueError('could not broadcast filter response of length %d into rows of length %d'
                         % (len(freq_resp_list), len(w)))


def _returns(ALPHA, vel, baz, mdccm, sigma_tau, t, stdict, nwin, w_array, h_array):
    """The reference's 9-tuple: OLS has no dictionary, LTS leaves ``sig_tau_array`` zero (calloc: no pages touched)."""
    if ALPHA == 1.0:
        stdict, sig_tau_array = None, sigma_tau
    else:
        sig_tau_array = np.zeros(sigma_tau.shape)
    return (vel, baz, mdccm, t, stdict, sig_tau_array, [int(n) for n in nwin], w_array, h_array)


def _band_prefix(band_number):
    """'<band:02d>_' as narrow_band_least_squares.py:114-124 builds it."""
    return str(band_number).zfill(2) + '_'


def _prefix_stdict(stdict, band_number):
    """Keys -> '<band:02d>_<key>', 'size' kept.  narrow_band_least_squares.py:114-124."""
    out = {}
    for key in stdict:
        if key != 'size':
            out[str(band_number).zfill(2) + '_' + key] = stdict[key]
        else:
            out[key] = stdict[key]
    return out


def _run_bands(bands, WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, freqlist, FREQ_BAND_TYPE,
               freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, vector_len, rij=None, want_keys=True,
               key_prefixes=None, want_beam=False, want_subsample=False, min_velocity=None, slowness_grid=None,
               want_grid_map=False, seed_period_fraction=None, want_consistency=False, beam_taps=0, keywords=None):
    """One device pass over the given band indices -> (BandBatch, w rows, h rows).

    Everything on the host that does not need a GPU result — the filter responses (``sosfreqz``,
    narrow_band_least_squares.py:78-80), the BT caution (:83-87) and the text of the ``stdict`` time
    keys — runs while the pass is in flight (``host_overlap`` of ``engine.process``).  The traces are
    uploaded row by row from the stream's own buffers.  ``keywords``: a function of (rij, fs, npts, edges, winlens,
    vector_len) that returns further keywords of ``engine.process`` — those of a feature that needs the call's own band edges
    or window lengths, as the Capon tables do."""
    rows, fs, t0 = engine.stream_rows(st)
    if rij is None:
        rij = get_rij(lat_list, lon_list, len(rows))
    edges = _band_edges(freqlist, FREQ_BAND_TYPE, bands)
    winlens = [WINLEN_list[ii] for ii in bands]
    out_rows = {}
    # the seeded lag search: half-widths from every band's upper edge (planner.seed_halfwidths)
    seeds = None if seed_period_fraction is None else planner.seed_halfwidths([e[1] for e in edges], fs, seed_period_fraction)

    def host_side(res):
        # (the two response arrays are made here, while the GPU works: 1.5 MB of fresh pages before the first launch
        #  were a tenth of a millisecond on the call's critical path)
        out_rows['w'], out_rows['h'] = filter_responses(res.sos, freq_resp_list, fs)
        _bt_cautions(winlens, edges)
        if ALPHA < 1.0 and want_keys:
            res.keys = engine.time_key_text(res.t, res.nwin, key_prefixes)
            res.stdict = engine.new_stdict(engine.n_keys(res.keys))
            res.pattern_cache = engine.new_pattern_cache()

    def group_done(res, b0, b1):
        # the dropped-element dictionary of the bands whose rows just landed, while later groups are still running
        if ALPHA < 1.0 and want_keys:
            engine.stdict_from_mask(res.mask[b0:b1], res.nwin[b0:b1], res.pair_idx, res.nchans, res.keys,
                                    into=res.stdict, k0=int(np.sum(res.nwin[:b0])), cache=res.pattern_cache)

    def units_done(res, u0, u1):
        # ... of the unit batch whose rows just landed (a streamed pass), while the GPU works on the next batch
        if ALPHA < 1.0 and want_keys:
            engine.stdict_from_mask(res.mask, res.nwin, res.pair_idx, res.nchans, res.keys, into=res.stdict,
                                    cache=res.pattern_cache, units=(u0, u1))

    res = engine.process(rows, fs, t0, rij, edges, winlens, WINOVER, ALPHA, FILTER_TYPE, FILTER_ORDER,
                         FILTER_RIPPLE, vector_len=vector_len, host_overlap=host_side, group_done=group_done,
                         units_done=units_done, want_beam=want_beam, want_subsample=want_subsample,
                         min_velocity=min_velocity, slowness_grid=slowness_grid, want_grid_map=want_grid_map,
                         seed_halfwidths=seeds, want_consistency=want_consistency, beam_taps=beam_taps,
                         **(keywords(rij, fs, len(rows[0]), edges, winlens, vector_len) if keywords is not None else {}))
    if ALPHA < 1.0 and want_keys and 'size' not in res.stdict:
        res.stdict['size'] = res.nchans            # (no band had a window: lts_array's dictionary still names the array size)
    if ALPHA < 1.0 and want_keys:
        # the helper objects of the dictionary (2*10^4 pattern records, 2.7 MB of key text at the benchmark's shape) are
        # taken apart by the NEXT call of this process behind its GPU pass, or at exit — not between the last row's
        # arrival and the return of this call
        engine.release_later(res.__dict__.pop('pattern_cache', None), res.__dict__.pop('keys', None))
    return res, out_rows['w'], out_rows['h']


def _check_alpha(ALPHA):
    if not (0.5 <= ALPHA <= 1.0):
        raise ValueError('ALPHA must be in [0.5, 1.0].')


def _all_bands(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist, FREQ_BAND_TYPE, freq_resp_list,
               FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij, tail=None, alpha_range=True, **requests):
    """The one body of the all-band single-stream entry points: the row length, the response rows, the range of ALPHA
    (``alpha_range``: the reference's own call has no such check), the pass over every band with the ``requests`` of
    ``_run_bands``, the reference's 9-tuple and behind it ``tail(res)``."""
    vector_len = _vector_len(WINLEN_list, WINOVER, st)
    _check_response_rows(w, h, freq_resp_list)
    if alpha_range:
        _check_alpha(ALPHA)
    bands = list(range(NBANDS))
    res, w_array, h_array = _run_bands(bands, WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, freqlist,
                                       FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER,
                                       FILTER_RIPPLE, vector_len, rij=rij,
                                       key_prefixes=[_band_prefix(ii + 1) for ii in bands], **requests)
    # (the dictionary was built group by group while the GPU was still working)
    out = _returns(ALPHA, res.vel, res.baz, res.mdccm, res.sigma_tau, res.t, getattr(res, 'stdict', None), res.nwin,
                   w_array, h_array)
    return out if tail is None else out + tail(res)


def _computed(res, rank=0):
    """Which cells of the (NBANDS, vector_len) result rows hold a window, with ``rank`` trailing axes of length 1."""
    computed = np.arange(res.vel.shape[1])[None, :] < np.asarray(res.nwin)[:, None]
    return computed.reshape(computed.shape + (1,) * rank)


def _zero_beyond(out, res, keys, rank=0):
    """The fields ``keys`` of the dict ``out`` — derived on the host, (NBANDS, vector_len) and ``rank`` trailing axes — zero
    beyond a band's windows, like ``vel_array``."""
    computed = _computed(res, rank)
    for k in keys:
        out[k] = np.where(computed, out[k], 0.0)


def _zero_spectra(out, res, names):
    """The derived slowness fields of the spectra ``names`` (``capon``, ``bartlett``, ``music``) in a dict of ``lts_array``'s:
    the maximum's and, where the pass kept peaks, every rank's; zero beyond a band's windows."""
    _zero_beyond(out, res, [n + k for n in names for k in ('_vel', '_baz')])
    peaks = [n for n in names if n + '_peak_vel' in out]
    _zero_beyond(out, res, [n + k for n in peaks for k in ('_peak_vel', '_peak_baz')], 1)
    _zero_beyond(out, res, [n + '_peak_slowness' for n in peaks], 2)
    return out


def _returns_grid(res, grid, grid_map):
    """The grid returns of ``narrow_band_least_squares_grid``: the slowness at the maximum (zero-padded like ``vel_array``),
    the three fields of the search and, when asked, the map."""
    computed = _computed(res)
    gvel, gbaz = (np.where(computed, a, 0.0) for a in grid_slowness(grid, res.grid_index))
    return (gvel, gbaz, res.grid_fstat, res.grid_power, res.grid_index) + ((res.grid_map,) if grid_map else ())


def narrow_band_least_squares(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist,
                              FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE,
                              rij=None):
    """Narrow-band least-squares / LTS array processing of every band in one GPU pass.

    Arguments and the 9-tuple ``(vel_array, baz_array, mdccm_array, t_array, stdict_all,
    sig_tau_array, num_compute_list, w_array, h_array)`` are those of the reference
    (narrow_band_least_squares.py:8-127).  Rows beyond ``num_compute_list[b]`` are zeros (the
    serial reference leaves them uninitialised, its parallel variant zero-fills).  ``ALPHA ==
    1.0`` fills ``sig_tau_array`` and returns ``stdict_all = None``; ``ALPHA < 1.0`` returns the
    merged dropped-element dictionary and leaves ``sig_tau_array`` zero, as the reference does.
    ``rij`` (2, N) km is an extension: it overrides the lat/lon geometry."""
    return _all_bands(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist, FREQ_BAND_TYPE, freq_resp_list,
                      FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij, alpha_range=False)


def narrow_band_least_squares_beam(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist,
                                   FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij=None):
    """``narrow_band_least_squares`` followed by ``beam_power_array`` and ``fstat_array``, each (NBANDS, vector_len) and
    zero-padded like ``vel_array``: per band and window the mean power of the delay-and-sum beam at the solved slowness
    and its Fisher F-statistic (``lts_array.ltsva_beam``), computed on the GPU behind each window's
    solve from the filtered band that is already there.  The first nine returns are those of
    ``narrow_band_least_squares``.  A trace so long that not one filtered band fits the HBM budget of a pass raises
    ``ValueError`` (the time-segmented path keeps the band on the host)."""
    return _all_bands(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist, FREQ_BAND_TYPE, freq_resp_list,
                      FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij, tail=lambda res: (res.beam_power, res.fstat), want_beam=True)


def narrow_band_least_squares_consistency(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist,
                                          FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij=None, *,
                                          subsample=False):
    """``narrow_band_least_squares`` followed by ``consistency_array`` and ``closure_max_array``, each (NBANDS, vector_len),
    and ``element_consistency_array`` (NBANDS, vector_len, N), zero-padded like ``vel_array``: per band and window the rms
    and the largest closure ``l_ij + l_jk - l_ik`` of the picked lags over the element triplets, in seconds, and per
    element the rms over the triplets that hold it (``lts_array.ltsva_consistency``), computed on the
    GPU behind each window's solve from the lag table that is already there.  ``subsample=True``: the lags are refined to
    sub-sample precision (``narrow_band_least_squares_subsample``) and the closure is that of the refined delays.  The first
    nine returns are those of ``narrow_band_least_squares`` (of ``narrow_band_least_squares_subsample`` with
    ``subsample=True``).  A ``subsample`` that is not a bool and fewer than 3 elements (4 under LTS) raise ``ValueError``
    before any GPU work, and so does a trace so long that not one filtered band fits the HBM budget of a pass."""
    _check_flag('subsample', subsample)
    _check_alpha(ALPHA)
    _check_elements_strict(len(st), ALPHA)
    return _all_bands(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist, FREQ_BAND_TYPE, freq_resp_list,
                      FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij, alpha_range=False,
                      tail=lambda res: (res.consistency, res.closure_max, res.element_consistency),
                      want_subsample=bool(subsample), want_consistency=True)


def narrow_band_least_squares_subsample(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist,
                                        FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij=None):
    """``narrow_band_least_squares`` on lags refined to sub-sample precision (``lts_array.ltsva_subsample``; DESIGN.md
    section 13): in every band each pair's picked lag gets the vertex offset of the parabola through its three nearest raw
    cross-correlation values, computed on the GPU behind the lag pick, and the slowness is fitted to the refined delays.
    Returns ``narrow_band_least_squares``'s nine values; ``t`` and the window counts are the same.  A trace so long that
    not one filtered band fits the HBM budget of a pass raises ``ValueError`` (the time-segmented path keeps the band on
    the host)."""
    return _all_bands(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist, FREQ_BAND_TYPE, freq_resp_list,
                      FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij, want_subsample=True)


def narrow_band_least_squares_bounded(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist,
                                      FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij=None, *,
                                      min_velocity):
    """``narrow_band_least_squares`` with every pair's lag searched only within its physical range
    (``lts_array.ltsva_bounded``): in every band ``|lag_k| <= ceil(fs |xij_k| / min_velocity) + 1``
    samples instead of all 2W-1 lags, on the GPU (csrc/xcorr_bounded.hip).  Returns ``narrow_band_least_squares``'s nine
    values; ``t`` and the window counts are the same.  ``min_velocity`` (km/s) must be a finite real > 0: ``ValueError``
    before any GPU work.  A trace so long that not one filtered band fits the HBM budget of a pass raises ``ValueError``
    (the time-segmented path correlates the band slice by slice)."""
    planner.check_min_velocity(min_velocity)
    return _all_bands(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist, FREQ_BAND_TYPE, freq_resp_list,
                      FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij, min_velocity=min_velocity)


def narrow_band_least_squares_grid(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist,
                                   FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij=None, *,
                                   slowness_grid, grid_map=False):
    """``narrow_band_least_squares`` followed by the slowness-grid search of the beam F-statistic in every band
    (``lts_array.ltsva_grid``): ``grid_vel_array``, ``grid_baz_array``, ``grid_fstat_array``,
    ``grid_power_array`` and ``grid_index_array`` (int32), each (NBANDS, vector_len) and zero-padded like ``vel_array``, and
    with ``grid_map=True`` the Fisher ratio at every grid point (NBANDS, vector_len, G).  Per band and window the
    delay-and-sum beam of the full array is steered over ``slowness_grid`` (G, 2) s/km on the GPU behind the window's
    solve, from the filtered band that is already there.  The first nine returns are those of
    ``narrow_band_least_squares``.  A bad grid raises ``ValueError`` before any GPU work, and so does a trace so long that
    not one filtered band fits the HBM budget of a pass (the time-segmented path keeps the band on the host)."""
    grid = planner.check_slowness_grid(slowness_grid)
    _check_flag('grid_map', grid_map)
    return _all_bands(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist, FREQ_BAND_TYPE, freq_resp_list,
                      FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij, tail=lambda res: _returns_grid(res, grid, grid_map), slowness_grid=grid,
                      want_grid_map=bool(grid_map))


def _returns_grid_refined(res):
    """The refined returns of ``narrow_band_least_squares_grid_refined``: the slowness at the refined maximum as velocity and
    back-azimuth (zero-padded like ``vel_array``) and the five fields of the refinement."""
    computed = _computed(res)
    rvel, rbaz = (np.where(computed, a, 0.0) for a in refined_slowness(res.grid_refined_slowness, res.grid_index))
    return (rvel, rbaz, res.grid_refined_slowness, res.grid_refined_fstat, res.grid_refined_power, res.grid_refined_path,
            res.grid_refined_stencil)


def narrow_band_least_squares_grid_refined(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist,
                                           FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij=None, *,
                                           slowness_grid, levels=4, step=None, taps=8, grid_map=False):
    """``narrow_band_least_squares_grid`` steered at fractional-sample delays (``taps`` 4, 6 or 8) with every window's grid
    maximum refined between the grid points (``lts_array.ltsva_grid_refined``): from the maximum,
    ``levels`` (1..12) times, the best of the centre and its eight neighbours at ``step`` (h0, h1) s/km halved per level —
    by default the lattice step of ``slowness_grid`` — becomes the new centre.  Returns
    ``narrow_band_least_squares_grid``'s tuple followed by ``refined_vel_array`` and ``refined_baz_array`` (zero-padded like
    ``vel_array``), ``refined_slowness_array`` (NBANDS, vector_len, 2), ``refined_fstat_array``, ``refined_power_array``,
    ``refined_path_array`` (NBANDS, vector_len, levels) int32 and ``refined_stencil_array`` (NBANDS, vector_len, 9).  The
    coarse step must not exceed the width of the array's main lobe.  Whatever the library would refuse raises ``ValueError``
    before any GPU work, and so does a trace so long that not one filtered band fits the HBM budget of a pass."""
    grid = planner.check_slowness_grid(slowness_grid)
    _check_flag('grid_map', grid_map)
    taps = planner.check_steering(taps)
    refine = planner.check_grid_refinement(levels, step, grid, taps)
    return _all_bands(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist, FREQ_BAND_TYPE, freq_resp_list,
                      FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij,
                      tail=lambda res: _returns_grid(res, grid, grid_map) + _returns_grid_refined(res), slowness_grid=grid,
                      want_grid_map=bool(grid_map), beam_taps=taps, keywords=lambda *_: dict(grid_refine=refine))


def narrow_band_least_squares_steered(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist,
                                      FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij=None, *,
                                      taps=8, slowness_grid=None, grid_map=False, subsample=False):
    """``narrow_band_least_squares_beam`` with the beam steered at fractional-sample delays (``lts_array.ltsva_steered``;
    DESIGN.md section 22): every element is read at ``fs xij . z`` itself through a Lagrange interpolator of ``taps`` (4, 6
    or 8) samples instead of at the nearest whole sample; ``planner.steering_error(taps, f / fs)`` is the interpolator's
    worst-case error in a band at f.  With ``slowness_grid`` (G, 2) s/km the five (with ``grid_map=True`` six) grid returns
    of ``narrow_band_least_squares_grid`` follow, the grid steered the same way; ``subsample=True`` fits the slowness to the
    refined lags (``narrow_band_least_squares_subsample``), so that the beam is steered by a continuous estimate.  Returns
    ``narrow_band_least_squares_beam``'s 11-tuple, then the grid returns.  Bad ``taps``, grid or flags raise ``ValueError``
    before any GPU work, and so does a trace so long that not one filtered band fits the HBM budget of a pass."""
    taps = planner.check_steering(taps)
    grid = None if slowness_grid is None else planner.check_slowness_grid(slowness_grid)
    _check_flag('grid_map', grid_map)
    _check_flag('subsample', subsample)
    if grid_map and grid is None:
        raise ValueError('grid_map needs slowness_grid')

    def tail(res):
        return (res.beam_power, res.fstat) + (() if grid is None else _returns_grid(res, grid, grid_map))
    return _all_bands(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist, FREQ_BAND_TYPE, freq_resp_list,
                      FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij, tail=tail, want_beam=True, want_subsample=bool(subsample),
                      slowness_grid=grid, want_grid_map=bool(grid_map), beam_taps=taps)


def narrow_band_least_squares_capon(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist,
                                    FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij=None, *,
                                    slowness_grid, capon_freqs=None, snapshots=None, loading=0.01, maps=False, peaks=0,
                                    peak_floor=0.25):
    """``narrow_band_least_squares`` followed by the Capon (MVDR) and Bartlett slowness spectra of every band's
    cross-spectral matrix (``lts_array.ltsva_capon``), computed on the GPU behind each window's solve
    from the filtered band that is already there.  ``capon_freqs`` (Hz per band) defaults to
    ``planner.capon_frequencies`` of the call's bands, ``snapshots`` ((Ls, Hs) in samples) to ``planner.capon_snapshots``.
    Returns the nine values of ``narrow_band_least_squares`` followed by one dict: ``capon_index`` / ``bartlett_index``
    (int32), ``capon_power`` / ``bartlett_power``, ``capon_vel`` / ``capon_baz`` / ``bartlett_vel`` / ``bartlett_baz``
    (``lts_array.grid_slowness`` at the indices), each (NBANDS, vector_len) with zeros beyond a band's windows, and with
    ``maps=True`` ``capon_map`` / ``bartlett_map`` (NBANDS, vector_len, G).  With ``peaks=K`` also the peak fields of
    ``lts_array.ltsva_capon``, (NBANDS, vector_len, ...) with zeros beyond a band's windows.  Whatever the library would refuse raises
    ``ValueError`` before any GPU work, and so does a trace so long that not one filtered band fits the HBM budget of a
    pass."""
    grid = planner.check_slowness_grid(slowness_grid)
    _check_flag('maps', maps)
    peak_kw = _peak_keywords(grid, peaks, peak_floor)
    return _all_bands(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist, FREQ_BAND_TYPE, freq_resp_list,
                      FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij,
                      tail=lambda res: (_zero_spectra(_returns_capon(res, grid, bool(maps), band=None), res, ('capon', 'bartlett')),),
                      keywords=_capon_band_keywords(len(st), grid, capon_freqs, snapshots, loading, maps, peak_kw, WINOVER))


def narrow_band_least_squares_clean(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist,
                                    FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij=None, *,
                                    slowness_grid, capon_freqs=None, snapshots=None, iterations=16, gain=0.5, floor=0.02,
                                    merge_radius=None, max_sources=4):
    """``narrow_band_least_squares`` followed by every window's arrivals and their powers by CLEAN-SC on the band's
    cross-spectral matrix (``lts_array.ltsva_clean``), computed on the GPU behind each window's solve.
    ``capon_freqs`` and ``snapshots`` as for ``narrow_band_least_squares_capon``.  Returns the nine values of
    ``narrow_band_least_squares`` followed by one dict with the fields of ``lts_array.ltsva_clean``'s, each (NBANDS, vector_len,
    ...) with zeros beyond a band's windows.  Whatever the library would refuse raises ``ValueError`` before any GPU work."""
    grid = planner.check_slowness_grid(slowness_grid)
    clean = planner.check_capon_clean(iterations, gain, floor, False)
    radius, max_sources = _check_clean_sources(grid, merge_radius, max_sources)

    def tail(res):
        out = _returns_clean(res, grid, radius, max_sources, band=None)
        _zero_beyond(out, res, ('clean_vel', 'clean_baz', 'source_power', 'source_vel', 'source_baz'), 1)
        _zero_beyond(out, res, ('source_slowness',), 2)
        return (out,)
    return _all_bands(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist, FREQ_BAND_TYPE, freq_resp_list,
                      FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij, tail=tail,
                      keywords=_capon_band_keywords(len(st), grid, capon_freqs, snapshots, 0.01, False, dict(capon_clean=clean), WINOVER))


def narrow_band_least_squares_music(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist,
                                    FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij=None, *,
                                    slowness_grid, capon_freqs=None, snapshots=None, sources=0, eig_floor=0.05, maps=False,
                                    vectors=False, peaks=0, peak_floor=0.0):
    """``narrow_band_least_squares`` followed by the eigenvalues of every window's cross-spectral matrix and its MUSIC
    pseudo-spectrum (``lts_array.ltsva_music``), computed on the GPU behind each window's solve.
    ``capon_freqs`` and ``snapshots`` as for ``narrow_band_least_squares_capon``.  Returns the nine values of
    ``narrow_band_least_squares`` followed by one dict with the fields of ``lts_array.ltsva_music``'s, each (NBANDS, vector_len,
    ...) with zeros beyond a band's windows.  Whatever the library would refuse raises ``ValueError`` before any GPU work."""
    grid = planner.check_slowness_grid(slowness_grid)
    peak_kw = _peak_keywords(grid, peaks, 0.25)
    music = planner.check_capon_music(len(st), sources, eig_floor, maps, vectors, bool(peak_kw), peak_floor)
    return _all_bands(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist, FREQ_BAND_TYPE, freq_resp_list,
                      FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij,
                      tail=lambda res: (_zero_spectra(_returns_music(res, grid, band=None), res, ('music',)),),
                      keywords=_capon_band_keywords(len(st), grid, capon_freqs, snapshots, 0.01, False,
                                                    dict(peak_kw, capon_music=music), WINOVER))


def _capon_band_keywords(nchans, grid, capon_freqs, snapshots, loading, maps, peak_kw, WINOVER):
    """The ``keywords`` callable of ``_run_bands`` behind the Capon arguments of a narrow-band call: the Capon keywords of
    ``engine.process`` for the call's bands, their frequencies and snapshots defaulted and checked."""
    def keywords(rij_used, fs, npts, edges, winlens, vector_len):
        W = engine.plan_windows(npts, fs, winlens, WINOVER, vector_len)[0]
        f = planner.capon_frequencies(edges) if capon_freqs is None else capon_freqs
        snaps = snapshots
        if snaps is None:
            f = planner.check_capon(nchans, grid, f, (1, 1), loading, W)[1]
            snaps = planner.capon_snapshots(planner.co_array(rij_used)[0], grid, fs, f, W)
        planner.check_capon(nchans, grid, f, snaps, loading, W, bool(maps))
        return dict(capon_grid=grid, capon_freqs=f, capon_snapshots=snaps, capon_loading=loading, want_capon_maps=bool(maps),
                    **peak_kw)
    return keywords


def narrow_band_least_squares_kept(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist,
                                   FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij=None, *,
                                   min_pairs=None, beam=True, slowness_grid=None, capon_freqs=None, snapshots=None,
                                   loading=0.01, maps=False, peaks=0, peak_floor=0.25):
    """``narrow_band_least_squares`` followed by the results of the elements FAST-LTS kept in every band and window
    (``lts_array.ltsva_kept``): an element at least ``min_pairs`` of whose N - 1 pairs have lost their
    weight (default: all of them) counts as dropped, and the beam of ``narrow_band_least_squares_beam`` (``beam=True``) and,
    with ``slowness_grid``, the spectra of ``narrow_band_least_squares_capon`` (its keywords) are formed over the other
    elements.  Returns the nine values of ``narrow_band_least_squares`` followed by one dict: ``dropped_elements`` (NBANDS,
    vector_len, N) bool, ``kept_count`` (NBANDS, vector_len) int32, with ``beam`` ``beam_power`` / ``fstat``, with the grid
    the fields of ``narrow_band_least_squares_capon``'s dict; zeros beyond a band's windows.  Whatever the library would
    refuse raises ``ValueError`` before any GPU work, and so does a trace so long that not one filtered band fits the HBM
    budget of a pass."""
    grid = None if slowness_grid is None else planner.check_slowness_grid(slowness_grid)
    if grid is None and (capon_freqs is not None or snapshots is not None or maps or peaks):
        raise ValueError('capon_freqs, snapshots, maps and peaks need slowness_grid')
    _check_flag('maps', maps)
    _check_alpha(ALPHA)
    _check_elements_strict(len(st), ALPHA)
    kept = planner.check_kept(len(st), min_pairs, beam, grid is not None)
    peak_kw = {} if grid is None else _peak_keywords(grid, peaks, peak_floor)
    capon_kw = None if grid is None else _capon_band_keywords(len(st), grid, capon_freqs, snapshots, loading, maps, peak_kw, WINOVER)

    def keywords(*args):           # (the keywords that ride beside the Capon ones into ``engine.process``)
        return dict({} if capon_kw is None else capon_kw(*args), kept=kept)

    def tail(res):
        out = _returns_kept(res, len(st), kept[1], None, band=None)
        if grid is not None:
            out.update(_zero_spectra(_returns_capon(res, grid, bool(maps), band=None), res, ('capon', 'bartlett')))
        return (out,)
    return _all_bands(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist, FREQ_BAND_TYPE, freq_resp_list,
                      FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij, tail=tail, alpha_range=False, want_beam=kept[1],
                      keywords=keywords)


def narrow_band_least_squares_seeded(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist,
                                     FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij=None, *,
                                     slowness_grid, period_fraction=0.5, grid_map=False):
    """``narrow_band_least_squares_grid`` whose lag picks are seeded by the grid maximum (``lts_array.ltsva_seeded``;
    DESIGN.md section 16): in every band and window the whole-array beam steered over ``slowness_grid`` chooses the cycle,
    every pair's lag is searched only within ``K_b = max(1, floor(period_fraction fs / fmax_b))`` samples of the delay that
    grid point predicts for the pair (``planner.seed_halfwidths``: by default half a period of the band's upper edge), and
    the solve runs on those picks, on the GPU (csrc/xcorr_seeded.hip).  Returns ``narrow_band_least_squares_grid``'s tuple;
    ``t``, the window counts and the grid returns are the same.  A bad grid or ``period_fraction`` raises ``ValueError``
    before any GPU work, and so does a trace so long that not one filtered band fits the HBM budget of a pass."""
    grid = planner.check_slowness_grid(slowness_grid)
    planner.seed_halfwidths([1.0], 1.0, period_fraction)         # (the check of period_fraction, before any GPU work)
    _check_flag('grid_map', grid_map)
    return _all_bands(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist, FREQ_BAND_TYPE, freq_resp_list,
                      FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij, tail=lambda res: _returns_grid(res, grid, grid_map),
                      slowness_grid=grid, want_grid_map=bool(grid_map), seed_period_fraction=period_fraction)


def narrow_band_least_squares_batch(WINLEN_list, WINOVER, ALPHA, streams, lat_list, lon_list, NBANDS, w, h, freqlist,
                                    FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij=None):
    """``narrow_band_least_squares`` over several recordings of ONE array in one GPU pass -> a list of 9-tuples,
    element i equal to ``narrow_band_least_squares(..., streams[i], ...)``.

    Every stream must have the same element count, trace length and sampling rate, and all share the geometry
    (``lat_list`` / ``lon_list`` or ``rij``); ``ValueError`` names a mismatch before any GPU work.  The S*N rows go up
    from the streams' own buffers.  Window times come from each stream's own start time, the dictionary is per
    recording; ``w_array`` / ``h_array`` are equal for all recordings (separate copies).  The BT caution prints once
    per batch.  An empty sequence gives ``[]``."""
    return _all_bands_batch(narrow_band_least_squares, WINLEN_list, WINOVER, ALPHA, streams, lat_list, lon_list, NBANDS, w, h, freqlist,
                            FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij)


def _all_bands_batch(single, WINLEN_list, WINOVER, ALPHA, streams, lat_list, lon_list, NBANDS, w, h, freqlist, FREQ_BAND_TYPE,
                     freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij, params=None, tail=None, **requests):
    """The one body of the ``_batch`` entry points: ``single`` with its keywords ``params`` for a batch of one recording, else
    one pass over every band of every recording with the ``requests`` of ``engine.process_batch`` and, per recording, the
    reference's 9-tuple and behind it ``tail(res, edges, fs, t0)``."""
    streams = list(streams)
    if not streams:
        return []
    recs, fs, t0s = engine.batch_rows(streams)
    if len(streams) == 1:          # a batch of one IS the single call (which overlaps its upload with the plan)
        return [single(WINLEN_list, WINOVER, ALPHA, streams[0], lat_list, lon_list, NBANDS, w, h, freqlist, FREQ_BAND_TYPE,
                       freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij=rij, **(params or {}))]
    vector_len = _vector_len(WINLEN_list, WINOVER, streams[0])
    _check_response_rows(w, h, freq_resp_list)
    nchans = len(recs[0])
    if rij is None:
        rij = get_rij(lat_list, lon_list, nchans)
    bands = list(range(NBANDS))
    edges = _band_edges(freqlist, FREQ_BAND_TYPE, bands)
    winlens = [WINLEN_list[ii] for ii in bands]
    results = engine.process_batch(recs, fs, t0s, rij, edges, winlens, WINOVER, ALPHA, FILTER_TYPE, FILTER_ORDER,
                                   FILTER_RIPPLE, vector_len=vector_len, **requests)
    w_rows, h_rows = filter_responses(results[0].sos, freq_resp_list, fs)
    _bt_cautions(winlens, edges)
    prefixes = [_band_prefix(ii + 1) for ii in bands]
    out = []
    for res, t0 in zip(results, t0s):
        stdict_all = None
        if ALPHA != 1.0:
            keys = engine.time_key_text(res.t, res.nwin, prefixes)
            stdict_all = engine.stdict_from_mask(res.mask, res.nwin, res.pair_idx, res.nchans, keys)
        out.append(_returns(ALPHA, res.vel, res.baz, res.mdccm, res.sigma_tau, res.t, stdict_all, res.nwin,
                            w_rows.copy(), h_rows.copy()) + (() if tail is None else tail(res, edges, fs, t0)))
    return out


def _reduced(st, lat_list, lon_list, rij, remove):
    """The stream, coordinates and geometry of the array without the traces in ``remove`` — what a single call on the
    reduced stream is given: ``rij[:, kept]`` as it stands, else ``get_rij`` of the reduced lists (whose origin is the
    reduced list's first element)."""
    nchans = len(st)
    if not remove:
        return st, lat_list, lon_list, (get_rij(lat_list, lon_list, nchans) if rij is None else rij)
    kept = engine.kept_elements(nchans, remove)
    sub = [st[i] for i in kept]
    lat = None if lat_list is None else [lat_list[i] for i in kept]
    lon = None if lon_list is None else [lon_list[i] for i in kept]
    if rij is not None:
        return sub, lat, lon, np.ascontiguousarray(np.asarray(rij)[:, kept])
    return sub, lat, lon, get_rij(lat, lon, len(kept))


def narrow_band_least_squares_multi(WINLEN_list, WINOVER, ESTIMATORS, st, lat_list, lon_list, NBANDS, w, h, freqlist,
                                    FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij=None):
    """``narrow_band_least_squares`` for several estimators in one GPU pass -> a list of 9-tuples.

    ``ESTIMATORS``: a sequence of ``(ALPHA, remove)``, ``remove`` a tuple of ascending 0-based trace indices of ``st``
    the estimator leaves out (a bare number means ``(ALPHA, ())``); at most 8.  Element e of the result equals
    ``narrow_band_least_squares(..., ALPHA_e, st without remove_e, ...)`` — with ``rij[:, kept]``, or the reduced
    ``lat_list`` / ``lon_list`` — : the dictionary's element numbers and ``'size'`` are the reduced array's, OLS estimators
    return ``stdict_all = None`` and fill ``sig_tau_array``.  The full array is filtered and correlated ONCE (a pair's lag
    does not depend on ALPHA or on the other elements); only the solve runs per estimator.  ``ValueError`` before any GPU
    work for an empty list, a bad ALPHA or ``remove`` and too few kept elements.  The BT caution prints once per call.
    One estimator that removes nothing is the single call.  A trace of which not even one filtered band fits the HBM
    budget runs as one single call per estimator."""
    rows, fs, _ = engine.stream_rows(st)
    nchans = len(rows)
    ests = engine.normalize_estimators(ESTIMATORS, nchans)
    single = functools.partial(narrow_band_least_squares, WINLEN_list, WINOVER)
    tail = (NBANDS, w, h, freqlist, FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE)
    if len(ests) == 1 and not ests[0][1]:
        return [single(ests[0][0], st, lat_list, lon_list, *tail, rij=rij)]
    reduced = [_reduced(st, lat_list, lon_list, rij, rm) for _, rm in ests]
    if engine.max_bands_per_pass(nchans, len(rows[0])) < 1:        # the time-segmented path: one single call per estimator
        return [single(a, sub, lat, lon, *tail, rij=r) for (a, _), (sub, lat, lon, r) in zip(ests, reduced)]
    vector_len = _vector_len(WINLEN_list, WINOVER, st)
    _check_response_rows(w, h, freq_resp_list)
    bands = list(range(NBANDS))
    edges = _band_edges(freqlist, FREQ_BAND_TYPE, bands)
    winlens = [WINLEN_list[ii] for ii in bands]
    prefixes = [_band_prefix(ii + 1) for ii in bands]
    rijs = [r for _, _, _, r in reduced]
    t0s = [engine.stream_rows(sub[:1])[2] for sub, _, _, _ in reduced]
    if all(rm for _, rm in ests):
        rijs.append(get_rij(lat_list, lon_list, nchans) if rij is None else rij)
    shared = {}

    def host_side(results):
        if len(results[0].sos) == NBANDS:      # (bands in several HBM rounds: their designs are complete only at the end)
            shared['w'], shared['h'] = filter_responses(results[0].sos, freq_resp_list, fs)
        _bt_cautions(winlens, edges)
        keys, cache = {}, engine.new_pattern_cache
        for res in results:
            if res.lts:                    # (the key text depends on the window times alone: once per start time)
                if id(res.t) not in keys:
                    keys[id(res.t)] = engine.time_key_text(res.t, res.nwin, prefixes)
                res.keys = keys[id(res.t)]
                res.stdict = engine.new_stdict(engine.n_keys(res.keys))
                res.pattern_cache = cache()

    def units_done(e, res, u0, u1):
        if res.lts:
            engine.stdict_from_mask(res.mask, res.nwin, res.pair_idx, res.nchans, res.keys, into=res.stdict,
                                    cache=res.pattern_cache, units=(u0, u1))

    results = engine.process_multi(rows, fs, t0s, rijs, edges, winlens, WINOVER, ests, FILTER_TYPE, FILTER_ORDER,
                                   FILTER_RIPPLE, vector_len=vector_len, host_overlap=host_side, units_done=units_done)
    if 'w' not in shared:
        shared['w'], shared['h'] = filter_responses(results[0].sos, freq_resp_list, fs)
    out = []
    for (alpha, _), res in zip(ests, results):
        if res.lts:
            if 'size' not in res.stdict:
                res.stdict['size'] = res.nchans
            engine.release_later(res.__dict__.pop('pattern_cache', None), res.__dict__.pop('keys', None))
        out.append(_returns(alpha, res.vel, res.baz, res.mdccm, res.sigma_tau, res.t if len(out) == 0 else res.t.copy(),
                            getattr(res, 'stdict', None), res.nwin, shared['w'].copy(), shared['h'].copy()))
    return out


def narrow_band_loop(ii, freqlist, FREQ_BAND_TYPE, freq_resp_list, st, FILTER_TYPE, FILTER_ORDER,
                     FILTER_RIPPLE, lat_list, lon_list, WINLEN_list, WINOVER, ALPHA, vector_len, rij=None):
    """One band (the reference's joblib task body, narrow_band_least_squares.py:134-218) ->
    ``(vel, baz, mdccm, t, stdict_times, stdict_elements, sig_tau, num_compute, w, h)`` with the
    vectors zero-padded to ``vector_len``."""
    res, w_rows, h_rows = _run_bands([ii], WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, freqlist,
                                     FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER,
                                     FILTER_RIPPLE, vector_len, rij=rij)
    num_compute = np.array(int(res.nwin[0]))
    if ALPHA == 1.0:
        stdict_times = None
        stdict_elements = None
    else:
        sd = res.stdict
        temp_array = np.array(list(sd.items()), dtype=object)
        stdict_times = temp_array[:, 0]
        stdict_elements = temp_array[:, 1]
    return (res.vel[0], res.baz[0], res.mdccm[0], res.t[0], stdict_times, stdict_elements,
            res.sigma_tau[0], num_compute, w_rows[0], h_rows[0])


def _launch_share(hd, up, rows, prep, mine, wsl, cap, block_bytes, use_stream):
    """Queue rank's share ``mine`` (band indices; ``wsl``: its window slice of all bands instead) on its handle ``hd``,
    whose trace ``up`` is bringing up."""
    if len(mine) <= cap:
        # (queued while the rows may still be going up: the library filters the channels as they land)
        try:
            engine.launch(hd, rows, prep, bands=None if wsl else mine, window_slice=wsl, reserve_bytes=block_bytes,
                          trace_ready=True, before_execute=None if up.row_pipeline else up.landed, stream=use_stream)
        except BaseException:
            up.landed()                     # the upload's own error is the cause, if it has one
            raise
        up.landed()
        return
    # the rank's share does not fit the HBM budget of one pass (NBLS_MAX_FILTERED_GB): consecutive passes of
    # <= cap bands, each fetched to the host; the assembled block goes back to the GPU for the ONE gather
    grids = np.zeros((4, len(mine), prep.vector_len))
    mask = np.zeros((len(mine), prep.vector_len, prep.mask_bytes), dtype=np.uint8)
    for k0 in range(0, len(mine), cap):
        sub = mine[k0:k0 + cap]
        engine.launch(hd, rows, prep, bands=sub, window_slice=wsl, reserve_bytes=block_bytes, trace_ready=True,
                      before_execute=up.landed)
        engine.drain(hd, False, grids, mask, k0, k0 + len(sub))
    hd.load_result_block(np.frombuffer(grids.tobytes() + mask.tobytes(), dtype=np.uint8))


def _stream_local_dictionaries(group, shards, prep, keys):
    """Where the shares are contiguous band ranges, every LOCAL pass also STREAMS its rows to the host
    (nbls_stream_results), and the dropped-element dictionary — one entry per window, ~130 ns each under the GIL: 6.5 ms
    at the benchmark's shape, more than an eighth of a GPU pass — is built for the local ranks while the GPUs are still
    working: all of it when one process drives every GPU, this rank's 1/world of it under a launcher (the other ranks'
    entries are made after the gather, from the gathered masks; so do the grids arrive).  -> (head, parts, pattern cache).
    Rank order = band order: the lowest local rank's batches first (the later ranks' rows wait in their pinned mirrors
    meanwhile).  Local ranks 0, 1, … (a prefix of the rank order) write straight into the final dictionary ``head``; a
    local rank r behind a remote one fills ``parts[r]``, merged in rank order after the gather (None: r's are in ``head``)."""
    cum = np.concatenate(([0], np.cumsum(prep.nwin))).astype(np.int64)
    smask = np.zeros((prep.nbands, prep.vector_len, prep.mask_bytes), dtype=np.uint8)
    head, parts, cache = engine.new_stdict(engine.n_keys(keys)), {}, engine.new_pattern_cache()
    order = sorted(range(len(group.handles)), key=lambda i: group.ranks[i])
    for n, i in enumerate(order):
        r, sh = group.ranks[i], shards[group.ranks[i]]
        target = head
        if r != n:
            target = parts[r] = engine.new_stdict(int(cum[sh[-1] + 1] - cum[sh[0]]) if sh else 0)
        parts.setdefault(r, None)
        if sh:
            engine.drain(group.handles[i], True, None, smask, sh[0], sh[-1] + 1, functools.partial(
                _units_into, target, cache, smask, prep, keys, int(cum[sh[0]])))
    return head, parts, cache


def _units_into(target, cache, mask, prep, keys, base, u0, u1):
    if u1 > u0:
        engine.stdict_from_mask(mask, prep.nwin, prep.pair_idx, prep.nchans, keys, into=target, cache=cache,
                                units=(base + u0, base + u1))


def _merge_dictionaries(head, parts, cache, shards, mask, prep, keys):
    """Rank order = band order = the order of the reference's dictionary: what a local rank streamed is there already
    (``_stream_local_dictionaries``), the rest comes from the gathered masks."""
    cum = np.concatenate(([0], np.cumsum(prep.nwin))).astype(np.int64)
    for r, sh in enumerate(shards):
        if r not in parts:
            if sh:
                engine.stdict_from_mask(mask, prep.nwin, prep.pair_idx, prep.nchans, keys, into=head, cache=cache,
                                        units=(int(cum[sh[0]]), int(cum[sh[-1] + 1])))
        elif parts[r] is not None:
            head.update(parts[r])
    if 'size' not in head:
        head['size'] = prep.nchans
    engine.release_later(cache)
    return head


def _assemble(blocks, shards, prep):
    """The ranks' gathered result blocks -> (grids (4, NBANDS, VL), mask).  ``shards`` None: window slices, which are
    disjoint, and rows outside a slice are zero: grids add, masks OR."""
    NB, VL, MB = prep.nbands, prep.vector_len, prep.mask_bytes
    grids = np.zeros((4, NB, VL))
    mask = np.zeros((NB, VL, MB), dtype=np.uint8)
    for r in range(len(blocks)):
        if shards is None:
            g, m = engine.split_block(blocks[r], NB, VL, MB)
            grids += g
            mask |= m
        else:
            g, m = engine.split_block(blocks[r], len(shards[r]), VL, MB)
            grids[:, shards[r], :] = g
            mask[shards[r]] = m
    return grids, mask


def narrow_band_least_squares_parallel(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h,
                                       freqlist, FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER,
                                       FILTER_RIPPLE, rij=None):
    """Band-parallel variant (reference: narrow_band_least_squares.py:223-323, joblib over bands).

    The bands are partitioned over the GPUs of the node by cost (fewer bands than GPUs, or
    ``NBLS_SHARD=windows``: every GPU takes all bands but one contiguous slice of each band's windows),
    every GPU runs the whole hot path for its share, and ONE grouped RCCL operation inside the library
    (``nbls_comm_gather``) collects the result blocks — grids and packed LTS weights together — over
    xGMI.  Either one process drives all visible GPUs (default; ``NBLS_DEVICES`` selects them), or one
    process per GPU was started by a launcher that exports ``RANK``/``WORLD_SIZE``/``LOCAL_RANK`` (then
    every rank returns the complete 9-tuple).  With one GPU this is the batched single-GPU call.  Results
    are identical in every form: no value crosses bands.  No PyTorch is involved."""
    group = dist.get_group()
    if group is None or group.world == 1 and os.environ.get('NBLS_FORCE_DIST_PATH') != '1':
        return narrow_band_least_squares(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h,
                                         freqlist, FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER,
                                         FILTER_RIPPLE, rij=rij)
    world = group.world
    vector_len = _vector_len(WINLEN_list, WINOVER, st)
    rows, fs, t0 = engine.stream_rows(st)
    nchans, npts = len(rows), len(rows[0])
    bands = list(range(NBANDS))
    winlens = [WINLEN_list[ii] for ii in bands]
    status, failure, prep, shards = 0, None, None, None
    by_windows = NBANDS < world or os.environ.get('NBLS_SHARD') == 'windows'
    # the trace goes up to every local GPU on helper threads (the copy runs inside the library, GIL released) while
    # this thread designs the filters of all bands; a pass is planned as soon as the design is there and queued when
    # its GPU's copy has landed (long traces: while the rows still go up)
    uploads = []                    # one engine.TraceUpload per local handle
    try:
        for hd in group.handles:
            uploads.append(engine.TraceUpload(hd, rows, fs))
    except Exception as e:
        status, failure = 1, e
    try:
        if rij is None:
            rij = get_rij(lat_list, lon_list, nchans)
        edges = _band_edges(freqlist, FREQ_BAND_TYPE, bands)
        prep = engine.prepare(nchans, npts, fs, rij, edges, winlens, WINOVER, ALPHA, FILTER_TYPE, FILTER_ORDER,
                              FILTER_RIPPLE, vector_len)
    except Exception as e:          # a rank that cannot even plan still takes part in the gather (status word)
        status, failure = 1, failure or e
    npairs = nchans * (nchans - 1) // 2
    nb_block = NBANDS
    if not by_windows:
        shards, contiguous = dist.plan_shards(dist.band_costs(npts, fs, winlens, WINOVER, npairs), world)
        nb_block = max(1, max(len(sh) for sh in shards))
    block_bytes = (nb_block * vector_len * (32 + (npairs + 7) // 8) + 7) // 8 * 8 + 8       # + the status word

    use_stream = False              # contiguous band shares under LTS: see _stream_local_dictionaries
    if status == 0:
        cap = max(1, engine.max_bands_per_pass(nchans, npts))      # filtered bands one pass may keep in HBM
        use_stream = (not by_windows and ALPHA < 1.0 and contiguous
                      and engine.stream_pays(ALPHA, prep.nwin, npairs) and max(len(sh) for sh in shards) <= cap
                      and all(hasattr(hd, 'wait_result_batch') for hd in group.handles))

        def start(i, hd):
            r = group.ranks[i]
            _launch_share(hd, uploads[i], rows, prep, bands if by_windows else shards[r], (r, world) if by_windows else None,
                          cap, block_bytes, use_stream)
        errs = [e for e in dist.run_on_handles(start, group.handles) if e is not None]
        if errs:
            status, failure = 1, errs[0]
    for up in uploads:              # (a failed rank never reached its join)
        up.close()

    # host work that needs no GPU result, while the passes run; then the local shares' dictionary, batch by batch
    w_array = h_array = t_array = keys = stdict_head = None
    if status == 0:
        try:
            w_array, h_array = filter_responses(prep.sos_ret, freq_resp_list, fs)
            if 0 in group.ranks:
                _bt_cautions(winlens, edges)
            t_array = engine.time_grid(t0, fs, prep.W, prep.inc, prep.nwin, vector_len)
            if ALPHA < 1.0:
                keys = engine.time_key_text(t_array, prep.nwin, [_band_prefix(ii + 1) for ii in bands])
            if use_stream:
                stdict_head, stdict_parts, cache = _stream_local_dictionaries(group, shards, prep, keys)
        except Exception as e:      # noqa: BLE001 - reported through the gather's status word like every other local failure
            status, failure, stdict_head = 1, e, None

    blocks = group.gather(block_bytes, status)          # the ONE collective
    if failure is not None:
        raise failure
    if blocks is None:                                  # this process does not drive the root GPU
        return None
    stat = np.ascontiguousarray(blocks[:, -8:]).view(np.int64).ravel()
    if np.any(stat != 0):
        raise RuntimeError('narrow_band_least_squares_parallel: rank(s) %s failed' % np.nonzero(stat)[0].tolist())

    grids, mask = _assemble(blocks, shards, prep)
    stdict_all = None
    if ALPHA != 1.0 and stdict_head is None:
        stdict_all = engine.stdict_from_mask(mask, prep.nwin, prep.pair_idx, nchans, keys)
    elif ALPHA != 1.0:
        stdict_all = _merge_dictionaries(stdict_head, stdict_parts, cache, shards, mask, prep, keys)
    return _returns(ALPHA, grids[0], grids[1], grids[2], grids[3], t_array, stdict_all, prep.nwin, w_array, h_array)


def narrow_band_least_squares_beam_trace(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist,
                                         FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij=None, *,
                                         mdccm_min=None, window='hann', kept=False):
    """``narrow_band_least_squares`` followed by ``beam_trace_array`` (NBANDS, npts): per band the delay-and-sum beam of the
    filtered band, steered window by window at the slowness the window solved and stitched over the overlapping windows
    with the synthesis window ``window`` (``'hann'`` / ``'boxcar'``; ``lts_array.ltsva_beam_trace``).
    ``mdccm_min``: only windows whose MdCCM reaches it enter, samples no accepted window covers are 0.0.  ``kept=True``
    (``ALPHA < 1``): every window is summed over the elements FAST-LTS kept in it (every pair of a dropped element has
    lost its weight).  The trace is formed on the GPU behind the last solve of every pass, from the filtered bands that
    are already there.  The first nine returns are those of ``narrow_band_least_squares``.  Whatever the library would
    refuse raises ``ValueError`` before any GPU work, and so does a trace so long that not one filtered band fits the HBM
    budget of a pass."""
    _check_alpha(ALPHA)
    _check_elements_strict(len(st), ALPHA)
    _check_flag('kept', kept)
    if not isinstance(window, str):
        raise ValueError("window must be 'hann' or 'boxcar', not %r" % (window,))
    kept_kw = planner.check_kept(len(st), None, False, False) if kept else None
    planner.check_beam_trace([1], window, mdccm_min, bool(kept), kept_kw is not None)       # (the bands' own lengths: engine.process)
    want = dict(window=window, mdccm_min=mdccm_min, kept=bool(kept))
    return _all_bands(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist, FREQ_BAND_TYPE, freq_resp_list,
                      FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij, tail=lambda res: (res.beam_trace,), alpha_range=False,
                      keywords=lambda *args: dict(kept=kept_kw, want_beam_trace=want))


def narrow_band_least_squares_element_delays(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist,
                                             FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij=None, *,
                                             max_shift=None, kept=False, min_pairs=None):
    """``narrow_band_least_squares`` followed by a dict of each element's delay against the beam of the others, per band:
    ``element_delay`` / ``element_cc`` (NBANDS, vector_len, N) and ``element_shift`` (likewise, int32) — per window and
    element the delay in seconds, the normalised correlation and the whole-sample shift at which the element correlates
    best with the sum of the other elements steered at the window's solved slowness, searched within ``max_shift``
    samples either side of the modelled delay (``lts_array.ltsva_element_delays``).  ``max_shift``: one
    integer in 0..256 or one per band; None: ``planner.element_shifts`` of every band's upper edge, half a period.
    ``kept=True`` (``ALPHA < 1``): the beam is that of the elements FAST-LTS kept in the window (``min_pairs`` as in
    ``lts_array.ltsva_kept``), and the dict also holds ``dropped_mask`` / ``kept_count`` (NBANDS, vector_len).  The first nine
    returns are those of ``narrow_band_least_squares``.  Whatever the library would refuse raises ``ValueError`` before any
    GPU work, and so does a trace so long that not one filtered band fits the HBM budget of a pass."""
    _check_alpha(ALPHA)
    _check_elements_strict(len(st), ALPHA)
    kept_kw = _kept_request(len(st), kept, min_pairs)
    if max_shift is not None:
        engine._check_element_delays(max_shift, bool(kept), NBANDS, len(st), kept_kw)
    elif len(st) > 32:
        raise ValueError('the element delays take at most 32 array elements, not %d' % len(st))

    def keywords(rij_, fs, npts, edges, winlens, vector_len):           # (the keywords that ride into ``engine.process``)
        shifts = max_shift if max_shift is not None else planner.element_shifts([e[1] for e in edges], fs)
        return dict(kept=kept_kw, element_max_shift=shifts, element_delays_kept=bool(kept))

    def tail(res):
        fields = ('element_delay', 'element_cc', 'element_shift') + (('dropped_mask', 'kept_count') if kept else ())
        return ({k: getattr(res, k) for k in fields},)
    return _all_bands(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist, FREQ_BAND_TYPE, freq_resp_list,
                      FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij, tail=tail, alpha_range=False, keywords=keywords)


def _families_of(res, edges, fs, t0):
    """(family_array, families) of a ``BandBatch`` with ``family`` / ``family_table``: the int32 grid and the per-family
    summary of ``planner.family_table`` (the table's own columns among it)."""
    return res.family, planner.family_table(res.family, res.family_table, res.vel, res.baz, res.mdccm, res.sigma_tau, edges, res.W,
                                            res.inc, fs, t0)


def narrow_band_least_squares_families(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist,
                                       FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij=None, *,
                                       mdccm_min, baz_tol, vel_tol, vel_min, vel_max, sigma_tau_max=None, band_reach=1,
                                       time_reach=1, min_pixels=4):
    """``narrow_band_least_squares`` followed by ``family_array`` (NBANDS, vector_len) int32 and ``families``: the (band,
    window) cells grouped into detections, as PMCC groups its pixels into families (the definition is
    in include/nbls.h).  A cell is eligible with ``mdccm >= mdccm_min``, ``vel_min <= vel <= vel_max`` and, where
    ``sigma_tau_max`` is given, ``sigma_tau <= sigma_tau_max``; two eligible cells are linked when their bands are at most
    ``band_reach`` apart, their window centres at most ``time_reach`` hops of the coarser band apart, their back-azimuths
    within ``baz_tol`` degrees (across 0 / 360) and their velocities within ``vel_tol`` km/s; a family is a connected component
    of at least ``min_pixels`` cells.  ``family_array`` holds the family id, -2 for an eligible cell of a smaller component
    and -1 elsewhere; ``families`` is the dict of ``planner.family_table`` (one entry per family: count, start and end,
    frequency range, circular mean and spread of the back-azimuth, velocity, MdCCM, the peak cell) with the raw table columns
    (``planner.FAMILY_FIELDS``).  Single linkage: a family can drift along a chain of cells that each agree with the next.
    Labelled on the GPU behind the pass's last solve; a call whose bands run in several passes is labelled by the same
    kernels on the assembled grids, with the same result.  ``ValueError`` before any GPU work for what the library refuses."""
    par = planner.check_families(mdccm_min, baz_tol, vel_tol, vel_min, vel_max, sigma_tau_max, band_reach, time_reach, min_pixels)

    def tail(res):
        _, fs, t0 = engine.stream_rows(st)
        return _families_of(res, _band_edges(freqlist, FREQ_BAND_TYPE, range(NBANDS)), fs, t0)
    return _all_bands(WINLEN_list, WINOVER, ALPHA, st, lat_list, lon_list, NBANDS, w, h, freqlist, FREQ_BAND_TYPE, freq_resp_list,
                      FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij, tail=tail, alpha_range=False, keywords=lambda *a: dict(families=par))


def narrow_band_least_squares_families_batch(WINLEN_list, WINOVER, ALPHA, streams, lat_list, lon_list, NBANDS, w, h, freqlist,
                                             FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij=None, *,
                                             mdccm_min, baz_tol, vel_tol, vel_min, vel_max, sigma_tau_max=None, band_reach=1,
                                             time_reach=1, min_pixels=4):
    """``narrow_band_least_squares_families`` over several recordings of ONE array in one GPU pass -> a list of its 11-tuples,
    element i equal to the single call on ``streams[i]``; the streams as for ``narrow_band_least_squares_batch``.  Recordings
    never link: every recording has its own families, numbered from 0."""
    par = planner.check_families(mdccm_min, baz_tol, vel_tol, vel_min, vel_max, sigma_tau_max, band_reach, time_reach, min_pixels)
    return _all_bands_batch(narrow_band_least_squares_families, WINLEN_list, WINOVER, ALPHA, streams, lat_list, lon_list, NBANDS, w, h,
                            freqlist, FREQ_BAND_TYPE, freq_resp_list, FILTER_TYPE, FILTER_ORDER, FILTER_RIPPLE, rij, par, _families_of,
                            families=par)


def label_families(vel, baz, mdccm, sigma_tau, nwin, winlens, incs, *, nseg=1, device=None, **params):
    """The families of result grids the caller already has (``nbls_label_families``): ``vel``, ``baz``, ``mdccm`` and
    ``sigma_tau`` (None exactly when ``sigma_tau_max`` is not given) of shape (nbands * nseg, vector_len), row b * nseg + s band
    b of recording s; ``nwin`` one entry per row; ``winlens`` / ``incs`` window length and hop of every band in samples;
    ``params`` the request of ``narrow_band_least_squares_families`` (``planner.check_families``).  The same kernels as the
    in-pass request, on the GPU: for the gathered result of ``narrow_band_least_squares_parallel``, the rows of another
    estimator, or another detector's grid handed in as ``mdccm``.  -> (family int32 of the grids' shape, table int64 (F, 8),
    columns ``planner.FAMILY_FIELDS``).  ``ValueError`` before any GPU work for what the library refuses."""
    try:
        par = planner.check_families(**params)
    except TypeError as e:
        raise ValueError('label_families: %s' % e)
    args = planner.check_family_lattice(nseg, winlens, incs, nwin, vel, baz, mdccm, sigma_tau, par['sigma_tau_max'] is not None)
    from ._hip import family_params
    h = engine.get_handle(device, 0)
    family, _, table = h.label_families(family_params(**par), args[0], args[1], args[2], args[3], args[4], args[5], args[6], args[7])
    return family, table
