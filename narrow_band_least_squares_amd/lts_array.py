"""GPU ``ltsva``: drop-in for ``from lts_array import ltsva`` (reference call sites
narrow_band_least_squares.py:91,183 and example.py:109; the lts_array source itself is an
empty git submodule in the reference checkout, so the algorithm follows the published one as
summarised in SURVEY.md §3.3).
"""
import typing

import numpy as np

from . import engine, planner
from .helpers import get_rij

OLS_MESSAGE = 'ALPHA is 1.0. Performing an ordinary least squares fit, NOT least trimmed squares.'


def _returns(res, nchans, alpha, keys=None):
    """One band's ``BandBatch`` -> ltsva's 8-tuple (copies of the band's first ``nwin`` cells).  The confidence intervals
    (Szuberla & Olson) are per-unit scalar math on the GPU behind the solve, csrc/solve.hip: uncertainty_kernel."""
    n = int(res.nwin[0])
    stdict = {}
    if alpha != 1.0:
        stdict = engine.stdict_from_mask(res.mask, res.nwin, res.pair_idx, nchans,
                                         engine.time_keys(res.t, res.nwin) if keys is None else keys)
    vel, baz, t, mdccm, sigma_tau, conf_int_vel, conf_int_baz = [
        a[0, :n].copy() for a in (res.vel, res.baz, res.t, res.mdccm, res.sigma_tau, res.vel_uncert, res.baz_uncert)]
    return vel, baz, t, mdccm, stdict, sigma_tau, conf_int_vel, conf_int_baz


def _returns_beam(res, nchans, alpha, keys=None):
    """``_returns`` followed by the band's ``beam_power`` and ``fstat`` (csrc/beam.hip: beam_fstat_kernel)."""
    return _returns(res, nchans, alpha, keys) + _beam_tail(res)


def _beam_tail(res):
    n = int(res.nwin[0])
    return res.beam_power[0, :n].copy(), res.fstat[0, :n].copy()


def _returns_consistency(res):
    """The band's ``consistency``, ``closure_max`` (nwin,) and ``element_consistency`` (nwin, N) (csrc/closure.hip:
    closure_kernel)."""
    n = int(res.nwin[0])
    return res.consistency[0, :n].copy(), res.closure_max[0, :n].copy(), res.element_consistency[0, :n].copy()


def grid_slowness(grid, index):
    """The slowness vectors ``grid[index]`` of a grid search as ``ltsva`` reports a slowness -> (grid_vel, grid_baz):
    ``grid_vel = 1 / |s|`` km/s (``inf`` for s = 0), ``grid_baz = (atan2(s0, s1) * 180 / pi - 360) mod 360`` degrees, the
    formula of the solve kernel (csrc/solve.hip); both NaN where the index is -1."""
    index = np.asarray(index)
    s = np.asarray(grid, dtype=np.float64)[np.maximum(index, 0)]
    with np.errstate(divide='ignore'):
        vel = 1.0 / np.hypot(s[..., 0], s[..., 1])
    baz = np.mod(np.arctan2(s[..., 0], s[..., 1]) * 180.0 / np.pi - 360.0, 360.0)
    none = index < 0
    return np.where(none, np.nan, vel), np.where(none, np.nan, baz)


def peak_slowness(grid, steps, index, offset):
    """The refined slowness vectors of a peak request -> (slowness (..., K, 2), vel (..., K), baz (..., K)):
    ``grid[index] + offset * steps`` s/km (``steps``: ``planner.grid_cells(grid)[1]``) and its velocity and back-azimuth by the
    formula of ``grid_slowness``; all NaN where the index is -1."""
    index = np.asarray(index)
    none = index < 0
    s = np.asarray(grid, dtype=np.float64)[np.maximum(index, 0)] + np.where(none[..., None], 0.0, offset) * np.asarray(steps)
    with np.errstate(divide='ignore'):
        vel = 1.0 / np.hypot(s[..., 0], s[..., 1])
    baz = np.mod(np.arctan2(s[..., 0], s[..., 1]) * 180.0 / np.pi - 360.0, 360.0)
    return np.where(none[..., None], np.nan, s), np.where(none, np.nan, vel), np.where(none, np.nan, baz)


def _returns_grid(res, grid, want_map):
    """The band's slowness-grid results behind ``_returns``: ``grid_vel, grid_baz, grid_fstat, grid_power, grid_index`` and,
    when asked, the map (csrc/beam_grid.hip: beam_grid_kernel)."""
    n = int(res.nwin[0])
    idx = res.grid_index[0, :n].copy()
    vel, baz = grid_slowness(grid, idx)
    out = (vel, baz, res.grid_fstat[0, :n].copy(), res.grid_power[0, :n].copy(), idx)
    return out + ((res.grid_map[0, :n].copy(),) if want_map else ())


def refined_slowness(slowness, index):
    """The refined slowness vectors ``slowness`` (..., 2) of a grid search with refinement -> (refined_vel, refined_baz) by
    the formula of ``grid_slowness``; both NaN where the grid index is -1."""
    s = np.asarray(slowness, dtype=np.float64)
    none = np.asarray(index) < 0
    with np.errstate(divide='ignore', invalid='ignore'):
        vel = 1.0 / np.hypot(s[..., 0], s[..., 1])
        baz = np.mod(np.arctan2(s[..., 0], s[..., 1]) * 180.0 / np.pi - 360.0, 360.0)
    return np.where(none, np.nan, vel), np.where(none, np.nan, baz)


REFINED_FIELDS = ('grid_refined_slowness', 'grid_refined_fstat', 'grid_refined_power', 'grid_refined_path', 'grid_refined_stencil')


def _returns_grid_refined(res):
    """The band's refined grid maximum behind ``_returns_grid``: ``refined_vel, refined_baz`` (``refined_slowness``) and the five
    fields of the refinement (csrc/beam_grid_refine.hip: grid_refine_kernel)."""
    n = int(res.nwin[0])
    slow = res.grid_refined_slowness[0, :n].copy()
    return refined_slowness(slow, res.grid_index[0, :n]) + (slow,) + tuple(getattr(res, k)[0, :n].copy() for k in REFINED_FIELDS[1:])


def _picker(band, n):
    """How the ``_returns_*`` dictionaries take a field of a ``BandBatch``: a copy of row ``band``, its first ``n`` cells or
    (``n=None``) all of them; ``band=None``: the array itself, every band's rows."""
    if band is None:
        return lambda a: a
    sl = slice(None) if n is None else slice(0, n)
    return lambda a: a[band, sl].copy()


def _returns_capon(res, grid, want_maps, band=0, n=None):
    """A band's Capon results as a dict: the four fields, the slowness (``grid_slowness``) at either index and, when asked,
    both maps (csrc/capon.hip: capon_kernel); for a pass with a peak request also its eight fields and the refined slowness
    of every rank (``peak_slowness``).  ``n=None``: the band's first ``nwin`` cells, copied; else whole rows."""
    pick = _picker(band, n)
    out = {k: pick(getattr(res, k)) for k in ('capon_index', 'capon_power', 'bartlett_index', 'bartlett_power')}
    out['capon_vel'], out['capon_baz'] = grid_slowness(grid, out['capon_index'])
    out['bartlett_vel'], out['bartlett_baz'] = grid_slowness(grid, out['bartlett_index'])
    if want_maps:
        out['capon_map'], out['bartlett_map'] = pick(res.capon_map), pick(res.bartlett_map)
    if getattr(res, 'capon_peak_count', None) is not None:
        steps = planner.grid_cells(grid)[1]
        for which in ('capon', 'bartlett'):
            for field in engine.PEAK_FIELDS:
                out[which + field] = pick(getattr(res, which + field))
            out[which + '_peak_slowness'], out[which + '_peak_vel'], out[which + '_peak_baz'] = peak_slowness(
                grid, steps, out[which + '_peak_index'], out[which + '_peak_offset'])
    return out


def _peak_keywords(grid, peaks, peak_floor):
    """The peak keywords of ``engine.process`` behind ``peaks`` / ``peak_floor`` of the Capon entry points ({} for ``peaks=0``);
    the cells are the grid's own lattice (``planner.grid_cells``).  ``ValueError`` before any GPU work."""
    if isinstance(peaks, (int, np.integer)) and not isinstance(peaks, (bool, np.bool_)) and peaks == 0:
        return {}
    cells, K, floor = planner.check_capon_peaks(len(grid), planner.grid_cells(grid)[0], peaks, peak_floor)
    return dict(capon_peaks=K, capon_peak_floor=floor, capon_cells=cells)


def _capon_keywords(nchans, rij, fs, W, slowness_grid, freq, snapshots, loading, maps, peaks=0, peak_floor=0.25):
    """The Capon keywords of ``engine.process`` for one filtered band of window length ``W`` samples; the snapshots default
    to ``planner.capon_snapshots``.  ``ValueError`` before any GPU work."""
    grid = planner.check_slowness_grid(slowness_grid)
    _check_flag('maps', maps)
    if snapshots is None:
        f = planner.check_capon(nchans, grid, [freq], (1, 1), loading, [W])[1]
        snapshots = planner.capon_snapshots(planner.co_array(rij)[0], grid, fs, f, [W])
    planner.check_capon(nchans, grid, [freq], snapshots, loading, [W], bool(maps))
    return dict(capon_grid=grid, capon_freqs=[freq], capon_snapshots=snapshots, capon_loading=loading,
                want_capon_maps=bool(maps), **_peak_keywords(grid, peaks, peak_floor))


class _Feature(typing.NamedTuple):
    """What an opt-in feature hands the two bodies below.  ``keywords(nchans, alpha, rij, fs, npts)``: its keywords of
    ``engine.process`` (``ValueError`` for whatever the library would refuse); ``tail(res, kw, nchans, fs, t0)``: the tuple its
    returns add to ``_returns(...)``, from one recording's result and those keywords; ``strict``: too few elements raise
    ``ValueError`` ahead of everything else (False: the engine's ``RuntimeError``, as the reference's ``ltsva``)."""
    keywords: typing.Callable
    tail: typing.Callable
    strict: bool = True


def _ltsva(st, lat_list, lon_list, window_length, window_overlap, alpha, rij, feature):
    """The one body of every single-stream entry point: the element checks, the geometry, the feature's keywords, the
    message, the device pass — the key text of the dictionary made while it is in flight —, the returns."""
    data, fs, t0 = engine.stream_rows(st)
    nchans = len(data)
    if feature.strict:
        _check_elements_strict(nchans, alpha)
    engine.check_elements(nchans, alpha)
    if rij is None:
        rij = get_rij(lat_list, lon_list, nchans)
    kw = feature.keywords(nchans, alpha, rij, fs, len(data[0]))
    if alpha == 1.0:
        print(OLS_MESSAGE)

    def host_side(res):        # key text of the dropped-element dictionary: needs no GPU result
        if alpha < 1.0:
            res.keys = engine.time_keys(res.t, res.nwin)

    res = engine.process(data, fs, t0, rij, [(None, None)], [window_length], window_overlap, alpha, prefiltered=True,
                         host_overlap=host_side, want_uncert=True, **kw)
    return _returns(res, nchans, alpha, getattr(res, 'keys', None)) + feature.tail(res, kw, nchans, fs, t0)


def _ltsva_batch(streams, lat_list, lon_list, window_length, window_overlap, alpha, rij, feature, one=None):
    """The one body of every ``_batch`` entry point: ``_ltsva`` for several recordings in one pass (no host work rides
    behind it: the key text is made in ``_returns``).  ``one``: the feature of the single call a batch of one recording is,
    where it is not ``feature`` itself."""
    streams = list(streams)
    if not streams:
        return []
    recs, fs, t0s = engine.batch_rows(streams)
    if len(streams) == 1:          # a batch of one IS the single call
        return [_ltsva(streams[0], lat_list, lon_list, window_length, window_overlap, alpha, rij, one or feature)]
    nchans = len(recs[0])
    if feature.strict:
        _check_elements_strict(nchans, alpha)
    engine.check_elements(nchans, alpha)
    if rij is None:
        rij = get_rij(lat_list, lon_list, nchans)
    kw = feature.keywords(nchans, alpha, rij, fs, len(recs[0][0]))
    if alpha == 1.0:
        print(OLS_MESSAGE)
    results = engine.process_batch(recs, fs, t0s, rij, [(None, None)], [window_length], window_overlap, alpha, prefiltered=True,
                                   want_uncert=True, **kw)
    return [_returns(res, nchans, alpha) + feature.tail(res, kw, nchans, fs, t0) for res, t0 in zip(results, t0s)]


def _window(npts, fs, window_length, window_overlap):
    """The window length in samples of a filtered stream's one band."""
    return int(planner.window_plan(npts, fs, window_length, window_overlap)[0])


def _plain(beam=False, subsample=False, min_velocity=None, grid=None, grid_map=False, seeds=None, consistency=False, capon=None,
           batch=False):
    """The feature of ``ltsva`` and of what combines with it in ``ltsva_batch`` / ``ltsva_multi``: beam, refined lags, bounded
    or seeded search, slowness grid, closure and (``capon``: a function of (nchans, rij, fs, npts) -> its keywords) the
    Capon spectra.  ``ltsva`` itself keeps the reference's ``RuntimeError`` for too few elements, and so does a batch of several
    recordings without the spectra; ``batch``: as ``ltsva_batch`` passes it on, without the keywords no batch form takes."""
    own = dict(want_beam=beam, want_subsample=subsample, min_velocity=min_velocity, slowness_grid=grid)
    if not batch:
        own.update(want_grid_map=grid_map, seed_halfwidths=seeds, want_consistency=consistency)

    def keywords(nchans, alpha, rij, fs, npts):
        return own if capon is None else dict(own, **capon(nchans, rij, fs, npts))

    def tail(res, kw, nchans, fs, t0):
        out = _beam_tail(res) if beam else ()
        if grid is not None:
            out += _returns_grid(res, grid, grid_map)
        if capon is not None:
            out += (_returns_capon(res, kw['capon_grid'], kw['want_capon_maps'], n=int(res.nwin[0])),)
        return out + _returns_consistency(res) if consistency else out
    flagged = beam or subsample or min_velocity is not None or grid is not None or consistency
    # (``ltsva_batch`` of several recordings has always left too few elements to the engine, flags or not; only its batch
    #  of one, the single call, and the forms with the spectra are strict)
    return _Feature(keywords, tail, capon is not None or (flagged and not batch))


_LTSVA = _plain()          # (the plain call builds nothing per call)


def ltsva(st, lat_list, lon_list, window_length, window_overlap, alpha=1.0,
          plot_array_coordinates=False, rij=None):
    """Window the (already filtered) stream, pick pairwise cross-correlation lags and solve for
    the slowness vector by OLS (``alpha == 1.0``) or FAST-LTS (``0.5 <= alpha < 1``).

    Returns ``(vel, baz, t, mdccm, stdict, sigma_tau, conf_int_vel, conf_int_baz)``:
    trace velocity km/s, back-azimuth degrees in [0, 360), window-centre times as matplotlib
    date numbers, median cross-correlation maximum, dropped-element dictionary (``{}`` for
    OLS), sigma_tau seconds, and the 90 % confidence half-widths of trace velocity (km/s) and
    back-azimuth (degrees; NaN where the direction is undetermined).  ``rij`` (2, N) km overrides the lat/lon geometry."""
    if plot_array_coordinates:
        import warnings
        warnings.warn('plot_array_coordinates is not supported on the HIP path; ignored.')
    return _ltsva(st, lat_list, lon_list, window_length, window_overlap, alpha, rij, _LTSVA)


def ltsva_beam(st, lat_list, lon_list, window_length, window_overlap, alpha=1.0, rij=None):
    """``ltsva`` followed by two more returns per window: ``beam_power``, the mean power of the delay-and-sum beam at the
    solved slowness, and ``fstat``, its Fisher ratio (N-1) S_b / (N S_t - S_b) — the array detector users threshold on
    beside MdCCM.  The elements are shifted by whole samples, the modelled lags of the pairs (0, i) rounded to even;
    samples outside the trace count as zeros (DESIGN.md section 12 has the definition).  ``fstat`` is ``inf`` for channels
    that line up exactly and NaN for an all-zero window or a slowness that is not finite.  Both are computed on the GPU
    behind each window's solve, from the filtered samples already there.  The first eight returns are ``ltsva``'s.
    Too few elements raise ``ValueError`` here (``ltsva`` keeps the reference's ``RuntimeError``)."""
    return _ltsva(st, lat_list, lon_list, window_length, window_overlap, alpha, rij, _plain(beam=True))


def _check_elements_strict(nchans, alpha):
    if nchans < 3 or (alpha < 1.0 and nchans < 4):
        raise ValueError('%d array elements: at least 3 are needed for the least squares estimate, 4 for least trimmed '
                         'squares' % nchans)


def _check_flag(name, value):
    if not isinstance(value, (bool, np.bool_)):
        raise ValueError('%s must be True or False, not %r' % (name, value))


def ltsva_subsample(st, lat_list, lon_list, window_length, window_overlap, alpha=1.0, rij=None):
    """``ltsva`` on lags refined to sub-sample precision: behind the lag pick every pair's lag l gets the vertex offset of
    the parabola through the raw cross-correlation values at l-1, l, l+1 (clamped to half a sample; 0 where there is no
    strict maximum, at the ends of the lag range and for windows that are not finite), and the slowness is fitted to
    ``tau = (lag + frac) / fs`` instead of ``lag / fs`` (DESIGN.md section 13 has the definition).  ``sigma_tau`` then no
    longer sits on the quantisation floor 1 / (fs sqrt(12)) of whole-sample lags, and the confidence intervals follow.
    MdCCM and the key text of ``stdict`` are those of ``ltsva``; which pairs LTS drops may differ, as the residuals do.
    The fractions are computed on the GPU from the filtered samples already there (csrc/refine.hip).  Returns ``ltsva``'s
    8-tuple.  Too few elements raise ``ValueError`` here (``ltsva`` keeps the reference's ``RuntimeError``)."""
    return _ltsva(st, lat_list, lon_list, window_length, window_overlap, alpha, rij, _plain(subsample=True))


def ltsva_consistency(st, lat_list, lon_list, window_length, window_overlap, alpha=1.0, rij=None, subsample=False):
    """``ltsva`` followed by the closure (consistency) of the picked lags, as PMCC uses it (Cansi 1995): for three elements
    i < j < k the lags of one coherent arrival satisfy ``l_ij + l_jk - l_ik = 0`` whatever its slowness, its wavefront's
    curvature or the elements' clock offsets; only noise, cycle skips and several arrivals break it.  Three more returns
    per window, in seconds: ``consistency`` (nwin,), the rms closure over all N (N-1) (N-2) / 6 triplets,
    ``closure_max`` (nwin,), the largest ``|closure|``, and ``element_consistency`` (nwin, N), per element the rms over the
    (N-1) (N-2) / 2 triplets that hold it (DESIGN.md section 17 has the definition).  A mistimed or misplaced element
    leaves all three untouched while LTS drops it; a noisy element raises its own column.  ``subsample=True``: the lags are
    refined to sub-sample precision first (``ltsva_subsample``), the closure is that of the refined delays and the first
    eight returns are ``ltsva_subsample``'s; else they are ``ltsva``'s.  Computed on the GPU behind each window's solve,
    from the lag table already there (csrc/closure.hip).  A ``subsample`` that is not a bool and too few elements raise
    ``ValueError`` before any GPU work."""
    _check_flag('subsample', subsample)
    return _ltsva(st, lat_list, lon_list, window_length, window_overlap, alpha, rij,
                  _plain(subsample=bool(subsample), consistency=True))


def ltsva_bounded(st, lat_list, lon_list, window_length, window_overlap, min_velocity, alpha=1.0, rij=None):
    """``ltsva`` with every pair's lag searched only within its physical range: ``|lag_k| <= L_k`` samples,
    ``L_k = ceil(fs |xij_k| / min_velocity) + 1`` (``planner.lag_limits``), the delay a plane wave no slower than
    ``min_velocity`` km/s can put between the pair's elements plus one sample of guard, instead of over all 2W-1 lags.  In
    a narrow band the correlation is nearly periodic and noise lifts a neighbouring cycle above the true one; such
    cycle-skipped picks land outside the range and are the outliers the fit then has to survive (DESIGN.md section 14 has
    the definition and the counts).  The pick, its ``cmax`` (so MdCCM) and everything fitted to it follow the restricted
    search; the search runs on the GPU (csrc/xcorr_bounded.hip).  Returns ``ltsva``'s 8-tuple.  ``min_velocity`` must be a
    finite real > 0 and too few elements raise ``ValueError`` before any GPU work."""
    planner.check_min_velocity(min_velocity)
    return _ltsva(st, lat_list, lon_list, window_length, window_overlap, alpha, rij, _plain(min_velocity=min_velocity))


def ltsva_grid(st, lat_list, lon_list, window_length, window_overlap, slowness_grid, alpha=1.0, rij=None, grid_map=False):
    """``ltsva`` followed by the slowness-grid search of the beam F-statistic: per window the delay-and-sum beam of the
    full array is steered over the slowness vectors ``slowness_grid`` (G, 2) s/km (``planner.slowness_grid`` makes a
    Cartesian one) by whole-sample delays, and the grid point with the largest Fisher ratio (N-1) S_b / (N S_t - S_b) is
    reported — the estimate that does not rest on pairwise lag picks, which at low SNR fail pair by pair where the whole
    array still sees the wave (DESIGN.md section 15 has the definition and the counts).  Returns ``ltsva``'s 8-tuple followed
    by ``grid_vel`` (1 / |s| km/s at the maximum, ``inf`` for s = 0), ``grid_baz`` (degrees, the solve's formula),
    ``grid_fstat``, ``grid_power``, ``grid_index`` (int32, -1 with NaN in the other four where no grid point has a ratio: an
    all-zero window) and, with ``grid_map=True``, the ratio at every grid point (nwin, G).  Among equal ratios the lowest
    index wins.  The search runs on the GPU behind each window's solve, from the filtered samples already there
    (csrc/beam_grid.hip).  A bad grid, a ``grid_map`` that is not a bool and too few elements raise ``ValueError`` before
    any GPU work."""
    grid = planner.check_slowness_grid(slowness_grid)
    _check_flag('grid_map', grid_map)
    return _ltsva(st, lat_list, lon_list, window_length, window_overlap, alpha, rij, _plain(grid=grid, grid_map=bool(grid_map)))


def ltsva_seeded(st, lat_list, lon_list, window_length, window_overlap, slowness_grid, halfwidth, alpha=1.0, rij=None,
                 grid_map=False):
    """``ltsva_grid`` whose lag picks are seeded by the grid maximum — the two-step estimate: per window the whole-array
    beam steered over ``slowness_grid`` chooses the cycle, every pair's cross-correlation is then searched only within
    ``halfwidth`` samples of the delay ``d_j - d_i`` that grid point predicts for the pair (whole samples, the steering
    the beam used), and the usual OLS / LTS solve runs on those picks with everything that hangs on them: ``sigma_tau``,
    confidence intervals, dropped elements (DESIGN.md section 16 has the definition and the counts).  ``halfwidth`` is in
    samples (an integer >= 0) because a filtered stream has no band edges to derive it from: half a period of the band's
    upper edge, ``planner.seed_halfwidths([fmax], fs)[0]``, keeps the neighbouring cycle outside.  Returns ``ltsva_grid``'s
    tuple; the grid returns are those of ``ltsva_grid``.  The search runs on the GPU (csrc/xcorr_seeded.hip).  A bad grid
    or half-width, a ``grid_map`` that is not a bool and too few elements raise ``ValueError`` before any GPU work."""
    grid = planner.check_slowness_grid(slowness_grid)
    seeds = planner.check_seed_halfwidths(halfwidth, 1)
    _check_flag('grid_map', grid_map)
    return _ltsva(st, lat_list, lon_list, window_length, window_overlap, alpha, rij,
                  _plain(grid=grid, grid_map=bool(grid_map), seeds=seeds))


def ltsva_capon(st, lat_list, lon_list, window_length, window_overlap, slowness_grid, freq, alpha=1.0, rij=None, snapshots=None,
                loading=0.01, maps=False, peaks=0, peak_floor=0.25):
    """``ltsva`` followed by the Capon (MVDR) and Bartlett slowness spectra of the narrow band's cross-spectral matrix: per
    window the snapshots (Hann-tapered DFT bins at ``freq`` Hz, ``snapshots = (Ls, Hs)`` samples long and apart; default
    ``planner.capon_snapshots``) of the full array give the matrix R, and over the slowness vectors ``slowness_grid`` (G, 2)
    s/km ``P_B = Re(a^H R a) / N^2`` and, with ``R' = R + loading (tr R / N) I``, ``P_C = 1 / (a^H R'^-1 a)`` — the adaptive
    beamformer that separates two arrivals closer than the array's beam width, where every other estimate here assumes one
    wave (DESIGN.md section 18 has the definition and the counts).  Returns ``ltsva``'s 8-tuple followed by one dict:
    ``capon_index`` / ``bartlett_index`` (int32, -1 where there is no maximum), ``capon_power`` / ``bartlett_power``,
    ``capon_vel`` / ``capon_baz`` / ``bartlett_vel`` / ``bartlett_baz`` (``grid_slowness`` at the indices) and, with
    ``maps=True``, ``capon_map`` / ``bartlett_map`` (nwin, G).  With ``peaks=K`` (1..8; the grid must be a lattice,
    ``planner.grid_cells``) the dict also holds the K strongest local maxima of either spectrum that reach ``peak_floor``
    times its maximum: ``capon_peak_count`` (nwin,), ``capon_peak_index`` / ``capon_peak_power`` (nwin,
    K), ``capon_peak_offset`` (nwin, K, 2) in lattice steps, ``capon_peak_slowness`` (nwin, K, 2) = ``grid[index] + offset *
    steps``, ``capon_peak_vel`` / ``capon_peak_baz`` (nwin, K) of that refined vector, and the same seven with ``bartlett_``;
    ranks beyond the kept peaks are -1 / NaN.  Computed on the GPU behind each window's solve (csrc/capon.hip).  Whatever the
    library would refuse raises ``ValueError`` before any GPU work."""
    return _ltsva(st, lat_list, lon_list, window_length, window_overlap, alpha, rij, _plain(capon=_capon_band(
        window_length, window_overlap, slowness_grid, freq, snapshots, loading, maps, peaks, peak_floor)))


def _capon_band(window_length, window_overlap, *capon):
    """``_capon_keywords`` of a filtered stream's one band, whose window length follows from the trace: the ``capon`` of
    ``_plain``."""
    return lambda nchans, rij, fs, npts: _capon_keywords(nchans, rij, fs, _window(npts, fs, window_length, window_overlap), *capon)


def ltsva_batch(streams, lat_list, lon_list, window_length, window_overlap, alpha=1.0, rij=None, beam=False,
                subsample=False, min_velocity=None, slowness_grid=None):
    """``ltsva`` over several (already filtered) recordings of ONE array in one GPU pass -> a list of 8-tuples,
    element i equal to ``ltsva(streams[i], ...)``.  Every stream must have the same element count, trace length and
    sampling rate, and all share the geometry; ``ValueError`` names a mismatch before any GPU work.  The "ALPHA is
    1.0" message prints once per batch.  An empty sequence gives ``[]``.  ``beam=True``: 10-tuples, element i equal to
    ``ltsva_beam(streams[i], ...)``.  ``subsample=True``: element i equal to ``ltsva_subsample(streams[i], ...)``; with both,
    the beam is steered by the slowness fitted to the refined delays.  ``min_velocity`` (km/s, default None: every lag):
    the lags are searched within their physical range as in ``ltsva_bounded``; it combines with both flags, the fractions
    and the beam then follow the bounded picks.  ``slowness_grid`` (G, 2) s/km, default None: every tuple is followed by the
    five grid returns of ``ltsva_grid`` (no map), element i equal to ``ltsva_grid(streams[i], ...)``; it combines with the
    others, because it reads none of their results.  ``ltsva_capon_batch`` is this call with the Capon spectra,
    ``ltsva_beam_trace_batch`` the one with the beam trace."""
    _check_flag('beam', beam)
    _check_flag('subsample', subsample)
    if min_velocity is not None:
        planner.check_min_velocity(min_velocity)
    if slowness_grid is not None:
        slowness_grid = planner.check_slowness_grid(slowness_grid)
    asked = (bool(beam), bool(subsample), min_velocity, slowness_grid)
    return _ltsva_batch(streams, lat_list, lon_list, window_length, window_overlap, alpha, rij, _plain(*asked, batch=True),
                        one=_plain(*asked))


def ltsva_capon_batch(streams, lat_list, lon_list, window_length, window_overlap, slowness_grid, freq, alpha=1.0, rij=None,
                      snapshots=None, loading=0.01, maps=False, peaks=0, peak_floor=0.25):
    """``ltsva_capon`` over several (already filtered) recordings of ONE array in one GPU pass -> a list of its 9-tuples,
    element i equal to ``ltsva_capon(streams[i], ...)``; the streams as for ``ltsva_batch``."""
    capon = _capon_band(window_length, window_overlap, slowness_grid, freq, snapshots, loading, maps, peaks, peak_floor)
    return _ltsva_batch(streams, lat_list, lon_list, window_length, window_overlap, alpha, rij, _plain(capon=capon, batch=True),
                        one=_plain(capon=capon))


def ltsva_multi(st, lat_list, lon_list, window_length, window_overlap, estimators, rij=None, beam=False, subsample=False,
                min_velocity=None, consistency=False):
    """``ltsva`` of one (already filtered) stream for several estimators ``(alpha, remove)`` in one GPU pass -> a list of
    ``ltsva``'s 8-tuples, element e equal to ``ltsva`` with ``alpha_e`` on the stream without the traces ``remove_e``
    (0-based, ascending; a bare number means nothing removed; at most 8 estimators).  The windows of the full array are
    correlated once, every window is solved once per estimator.  ``ValueError`` before any GPU work for an empty list, a
    bad alpha or ``remove`` and too few kept elements.  The "ALPHA is 1.0" message prints once per call.  ``beam=True``:
    10-tuples, element e equal to ``ltsva_beam`` on the reduced stream (the beam of estimator e's elements at its
    slowness).  ``subsample=True``: the full array's lags are refined once (``ltsva_subsample``) and element e equals
    ``ltsva_subsample`` on the reduced stream.  ``min_velocity`` (km/s, default None): the full array's lags are searched
    within their physical range once (``ltsva_bounded``) and every estimator reads the picks of its pairs.
    ``consistency=True``: element e's tuple is followed by the three returns of ``ltsva_consistency`` on the reduced stream,
    the closure of the lags over the triplets of estimator e's elements."""
    _check_flag('beam', beam)
    _check_flag('subsample', subsample)
    _check_flag('consistency', consistency)
    if min_velocity is not None:
        planner.check_min_velocity(min_velocity)
    data, fs, _ = engine.stream_rows(st)
    nchans = len(data)
    ests = engine.normalize_estimators(estimators, nchans)
    if len(ests) == 1 and not ests[0][1]:          # one estimator with nothing removed IS the single call
        return [_ltsva(st, lat_list, lon_list, window_length, window_overlap, ests[0][0], rij,
                       _plain(bool(beam), bool(subsample), min_velocity, consistency=bool(consistency)))]
    rijs, t0s = [], []
    for _, remove in ests:
        kept = engine.kept_elements(nchans, remove)
        if rij is not None:
            rijs.append(np.ascontiguousarray(np.asarray(rij)[:, kept]) if remove else rij)
        else:
            rijs.append(get_rij([lat_list[i] for i in kept], [lon_list[i] for i in kept], len(kept)))
        t0s.append(engine.stream_rows([st[kept[0]]])[2])
    if all(rm for _, rm in ests):
        rijs.append(get_rij(lat_list, lon_list, nchans) if rij is None else rij)
    if any(a == 1.0 for a, _ in ests):
        print(OLS_MESSAGE)
    results = engine.process_multi(data, fs, t0s, rijs, [(None, None)], [window_length], window_overlap, ests,
                                   prefiltered=True, want_uncert=True, want_beam=bool(beam), want_subsample=bool(subsample),
                                   min_velocity=min_velocity, want_consistency=bool(consistency))
    keys = {}
    out = []
    for (alpha, _), res in zip(ests, results):
        if alpha != 1.0 and id(res.t) not in keys:
            keys[id(res.t)] = engine.time_keys(res.t, res.nwin)
        out.append((_returns_beam if beam else _returns)(res, res.nchans, alpha, keys.get(id(res.t))) +
                   (_returns_consistency(res) if consistency else ()))
    return out


def _returns_kept(res, nchans, beam, capon_kw, band=0, n=None):
    """A band's kept-element results as a dict: ``dropped_elements`` (bool, one column per element, from the bits of the
    mask), ``kept_count`` and, where the pass formed them, ``beam_power`` / ``fstat`` and the fields of ``_returns_capon``
    (csrc/kept.hip, csrc/beam.hip, csrc/capon.hip).  ``band`` / ``n`` as for ``_returns_capon``."""
    pick = _picker(band, n)
    mask = pick(res.dropped_mask)
    out = dict(dropped_elements=((mask[..., None] >> np.arange(nchans, dtype=np.uint32)) & 1).astype(bool),
               kept_count=pick(res.kept_count))
    if beam:
        out['beam_power'], out['fstat'] = pick(res.beam_power), pick(res.fstat)
    if capon_kw:
        out.update(_returns_capon(res, capon_kw['capon_grid'], capon_kw['want_capon_maps'], band=band, n=n))
    return out


def _kept(window_length, window_overlap, min_pairs, beam, slowness_grid, freq, snapshots, loading, maps, peaks, peak_floor):
    """The feature behind the arguments of ``ltsva_kept``."""
    def keywords(nchans, alpha, rij, fs, npts):
        if slowness_grid is None and (freq is not None or snapshots is not None or maps or peaks):
            raise ValueError('freq, snapshots, maps and peaks need slowness_grid')
        if slowness_grid is not None and freq is None:
            raise ValueError('slowness_grid needs freq, the frequency in Hz at which the spectra are formed')
        q, kb, kc = planner.check_kept(nchans, min_pairs, beam, slowness_grid is not None)
        ckw = {} if slowness_grid is None else _capon_keywords(nchans, rij, fs, _window(npts, fs, window_length, window_overlap),
                                                                slowness_grid, freq, snapshots, loading, maps, peaks, peak_floor)
        return dict(ckw, want_beam=kb, kept=(q, kb, kc))

    def tail(res, kw, nchans, fs, t0):
        return (_returns_kept(res, nchans, kw['want_beam'], kw if 'capon_grid' in kw else {}, n=int(res.nwin[0])),)
    return _Feature(keywords, tail)


def _kept_request(nchans, kept, min_pairs, beam=False, capon=False):
    """``kept`` / ``min_pairs`` of the entry points that form their own result over the kept elements -> the ``kept`` keyword of
    ``engine.process`` (``planner.check_kept``), None without ``kept``.  ``ValueError`` before any GPU work."""
    _check_flag('kept', kept)
    if min_pairs is not None and not kept:
        raise ValueError('min_pairs needs kept=True')
    return planner.check_kept(nchans, min_pairs, beam, capon) if kept else None


def ltsva_kept(st, lat_list, lon_list, window_length, window_overlap, alpha=1.0, rij=None, min_pairs=None, beam=True,
               slowness_grid=None, freq=None, snapshots=None, loading=0.01, maps=False, peaks=0, peak_floor=0.25):
    """``ltsva`` followed by the results of the elements FAST-LTS kept: per window, an element at least ``min_pairs`` of
    whose N - 1 pairs have lost their weight (default: all of them) counts as dropped, and the beam of ``ltsva_beam``
    (``beam=True``) and, with ``slowness_grid`` (G, 2) s/km and ``freq`` Hz, the Capon and Bartlett spectra of ``ltsva_capon``
    (its keywords ``snapshots``, ``loading``, ``maps``, ``peaks``, ``peak_floor``) are formed over the other elements — the
    whole array where fewer than 3 would remain (DESIGN.md section 20 has the definition and the counts).  A mistimed element
    costs the full-array beam its F and makes the full-array Capon beamformer null the signal itself; without the element
    both recover.  Returns ``ltsva``'s 8-tuple followed by one dict: ``dropped_elements`` (nwin, N) bool, ``kept_count``
    (nwin,) int32, with ``beam`` ``beam_power`` / ``fstat`` (nwin,), with the grid the fields of ``ltsva_capon``'s dict.  With
    ``alpha == 1.0`` nothing is dropped and every field is that of ``ltsva_beam`` / ``ltsva_capon``.  All of it is computed on
    the GPU behind each window's solve (csrc/kept.hip).  Whatever the library would refuse raises ``ValueError`` before any
    GPU work."""
    return _ltsva(st, lat_list, lon_list, window_length, window_overlap, alpha, rij, _kept(
        window_length, window_overlap, min_pairs, beam, slowness_grid, freq, snapshots, loading, maps, peaks, peak_floor))


def ltsva_kept_batch(streams, lat_list, lon_list, window_length, window_overlap, alpha=1.0, rij=None, min_pairs=None,
                     beam=True, slowness_grid=None, freq=None, snapshots=None, loading=0.01, maps=False, peaks=0,
                     peak_floor=0.25):
    """``ltsva_kept`` over several (already filtered) recordings of ONE array in one GPU pass -> a list of its 9-tuples,
    element i equal to ``ltsva_kept(streams[i], ...)``; the streams as for ``ltsva_batch``."""
    return _ltsva_batch(streams, lat_list, lon_list, window_length, window_overlap, alpha, rij, _kept(
        window_length, window_overlap, min_pairs, beam, slowness_grid, freq, snapshots, loading, maps, peaks, peak_floor))


def ltsva_beam_trace(st, lat_list, lon_list, window_length, window_overlap, alpha=1.0, rij=None, mdccm_min=None, window='hann',
                     kept=False, min_pairs=None):
    """``ltsva`` followed by the waveform its numbers describe: the beam trace (npts,), the delay-and-sum beam steered, window
    by window, at the slowness the window solved — the elements shifted by whole samples against element 0, as in
    ``ltsva_beam`` — and the overlapping windows stitched with the synthesis window ``window`` (``'hann'``: sin^2, ``'boxcar'``:
    the plain average, or the W values themselves; ``planner.beam_trace_window``).  ``mdccm_min``: only windows whose MdCCM
    reaches it enter the trace; samples no accepted window covers are 0.0.  ``kept=True`` (LTS, ``alpha < 1``): every window
    is summed over the elements FAST-LTS kept in it (``ltsva_kept``; ``min_pairs`` as there) and divided by their count, the
    time base still element 0's.  DESIGN.md section 21 has the definition.  The trace is formed on the GPU behind the last
    solve, from the filtered samples already there (csrc/beam_trace.hip): 1/N of the data a host-side beam would have to
    fetch.  Returns ``ltsva``'s 8-tuple followed by the trace.  Whatever the library would refuse raises ``ValueError``
    before any GPU work."""
    return _ltsva(st, lat_list, lon_list, window_length, window_overlap, alpha, rij,
                  _beam_trace(window_length, window_overlap, mdccm_min, window, kept, min_pairs))


def _beam_trace(window_length, window_overlap, mdccm_min, window, kept, min_pairs):
    """The feature behind the arguments of ``ltsva_beam_trace``."""
    def keywords(nchans, alpha, rij, fs, npts):
        kept_kw = _kept_request(nchans, kept, min_pairs)
        want = dict(window=window, mdccm_min=mdccm_min, kept=bool(kept))
        engine._check_beam_trace(want, [_window(npts, fs, window_length, window_overlap)], kept_kw)
        return dict(kept=kept_kw, want_beam_trace=want)
    return _Feature(keywords, lambda res, *_: (res.beam_trace[0].copy(),))


def _steered(taps, slowness_grid, grid_map, subsample, kept, min_pairs):
    """The feature behind the arguments of ``ltsva_steered``."""
    def keywords(nchans, alpha, rij, fs, npts):
        checked = planner.check_steering(taps)
        grid = None if slowness_grid is None else planner.check_slowness_grid(slowness_grid)
        for name, flag in (('grid_map', grid_map), ('subsample', subsample)):
            _check_flag(name, flag)
        if grid_map and grid is None:
            raise ValueError('grid_map needs slowness_grid')
        kept_kw = _kept_request(nchans, kept, min_pairs, beam=True)
        kw = dict(want_beam=True, want_subsample=bool(subsample), slowness_grid=grid, want_grid_map=bool(grid_map), beam_taps=checked)
        return kw if kept_kw is None else dict(kw, kept=kept_kw)

    def tail(res, kw, nchans, fs, t0):
        out = (_returns_kept(res, nchans, True, {}, n=int(res.nwin[0])),) if 'kept' in kw else _beam_tail(res)
        return out if kw['slowness_grid'] is None else out + _returns_grid(res, kw['slowness_grid'], kw['want_grid_map'])
    return _Feature(keywords, tail)


def ltsva_steered(st, lat_list, lon_list, window_length, window_overlap, alpha=1.0, rij=None, taps=8, slowness_grid=None,
                  grid_map=False, subsample=False, kept=False, min_pairs=None):
    """``ltsva_beam`` with the beam steered at fractional-sample delays: every element is read at the delay
    ``fs xij . z`` itself, through a Lagrange interpolator of ``taps`` (4, 6 or 8) samples around ``floor`` of it, where
    ``ltsva_beam`` reads the nearest whole sample (DESIGN.md section 22 has the definition).  On an array whose aperture is a
    few samples of delay the whole-sample beam is piecewise constant in the slowness — many slowness vectors share one row
    of delays — and its maximum a plateau; the interpolated beam is smooth.  ``planner.steering_error(taps, f / fs)`` is the
    interpolator's worst-case error on a sinusoid at f: 8 taps stay below 2.4e-5 up to a tenth of the sampling rate, 4 taps
    below 3.5e-3.  With ``slowness_grid`` (G, 2) s/km the grid search of ``ltsva_grid`` is steered the same way and its five
    (with ``grid_map=True`` six) returns follow; ``subsample=True`` fits the slowness to the refined lags
    (``ltsva_subsample``), so the beam is steered by a continuous estimate; ``kept=True`` forms the beam over the elements
    FAST-LTS kept and returns ``ltsva_kept(beam=True)``'s 9-tuple instead of ``ltsva_beam``'s 10 (``min_pairs`` as there).
    ``taps=0`` is the whole-sample beam.  Computed on the GPU behind each window's solve (csrc/beam.hip, csrc/beam_grid.hip).
    Whatever the library would refuse raises ``ValueError`` before any GPU work."""
    return _ltsva(st, lat_list, lon_list, window_length, window_overlap, alpha, rij,
                  _steered(taps, slowness_grid, grid_map, subsample, kept, min_pairs))


def _grid_refined(slowness_grid, levels, step, taps, grid_map):
    """The feature behind the arguments of ``ltsva_grid_refined``."""
    def keywords(nchans, alpha, rij, fs, npts):
        grid = planner.check_slowness_grid(slowness_grid)
        _check_flag('grid_map', grid_map)
        checked = planner.check_steering(taps)
        refine = planner.check_grid_refinement(levels, step, grid, checked)
        return dict(slowness_grid=grid, want_grid_map=bool(grid_map), beam_taps=checked, grid_refine=refine)

    def tail(res, kw, nchans, fs, t0):
        return _returns_grid(res, kw['slowness_grid'], kw['want_grid_map']) + _returns_grid_refined(res)
    return _Feature(keywords, tail)


def ltsva_grid_refined(st, lat_list, lon_list, window_length, window_overlap, slowness_grid, alpha=1.0, rij=None, levels=4,
                       step=None, taps=8, grid_map=False):
    """``ltsva_grid`` steered at fractional-sample delays (``ltsva_steered``: ``taps`` 4, 6 or 8) with the maximum refined
    between the grid points: from the window's grid maximum, ``levels`` (1..12) times, the best of the centre and its eight
    neighbours at ``step`` (h0, h1) s/km halved per level — by default the lattice step of ``slowness_grid``
    (``planner.grid_cells``) — becomes the new centre (DESIGN.md section 28 has the definition and the counts).  A coarse
    grid then finds the lobe and the search climbs it: a tenth to a quarter of the evaluations of a fine grid and a continuous
    slowness.  The coarse step must not exceed the width of the array's main lobe, or the grid misses it.  Returns
    ``ltsva_grid``'s tuple followed by ``refined_vel``, ``refined_baz`` (the formula of ``grid_slowness``),
    ``refined_slowness`` (nwin, 2) s/km, ``refined_fstat`` (never below ``grid_fstat``), ``refined_power``, ``refined_path``
    (nwin, levels) int32 — the candidate 0..8 chosen on every level, 4 the centre — and ``refined_stencil`` (nwin, 9), the
    nine ratios of the last level; NaN (-1 in the path) where ``grid_index`` is -1.  Computed on the GPU behind each window's
    grid search (csrc/beam_grid_refine.hip).  Whatever the library would refuse raises ``ValueError`` before any GPU work."""
    return _ltsva(st, lat_list, lon_list, window_length, window_overlap, alpha, rij,
                  _grid_refined(slowness_grid, levels, step, taps, grid_map))


def ltsva_grid_refined_batch(streams, lat_list, lon_list, window_length, window_overlap, slowness_grid, alpha=1.0, rij=None,
                             levels=4, step=None, taps=8, grid_map=False):
    """``ltsva_grid_refined`` over several (already filtered) recordings of ONE array in one GPU pass -> a list of its tuples,
    element i equal to ``ltsva_grid_refined(streams[i], ...)`` bit for bit; the streams as for ``ltsva_batch``."""
    return _ltsva_batch(streams, lat_list, lon_list, window_length, window_overlap, alpha, rij,
                        _grid_refined(slowness_grid, levels, step, taps, grid_map))


def ltsva_steered_batch(streams, lat_list, lon_list, window_length, window_overlap, alpha=1.0, rij=None, taps=8,
                        slowness_grid=None, grid_map=False, subsample=False, kept=False, min_pairs=None):
    """``ltsva_steered`` over several (already filtered) recordings of ONE array in one GPU pass -> a list of its tuples,
    element i equal to ``ltsva_steered(streams[i], ...)`` bit for bit; the streams as for ``ltsva_batch``."""
    return _ltsva_batch(streams, lat_list, lon_list, window_length, window_overlap, alpha, rij,
                        _steered(taps, slowness_grid, grid_map, subsample, kept, min_pairs))


def ltsva_beam_trace_batch(streams, lat_list, lon_list, window_length, window_overlap, alpha=1.0, rij=None, mdccm_min=None,
                           window='hann', kept=False, min_pairs=None):
    """``ltsva_beam_trace`` over several (already filtered) recordings of ONE array in one GPU pass -> a list of its 9-tuples,
    element i equal to ``ltsva_beam_trace(streams[i], ...)`` bit for bit; the streams as for ``ltsva_batch``.  (``ltsva_batch``
    and ``ltsva_kept_batch`` keep their signatures: the batch form of the trace is this function.)"""
    return _ltsva_batch(streams, lat_list, lon_list, window_length, window_overlap, alpha, rij,
                        _beam_trace(window_length, window_overlap, mdccm_min, window, kept, min_pairs))


def _element_delays(max_shift, kept, min_pairs):
    """The feature behind the arguments of ``ltsva_element_delays``."""
    def keywords(nchans, alpha, rij, fs, npts):
        kept_kw = _kept_request(nchans, kept, min_pairs)
        if max_shift is None:
            raise ValueError('max_shift is required: an already filtered stream names no band whose upper edge could set the '
                             'shift range (planner.element_shifts(fmax, fs) makes one)')
        shifts = engine._check_element_delays(max_shift, bool(kept), 1, nchans, kept_kw)
        return dict(kept=kept_kw, element_max_shift=shifts, element_delays_kept=bool(kept))

    def tail(res, kw, nchans, fs, t0):
        n = int(res.nwin[0])
        fields = ('element_delay', 'element_cc', 'element_shift') + (('dropped_mask', 'kept_count') if kept else ())
        return tuple(getattr(res, k)[0, :n].copy() for k in fields)
    return _Feature(keywords, tail)


def ltsva_element_delays(st, lat_list, lon_list, window_length, window_overlap, alpha=1.0, rij=None, max_shift=None, kept=False,
                         min_pairs=None):
    """``ltsva`` followed by each element's delay against the beam of the others: per window and element the shift, within
    ``max_shift`` samples (0..256; ``planner.element_shifts(fmax, fs)`` gives half a period of the band's upper edge) either
    side of the delay the solved slowness predicts, at which the element correlates best with the sum of the other
    elements steered at that slowness.  Returns ``ltsva``'s 8-tuple followed by ``element_delay`` (nwin, N) in seconds —
    the shift plus a parabola fraction, positive where the element records the beam's waveform later than the plane wave
    predicts: a clock step, or the station static of a healthy array —, ``element_cc`` (nwin, N), the normalised
    correlation there, and ``element_shift`` (nwin, N) int32.  ``kept=True`` (LTS, ``alpha < 1``): the beam is summed over
    the elements FAST-LTS kept in the window (``ltsva_kept``; ``min_pairs`` as there), so a dropped element is measured
    against a beam it has not biased, and ``dropped_mask`` (nwin,) uint32 and ``kept_count`` (nwin,) int32 follow.  The
    stream is already filtered and names no band, so ``max_shift`` is required.  DESIGN.md section 23 has the definition;
    computed on the GPU behind each window's solve (csrc/element_delay.hip).  Whatever the library would refuse raises
    ``ValueError`` before any GPU work."""
    return _ltsva(st, lat_list, lon_list, window_length, window_overlap, alpha, rij, _element_delays(max_shift, kept, min_pairs))


def ltsva_element_delays_batch(streams, lat_list, lon_list, window_length, window_overlap, alpha=1.0, rij=None, max_shift=None,
                               kept=False, min_pairs=None):
    """``ltsva_element_delays`` over several (already filtered) recordings of ONE array in one GPU pass -> a list of its
    tuples, element i equal to ``ltsva_element_delays(streams[i], ...)`` bit for bit; the streams as for ``ltsva_batch``."""
    return _ltsva_batch(streams, lat_list, lon_list, window_length, window_overlap, alpha, rij,
                        _element_delays(max_shift, kept, min_pairs))


def clean_map(index, power, count, G):
    """The CLEAN-SC components of ``Handle.fetch_capon_clean`` as a map: ``index`` / ``power`` (..., I) and ``count`` (...) ->
    float64 (..., G), every window's ranks below its ``count`` scatter-added onto the grid (components that share a grid
    point add up); zeros elsewhere."""
    index, power, count = np.asarray(index), np.asarray(power, dtype=np.float64), np.asarray(count)
    out = np.zeros(count.shape + (int(G),))
    flat, idx, pw = out.reshape(-1, int(G)), index.reshape(-1, index.shape[-1]), power.reshape(-1, index.shape[-1])
    for w, c in enumerate(count.reshape(-1)):
        np.add.at(flat[w], idx[w, :c], pw[w, :c])
    return out


def clean_sources(index, power, count, grid, radius, max_sources):
    """The CLEAN-SC components of every window merged into sources -> (source_power (..., S), source_slowness (..., S, 2),
    source_vel (..., S), source_baz (..., S)) with S = ``max_sources``.  Per window: the strongest component not merged yet
    (of equal ones the lower rank) takes every unmerged component within ``radius`` s/km of its grid point; the source's power
    is their sum, its slowness their power-weighted mean, velocity and back-azimuth by the formula of ``grid_slowness``;
    again on what is left, up to S sources in the order they are found.  NaN beyond the sources a window has."""
    index, power, count = np.asarray(index), np.asarray(power, dtype=np.float64), np.asarray(count)
    grid, S = np.asarray(grid, dtype=np.float64), int(max_sources)
    spw = np.full(count.shape + (S,), np.nan)
    ssl = np.full(count.shape + (S, 2), np.nan)
    fpw, fsl = spw.reshape(-1, S), ssl.reshape(-1, S, 2)
    idx, pw = index.reshape(-1, index.shape[-1]), power.reshape(-1, index.shape[-1])
    for w, c in enumerate(count.reshape(-1)):
        s, p = grid[idx[w, :c]], pw[w, :c]
        free = np.ones(int(c), dtype=bool)
        for k in range(S):
            if not free.any():
                break
            lead = int(np.flatnonzero(free)[np.argmax(p[free])])
            take = free & (np.hypot(s[:, 0] - s[lead, 0], s[:, 1] - s[lead, 1]) <= radius)
            fpw[w, k] = p[take].sum()
            fsl[w, k] = (s[take] * p[take, None]).sum(axis=0) / fpw[w, k]
            free &= ~take
    with np.errstate(divide='ignore', invalid='ignore'):
        vel = 1.0 / np.hypot(ssl[..., 0], ssl[..., 1])
    baz = np.mod(np.arctan2(ssl[..., 0], ssl[..., 1]) * 180.0 / np.pi - 360.0, 360.0)
    return spw, ssl, vel, baz


def _check_clean_sources(grid, merge_radius, max_sources):
    """``merge_radius`` / ``max_sources`` of the CLEAN-SC entry points -> (the radius in s/km, default 1.5 steps of the lattice
    of ``grid``, max_sources); ``ValueError`` before any GPU work."""
    if isinstance(max_sources, (bool, np.bool_)) or not isinstance(max_sources, (int, np.integer)) or int(max_sources) < 1:
        raise ValueError('max_sources must be a positive integer, not %r' % (max_sources,))
    if merge_radius is None:
        merge_radius = 1.5 * float(np.max(planner.grid_cells(grid)[1]))
    elif not planner._real(merge_radius) or not (0.0 <= float(merge_radius) < np.inf):
        raise ValueError('merge_radius must be a finite number >= 0 (s/km), not %r' % (merge_radius,))
    return float(merge_radius), int(max_sources)


def _clean(window_length, window_overlap, slowness_grid, freq, snapshots, iterations, gain, floor, kept, min_pairs, merge_radius,
           max_sources):
    """The feature behind the arguments of ``ltsva_clean``."""
    def keywords(nchans, alpha, rij, fs, npts):
        kept_kw = _kept_request(nchans, kept, min_pairs, capon=True)
        kw = _capon_keywords(nchans, rij, fs, _window(npts, fs, window_length, window_overlap), slowness_grid, freq, snapshots, 0.01,
                             False)
        kw['capon_clean'] = planner.check_capon_clean(iterations, gain, floor, False)
        if kept_kw is not None:
            kw['kept'] = kept_kw
        sources[:] = _check_clean_sources(kw['capon_grid'], merge_radius, max_sources)
        return kw

    def tail(res, kw, nchans, fs, t0):
        return (_returns_clean(res, kw['capon_grid'], *sources, n=int(res.nwin[0])),)
    sources = []               # (merge radius, max_sources): checked once per call, beside the keywords
    return _Feature(keywords, tail)


def _returns_clean(res, grid, radius, max_sources, band=0, n=None):
    """A band's CLEAN-SC results as a dict: the fields of ``engine.CLEAN_FIELDS``, the slowness of every component
    (``grid_slowness``), and the merged sources of ``clean_sources`` (csrc/capon_clean.hip: capon_clean_kernel).  ``band`` / ``n``
    as for ``_returns_capon``."""
    pick = _picker(band, n)
    out = {k: pick(getattr(res, k)) for k in engine.CLEAN_FIELDS}
    if getattr(res, 'clean_csdm', None) is not None:
        out['clean_csdm'] = pick(res.clean_csdm)
    out['clean_vel'], out['clean_baz'] = grid_slowness(grid, out['clean_index'])
    out['source_power'], out['source_slowness'], out['source_vel'], out['source_baz'] = clean_sources(
        out['clean_index'], out['clean_power'], out['clean_count'], grid, radius, max_sources)
    if getattr(res, 'dropped_mask', None) is not None:
        out['kept_count'] = pick(res.kept_count)
    return out


def ltsva_clean(st, lat_list, lon_list, window_length, window_overlap, slowness_grid, freq, alpha=1.0, rij=None, snapshots=None,
                iterations=16, gain=0.5, floor=0.02, kept=False, min_pairs=None, merge_radius=None, max_sources=4):
    """``ltsva`` followed by the window's arrivals and their powers by CLEAN-SC (Sijtsma 2007) on the narrow band's
    cross-spectral matrix of ``ltsva_capon`` (``slowness_grid`` (G, 2) s/km, ``freq`` Hz, ``snapshots``): up to ``iterations``
    (1..32) times the Bartlett maximum of the matrix is taken as a component and ``gain`` of everything coherent with that
    beam removed — sidelobes leave with their source — until a maximum falls below ``floor`` times the first (DESIGN.md
    section 24 has the definition and the counts).  ``kept=True``: on the elements FAST-LTS kept (``min_pairs`` as for
    ``ltsva_kept``).  Returns ``ltsva``'s 8-tuple followed by one dict: ``clean_count`` (nwin,) int32, ``clean_index`` (nwin, I)
    int32 and ``clean_power`` (nwin, I) (-1 / NaN beyond the count), ``clean_vel`` / ``clean_baz`` (``grid_slowness``),
    ``clean_total`` and ``clean_residual`` (nwin,), the mean element power before and after, and the components merged into
    sources by ``clean_sources`` within ``merge_radius`` s/km (default: 1.5 steps of the grid's lattice): ``source_power``
    (nwin, max_sources), ``source_slowness`` (.., 2), ``source_vel``, ``source_baz``.  Computed on the GPU behind each window's
    solve (csrc/capon_clean.hip).  Whatever the library would refuse raises ``ValueError`` before any GPU work."""
    return _ltsva(st, lat_list, lon_list, window_length, window_overlap, alpha, rij, _clean(
        window_length, window_overlap, slowness_grid, freq, snapshots, iterations, gain, floor, kept, min_pairs, merge_radius, max_sources))


def ltsva_clean_batch(streams, lat_list, lon_list, window_length, window_overlap, slowness_grid, freq, alpha=1.0, rij=None,
                      snapshots=None, iterations=16, gain=0.5, floor=0.02, kept=False, min_pairs=None, merge_radius=None,
                      max_sources=4):
    """``ltsva_clean`` over several (already filtered) recordings of ONE array in one GPU pass -> a list of its 9-tuples,
    element i equal to ``ltsva_clean(streams[i], ...)``; the streams as for ``ltsva_batch``."""
    return _ltsva_batch(streams, lat_list, lon_list, window_length, window_overlap, alpha, rij, _clean(
        window_length, window_overlap, slowness_grid, freq, snapshots, iterations, gain, floor, kept, min_pairs, merge_radius, max_sources))


def _music(window_length, window_overlap, slowness_grid, freq, snapshots, sources, eig_floor, maps, vectors, peaks, peak_floor):
    """The feature behind the arguments of ``ltsva_music``."""
    def keywords(nchans, alpha, rij, fs, npts):
        kw = _capon_keywords(nchans, rij, fs, _window(npts, fs, window_length, window_overlap), slowness_grid, freq, snapshots, 0.01,
                             False, peaks)
        kw['capon_music'] = planner.check_capon_music(nchans, sources, eig_floor, maps, vectors, 'capon_peaks' in kw, peak_floor)
        return kw
    return _Feature(keywords, lambda res, kw, *_: (_returns_music(res, kw['capon_grid'], n=int(res.nwin[0])),))


def _returns_music(res, grid, band=0, n=None):
    """A band's MUSIC results as a dict: the fields of ``engine.MUSIC_FIELDS``, the slowness of the spectrum's maximum
    (``grid_slowness``) and, where the pass kept them, ``music_map``, ``music_vectors`` and the peaks' four fields with the refined
    slowness of every rank (``peak_slowness``) (csrc/capon_music.hip: capon_music_kernel).  ``band`` / ``n`` as for ``_returns_capon``."""
    pick = _picker(band, n)
    out = {k: pick(getattr(res, k)) for k in engine.MUSIC_FIELDS}
    for k in ('music_map', 'music_vectors'):
        if getattr(res, k, None) is not None:
            out[k] = pick(getattr(res, k))
    out['music_vel'], out['music_baz'] = grid_slowness(grid, out['music_index'])
    if getattr(res, 'music_peak_count', None) is not None:
        for field in engine.PEAK_FIELDS:
            out['music' + field] = pick(getattr(res, 'music' + field))
        out['music_peak_slowness'], out['music_peak_vel'], out['music_peak_baz'] = peak_slowness(
            grid, planner.grid_cells(grid)[1], out['music_peak_index'], out['music_peak_offset'])
    return out


def ltsva_music(st, lat_list, lon_list, window_length, window_overlap, slowness_grid, freq, alpha=1.0, rij=None, snapshots=None,
                sources=0, eig_floor=0.05, maps=False, vectors=False, peaks=0, peak_floor=0.0):
    """``ltsva`` followed by the eigenvalues of every window's narrow-band cross-spectral matrix and its MUSIC pseudo-spectrum
    (Schmidt 1986) over ``slowness_grid`` (G, 2) s/km at ``freq`` Hz (``snapshots`` as for ``ltsva_capon``): the matrix is
    decomposed by a cyclic Jacobi method, the ``sources`` = M strongest eigenvectors span the signals — ``sources=0``: as many
    as there are eigenvalues of at least ``eig_floor`` times the largest — and P(g) = N / sum_{k > M} |e_k^H a(g)|^2 peaks
    where a steering vector is orthogonal to the others (DESIGN.md section 25 has the definition, the error bounds and the
    counts).  Returns ``ltsva``'s 8-tuple followed by one dict: ``music_eigenvalues`` (nwin, N) descending, ``music_sources``,
    ``music_sweeps`` and ``music_index`` (nwin,) int32, ``music_power`` (nwin,), ``music_vel`` / ``music_baz``
    (``grid_slowness``), with ``maps`` ``music_map`` (nwin, G) and with ``vectors`` ``music_vectors`` (nwin, N, N) complex,
    column k beside eigenvalue k; with ``peaks`` = K in 1..8 the K strongest local maxima of the pseudo-spectrum that reach
    ``peak_floor`` times its maximum, as ``ltsva_capon`` returns a spectrum's: ``music_peak_count``, ``music_peak_index`` /
    ``_power`` (nwin, K), ``music_peak_offset`` (nwin, K, 2) and the refined ``music_peak_slowness``, ``music_peak_vel``,
    ``music_peak_baz`` (the Capon and Bartlett peaks of the pass are not returned).  Computed on the GPU behind each window's solve (csrc/capon_music.hip).  Whatever the
    library would refuse raises ``ValueError`` before any GPU work."""
    return _ltsva(st, lat_list, lon_list, window_length, window_overlap, alpha, rij, _music(
        window_length, window_overlap, slowness_grid, freq, snapshots, sources, eig_floor, maps, vectors, peaks, peak_floor))


def ltsva_music_batch(streams, lat_list, lon_list, window_length, window_overlap, slowness_grid, freq, alpha=1.0, rij=None,
                      snapshots=None, sources=0, eig_floor=0.05, maps=False, vectors=False, peaks=0, peak_floor=0.0):
    """``ltsva_music`` over several (already filtered) recordings of ONE array in one GPU pass -> a list of its 9-tuples,
    element i equal to ``ltsva_music(streams[i], ...)``; the streams as for ``ltsva_batch``."""
    return _ltsva_batch(streams, lat_list, lon_list, window_length, window_overlap, alpha, rij, _music(
        window_length, window_overlap, slowness_grid, freq, snapshots, sources, eig_floor, maps, vectors, peaks, peak_floor))


def _families(**params):
    """The feature behind the arguments of ``ltsva_families``."""
    def tail(res, kw, nchans, fs, t0):
        n = int(res.nwin[0])
        return res.family[0, :n].copy(), planner.family_table(res.family, res.family_table, res.vel, res.baz, res.mdccm,
                                                              res.sigma_tau, [(np.nan, np.nan)], res.W, res.inc, fs, t0)
    return _Feature(lambda *_: dict(families=planner.check_families(**params)), tail)


def ltsva_families(st, lat_list, lon_list, window_length, window_overlap, alpha=1.0, rij=None, *, mdccm_min, baz_tol, vel_tol,
                   vel_min, vel_max, sigma_tau_max=None, band_reach=1, time_reach=1, min_pixels=4):
    """``ltsva`` followed by ``family_array`` (nwin,) int32 and ``families``: the windows grouped into detections — runs of
    windows at most ``time_reach`` apart that pass the gates (``mdccm_min``, ``vel_min`` .. ``vel_max``, ``sigma_tau_max``) and
    agree with their neighbours within ``baz_tol`` degrees and ``vel_tol`` km/s, at least ``min_pixels`` windows long;
    ``narrow_band_least_squares_families`` has the details (one band here: ``band_reach`` plays no part; ``f_lo`` / ``f_hi``
    are NaN), DESIGN.md section 26 the definition.  ``ValueError`` before any GPU work for what the library refuses."""
    return _ltsva(st, lat_list, lon_list, window_length, window_overlap, alpha, rij, _families(
        mdccm_min=mdccm_min, baz_tol=baz_tol, vel_tol=vel_tol, vel_min=vel_min, vel_max=vel_max, sigma_tau_max=sigma_tau_max,
        band_reach=band_reach, time_reach=time_reach, min_pixels=min_pixels))


def ltsva_families_batch(streams, lat_list, lon_list, window_length, window_overlap, alpha=1.0, rij=None, *, mdccm_min, baz_tol,
                         vel_tol, vel_min, vel_max, sigma_tau_max=None, band_reach=1, time_reach=1, min_pixels=4):
    """``ltsva_families`` over several (already filtered) recordings of ONE array in one GPU pass -> a list of its 10-tuples,
    element i equal to ``ltsva_families(streams[i], ...)``; the streams as for ``ltsva_batch``."""
    params = dict(mdccm_min=mdccm_min, baz_tol=baz_tol, vel_tol=vel_tol, vel_min=vel_min, vel_max=vel_max, sigma_tau_max=sigma_tau_max,
                  band_reach=band_reach, time_reach=time_reach, min_pixels=min_pixels)
    streams = list(streams)
    if not streams:
        planner.check_families(**params)
    return _ltsva_batch(streams, lat_list, lon_list, window_length, window_overlap, alpha, rij, _families(**params))
