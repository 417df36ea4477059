"""A stand-in for ``engine.process`` / ``process_batch`` / ``process_multi`` and one call per public entry point of
``lts_array`` and ``narrow_band_least_squares``, shared by tests/test_entry_points_host.py.  The stand-in records the
arguments of every engine call, answers with the ``BandBatch`` the real driver would allocate for the call's own requests
(``Requests.check`` -> ``engine.new_result``), filled from a fixed seed, and tells the caller about it as ``process`` does
for one group: ``host_overlap(res)``, then ``units_done`` / ``group_done`` through the driver's own notifier.  N = 5 elements,
601 samples, 2 bands (the recording of tests/requests_cases.py).  CPU only: nothing here opens the GPU library."""
import contextlib
import importlib

import numpy as np

import requests_cases as rc
from narrow_band_least_squares_amd import engine, lts_array as la, synthetic
from narrow_band_least_squares_amd.call_requests import Requests

nb = importlib.import_module('narrow_band_least_squares_amd.narrow_band_least_squares')      # (the package exports the function)

OLS_MESSAGE = 'ALPHA is 1.0. Performing an ordinary least squares fit, NOT least trimmed squares.'
SEED = 20261021
WINLEN, OVERLAP = rc.WINLENS[0], rc.OVERLAP
WINLEN_LIST = [65.5 / rc.FS, 45.5 / rc.FS]           # (the last one sets the row length: 30 cells for 17 and 26 windows)
FREQLIST = [0.5, 1.5, 4.0]
FREQ_RESP = np.logspace(-1, 1, 8)
GRID = rc.GRID
FAMILIES = dict(rc.FAMILIES)


def stream(shift_days=0.0):
    """The recording of tests/requests_cases.py as a stream that starts ``shift_days`` after ``rc.T0``."""
    return synthetic.make_stream(rc.recording()[0], rc.FS, starttime=rc.T0 + shift_days)


def rij():
    return rc.recording()[1]


def _fill(res):
    """Every array of ``res`` from the fixed seed, in the order of the names: floats in (0, 1), whole numbers 0 or 1 (a valid
    grid index, rank, count and shift everywhere), the packed weights any bits."""
    rng = np.random.default_rng(SEED)
    for name in sorted(res.__dict__):
        a = res.__dict__[name]
        if not isinstance(a, np.ndarray) or name in ('nwin', 'pair_idx', 'xij', 't') + engine.GRID_NAMES:
            continue
        if name == 'mask':
            a[...] = rng.integers(0, 256, a.shape)
        elif a.dtype.kind == 'f':
            a[...] = rng.random(a.shape)
        elif a.dtype.kind == 'c':
            a[...] = rng.random(a.shape) + 1j * rng.random(a.shape)
        else:
            a[...] = rng.integers(0, 2, a.shape)


class StandIn:
    """``calls``: (name, positional arguments, keywords) of every engine call; ``results``: every ``BandBatch`` handed out."""

    def __init__(self):
        self.calls, self.results = [], []

    def names(self):
        return [c[0] for c in self.calls]

    def _result(self, nchans, npts, fs, t0, rij_, edges, winlens, winover, alpha, tail, kw, asked, times=None):
        ftype, forder, fripple = (tuple(tail) + (None, None, None))[:3]
        prefiltered = bool(kw.get('prefiltered', False))
        prep = engine.prepare(nchans, npts, fs, rij_, edges, winlens, winover, alpha, ftype, forder, fripple,
                              kw.get('vector_len'), prefiltered)
        req = Requests.check(nchans, len(edges), fs, list(prep.W), rij=rij_, **asked)
        res = engine.new_result(nchans, alpha, fs, prep.W, prep.inc, prep.nwin, prep.vector_len, **req.result_keywords(npts))
        _fill(res)
        if times is None:
            res.t = engine.time_grid(t0, fs, prep.W, prep.inc, prep.nwin, prep.vector_len)
        else:
            res.t = times.setdefault(t0, engine.time_grid(t0, fs, prep.W, prep.inc, prep.nwin, prep.vector_len))
        res.sos, res.pair_idx, res.xij = list(prep.sos_ret), prep.pair_idx, prep.xij
        if req.families is not None:        # one family: the first two cells of band 0
            res.family = np.full(res.vel.shape, -1, dtype=np.int32)
            res.family[0, :2] = 0
            res.family_table = np.array([[2, 0, 0, 0, 0, 0, 0, 100]], dtype=np.int64)
        self.results.append(res)
        return res

    def process(self, data, fs, t0, rij_, edges, winlens, winover, alpha, *tail, host_overlap=None, group_done=None,
                units_done=None, **kw):
        told = {k: v is not None for k, v in dict(host_overlap=host_overlap, group_done=group_done, units_done=units_done).items()
                if v is not None}
        self.calls.append(('process', (data, fs, t0, rij_, edges, winlens, winover, alpha) + tail, dict(kw, **told)))
        res = self._result(len(data), len(data[0]), fs, t0, rij_, edges, winlens, winover, alpha, tail, kw, Requests.keywords_of(kw))
        if host_overlap is not None:
            host_overlap(res)
        note = engine._Notifier(res, units_done, group_done)
        note.ready = True
        note.bands(0, len(edges))
        return res

    def process_batch(self, recordings, fs, t0s, rij_, edges, winlens, winover, alpha, *tail, **kw):
        self.calls.append(('process_batch', (recordings, fs, t0s, rij_, edges, winlens, winover, alpha) + tail, dict(kw)))
        return [self._result(len(rec), len(rec[0]), fs, t0, rij_, edges, winlens, winover, alpha, tail, kw, Requests.keywords_of(kw))
                for rec, t0 in zip(recordings, t0s)]

    def process_multi(self, data, fs, t0s, rijs, edges, winlens, winover, estimators, *tail, host_overlap=None,
                      units_done=None, **kw):
        told = {k: True for k, v in dict(host_overlap=host_overlap, units_done=units_done).items() if v is not None}
        self.calls.append(('process_multi', (data, fs, t0s, rijs, edges, winlens, winover, estimators) + tail, dict(kw, **told)))
        times, results = {}, []
        for (alpha, remove), t0, r in zip(estimators, t0s, rijs):
            results.append(self._result(len(data) - len(remove), len(data[0]), fs, t0, r, edges, winlens, winover, alpha, tail, kw,
                                        Requests.keywords_of(kw), times))
        if host_overlap is not None:
            host_overlap(results)
        if units_done is not None:
            for e, res in enumerate(results):
                units_done(e, res, 0, int(np.sum(res.nwin)))
        return results


@contextlib.contextmanager
def stand_in():
    """The engine's three drivers replaced by one ``StandIn`` for the block, and no device to open."""
    s = StandIn()

    def refuse(*a, **k):
        raise AssertionError('a device was opened')
    saved = {name: getattr(engine, name) for name in ('process', 'process_batch', 'process_multi', 'get_handle')}
    engine.process, engine.process_batch, engine.process_multi, engine.get_handle = s.process, s.process_batch, s.process_multi, refuse
    try:
        yield s
    finally:
        for name, fn in saved.items():
            setattr(engine, name, fn)


def nb_args(st, alpha, rows=len(FREQ_RESP)):
    """The positional arguments of every narrow-band entry point for the stream (or the streams) ``st``; ``rows``: the length
    of the caller's response rows ``w`` and ``h``."""
    return (WINLEN_LIST, OVERLAP, alpha, st, None, None, 2, np.zeros(rows), np.zeros(rows), FREQLIST, 'octave', FREQ_RESP, *rc.FILTER)


def _lt(fn, *more, **kw):
    return lambda st, alpha: fn(st, None, None, WINLEN, OVERLAP, *more, alpha=alpha, rij=rij(), **kw)


def _nb(fn, **kw):
    return lambda st, alpha, rows=len(FREQ_RESP): fn(*nb_args(st, alpha, rows), rij=rij(), **kw)


_BASE = {'prefiltered', 'want_uncert'}
_PLAIN = _BASE | {'want_beam', 'want_subsample', 'min_velocity', 'slowness_grid', 'want_grid_map', 'seed_halfwidths', 'want_consistency'}
_PLAIN_BATCH = _BASE | {'want_beam', 'want_subsample', 'min_velocity', 'slowness_grid'}
_CAPON = {'capon_grid', 'capon_freqs', 'capon_snapshots', 'capon_loading', 'want_capon_maps'}
_NB = {'vector_len', 'want_beam', 'want_subsample', 'min_velocity', 'slowness_grid', 'want_grid_map', 'seed_halfwidths',
       'want_consistency', 'beam_taps'}
_TOLD = {'host_overlap'}
_NB_TOLD = {'host_overlap', 'group_done', 'units_done'}

# name -> (the single form, the batch form or None, the keywords the single form passes to ``engine.process`` beside the
# callbacks, those the batch form passes to ``engine.process_batch``): the keyword sets as the entry points passed them
# before they shared a body
PAIRS = {
    'ltsva': (_lt(la.ltsva), _lt(la.ltsva_batch), _PLAIN, _PLAIN_BATCH),
    'ltsva_beam': (_lt(la.ltsva_beam), _lt(la.ltsva_batch, beam=True), _PLAIN, _PLAIN_BATCH),
    'ltsva_subsample': (_lt(la.ltsva_subsample), _lt(la.ltsva_batch, subsample=True), _PLAIN, _PLAIN_BATCH),
    'ltsva_bounded': (_lt(la.ltsva_bounded, 0.2), _lt(la.ltsva_batch, min_velocity=0.2), _PLAIN, _PLAIN_BATCH),
    'ltsva_grid': (_lt(la.ltsva_grid, GRID), _lt(la.ltsva_batch, slowness_grid=GRID), _PLAIN, _PLAIN_BATCH),
    'ltsva_seeded': (_lt(la.ltsva_seeded, GRID, 4), None, _PLAIN, None),
    'ltsva_consistency': (_lt(la.ltsva_consistency), None, _PLAIN, None),
    'ltsva_capon': (_lt(la.ltsva_capon, GRID, 1.0), _lt(la.ltsva_capon_batch, GRID, 1.0), _PLAIN | _CAPON, _PLAIN_BATCH | _CAPON),
    'ltsva_kept': (_lt(la.ltsva_kept, slowness_grid=GRID, freq=1.0), _lt(la.ltsva_kept_batch, slowness_grid=GRID, freq=1.0),
                   _BASE | _CAPON | {'want_beam', 'kept'}, _BASE | _CAPON | {'want_beam', 'kept'}),
    'ltsva_beam_trace': (_lt(la.ltsva_beam_trace), _lt(la.ltsva_beam_trace_batch),
                         _BASE | {'kept', 'want_beam_trace'}, _BASE | {'kept', 'want_beam_trace'}),
    'ltsva_steered': (_lt(la.ltsva_steered, slowness_grid=GRID), _lt(la.ltsva_steered_batch, slowness_grid=GRID),
                      _BASE | {'want_beam', 'want_subsample', 'slowness_grid', 'want_grid_map', 'beam_taps'},
                      _BASE | {'want_beam', 'want_subsample', 'slowness_grid', 'want_grid_map', 'beam_taps'}),
    'ltsva_element_delays': (_lt(la.ltsva_element_delays, max_shift=3), _lt(la.ltsva_element_delays_batch, max_shift=3),
                             _BASE | {'kept', 'element_max_shift', 'element_delays_kept'},
                             _BASE | {'kept', 'element_max_shift', 'element_delays_kept'}),
    'ltsva_clean': (_lt(la.ltsva_clean, GRID, 1.0, iterations=2), _lt(la.ltsva_clean_batch, GRID, 1.0, iterations=2),
                    _BASE | _CAPON | {'capon_clean'}, _BASE | _CAPON | {'capon_clean'}),
    'ltsva_music': (_lt(la.ltsva_music, GRID, 1.0), _lt(la.ltsva_music_batch, GRID, 1.0),
                    _BASE | _CAPON | {'capon_music'}, _BASE | _CAPON | {'capon_music'}),
    'ltsva_families': (_lt(la.ltsva_families, **FAMILIES), _lt(la.ltsva_families_batch, **FAMILIES),
                       _BASE | {'families'}, _BASE | {'families'}),
    'narrow_band_least_squares': (_nb(nb.narrow_band_least_squares), _nb(nb.narrow_band_least_squares_batch), _NB, {'vector_len'}),
    'narrow_band_least_squares_families': (_nb(nb.narrow_band_least_squares_families, **FAMILIES),
                                           _nb(nb.narrow_band_least_squares_families_batch, **FAMILIES),
                                           _NB | {'families'}, {'vector_len', 'families'}),
}

# the 15 all-band single-stream entry points of the narrow-band module: name -> (the call, the keywords it passes to
# ``engine.process`` beside the callbacks, whether it has an ALPHA range check of its own)
NARROW_BAND = {
    'narrow_band_least_squares': (_nb(nb.narrow_band_least_squares), _NB, False),
    'narrow_band_least_squares_beam': (_nb(nb.narrow_band_least_squares_beam), _NB, True),
    'narrow_band_least_squares_consistency': (_nb(nb.narrow_band_least_squares_consistency), _NB, True),
    'narrow_band_least_squares_subsample': (_nb(nb.narrow_band_least_squares_subsample), _NB, True),
    'narrow_band_least_squares_bounded': (_nb(nb.narrow_band_least_squares_bounded, min_velocity=0.2), _NB, True),
    'narrow_band_least_squares_grid': (_nb(nb.narrow_band_least_squares_grid, slowness_grid=GRID), _NB, True),
    'narrow_band_least_squares_steered': (_nb(nb.narrow_band_least_squares_steered, slowness_grid=GRID), _NB, True),
    'narrow_band_least_squares_capon': (_nb(nb.narrow_band_least_squares_capon, slowness_grid=GRID), _NB | _CAPON, True),
    'narrow_band_least_squares_clean': (_nb(nb.narrow_band_least_squares_clean, slowness_grid=GRID, iterations=2),
                                        _NB | _CAPON | {'capon_clean'}, True),
    'narrow_band_least_squares_music': (_nb(nb.narrow_band_least_squares_music, slowness_grid=GRID), _NB | _CAPON | {'capon_music'}, True),
    'narrow_band_least_squares_kept': (_nb(nb.narrow_band_least_squares_kept, slowness_grid=GRID), _NB | _CAPON | {'kept'}, True),
    'narrow_band_least_squares_seeded': (_nb(nb.narrow_band_least_squares_seeded, slowness_grid=GRID), _NB, True),
    'narrow_band_least_squares_beam_trace': (_nb(nb.narrow_band_least_squares_beam_trace), _NB | {'kept', 'want_beam_trace'}, True),
    'narrow_band_least_squares_element_delays': (_nb(nb.narrow_band_least_squares_element_delays),
                                                 _NB | {'kept', 'element_max_shift', 'element_delays_kept'}, True),
    'narrow_band_least_squares_families': (_nb(nb.narrow_band_least_squares_families, **FAMILIES), _NB | {'families'}, False),
}
ALPHA_MESSAGE = 'ALPHA must be in [0.5, 1.0].'
RESPONSE_MESSAGE = 'could not broadcast filter response of length 8 into rows of length 7'

# some of the keywords' values, as the entry points passed them before they shared a body (alpha 0.75): name -> the values
# the single form passes to ``engine.process``; the batch form passes the same where it passes the keyword at all
VALUES = {
    'ltsva': dict(prefiltered=True, want_uncert=True, want_beam=False, want_subsample=False, want_grid_map=False, want_consistency=False),
    'ltsva_beam': dict(want_beam=True, want_subsample=False, min_velocity=None, want_grid_map=False, want_consistency=False),
    'ltsva_subsample': dict(want_beam=False, want_subsample=True, min_velocity=None, want_grid_map=False),
    'ltsva_bounded': dict(want_beam=False, want_subsample=False, min_velocity=0.2),
    'ltsva_consistency': dict(want_beam=False, want_subsample=False, want_consistency=True),
    'ltsva_steered': dict(want_beam=True, want_subsample=False, want_grid_map=False, beam_taps=8),
    'ltsva_kept': dict(want_beam=True, kept=(4, True, True)),
    'ltsva_beam_trace': dict(kept=None),
    'ltsva_element_delays': dict(kept=None, element_delays_kept=False),
    'narrow_band_least_squares': dict(vector_len=30, want_beam=False, want_subsample=False, want_consistency=False, beam_taps=0),
    'narrow_band_least_squares_beam': dict(vector_len=30, want_beam=True, want_subsample=False, beam_taps=0),
    'narrow_band_least_squares_consistency': dict(want_beam=False, want_subsample=False, want_consistency=True),
    'narrow_band_least_squares_steered': dict(want_beam=True, want_subsample=False, want_grid_map=False, beam_taps=8),
    'narrow_band_least_squares_kept': dict(want_beam=True, beam_taps=0, kept=(4, True, True)),
}
