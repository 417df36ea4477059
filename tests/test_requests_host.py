"""The record of a call's opt-in requests (``call_requests.Requests``) and the table of result groups against a stand-in
handle that records its calls: what ``launch`` sets and unsets around a plan on every way out, that every field of a pass
arrives in the right rows of the right recording, which ``Handle`` calls a pass makes, and the refusals of the
time-segmented path.  The call is that of tests/requests_cases.py.  CPU only, no GPU library."""
import numpy as np
import pytest

import requests_cases as rc
import scale_cases as sc
from narrow_band_least_squares_amd import engine
from narrow_band_least_squares_amd.call_requests import Requests

F8, I4, U4, C16 = np.float64, np.int32, np.uint32, np.complex128
N, G, K, I, VL = rc.N, len(rc.GRID), rc.PEAKS, rc.ITERATIONS, rc.VECTOR_LEN
P = N * (N - 1) // 2
_PEAK = (('_peak_count', (), I4), ('_peak_index', (K,), I4), ('_peak_power', (K,), F8), ('_peak_offset', (K, 2), F8))

# what every fetch of ``_hip.Handle`` returns (its docstrings), written out here on its own: (field, trailing shape, dtype)
RETURNS = {
    'fetch_uncertainty': (('vel_uncert', (), F8), ('baz_uncert', (), F8)),
    'fetch_beam': (('beam_power', (), F8), ('fstat', (), F8)),
    'fetch_closure': (('consistency', (), F8), ('closure_max', (), F8), ('element_consistency', (N,), F8)),
    'fetch_lag_fraction': (('lag_frac', (P,), F8),),
    'fetch_beam_grid': (('grid_index', (), I4), ('grid_fstat', (), F8), ('grid_power', (), F8)),
    'fetch_beam_grid_map': (('grid_map', (G,), F8),),
    'fetch_capon': (('capon_index', (), I4), ('capon_power', (), F8), ('bartlett_index', (), I4), ('bartlett_power', (), F8)),
    'fetch_capon_maps': (('capon_map', (G,), F8), ('bartlett_map', (G,), F8)),
    'fetch_capon_csdm': (('capon_csdm', (N, N), C16),),
    'fetch_capon_peaks': None,                                 # (by its argument, below)
    'fetch_capon_clean': (('clean_count', (), I4), ('clean_index', (I,), I4), ('clean_power', (I,), F8), ('clean_total', (), F8),
                          ('clean_residual', (), F8)),
    'fetch_capon_clean_csdm': (('clean_csdm', (N, N), C16),),
    'fetch_capon_music': (('music_eigenvalues', (N,), F8), ('music_sources', (), I4), ('music_sweeps', (), I4),
                          ('music_index', (), I4), ('music_power', (), F8)),
    'fetch_capon_music_map': (('music_map', (G,), F8),),
    'fetch_capon_music_vectors': (('music_vectors', (N, N), C16),),
    'fetch_capon_music_peaks': tuple(('music' + f, t, d) for f, t, d in _PEAK),
    'fetch_kept_elements': (('dropped_mask', (), U4), ('kept_count', (), I4)),
    'fetch_element_delays': (('element_delay', (N,), F8), ('element_cc', (N,), F8), ('element_shift', (N,), I4)),
}
BARE = {m for m, r in RETURNS.items() if r is not None and len(r) == 1}      # one array, not a tuple of them
FETCHED = {'lag': ((P,), I4), 'cmax': ((P,), F8), 'z': ((2,), F8)}           # the planes of ``Handle.fetch``
PER_ESTIMATOR = ('fetch_uncertainty', 'fetch_beam', 'fetch_closure', 'fetch_lag_fraction')

# every array of a pass but its result block, by tests/scale_cases.py; each gets a constant of its own
BROUGHT = sorted(set(sc.batch_fields()[0]) - set(sc.CONFIG) - {'grids', 'mask', 'weights', 'family', 'family_table'}
                 - set(engine.GRID_NAMES))
CONST = {name: 3 + i for i, name in enumerate(BROUGHT)}


class Refused(RuntimeError):
    pass


class StubHandle:
    """Logs every call as (name, args, kwargs).  ``rows``: the result rows of its pass; a fetch fills row r of a field with
    the field's constant + 100 r.  ``refuse``: the first call of that method raises ``Refused``."""
    est_npairs = None
    profiling = False

    def __init__(self, rows=1, refuse=None):
        self.rows, self.refuse, self.log = rows, refuse, []

    def names(self):
        return [name for name, _, _ in self.log]

    def _array(self, name, trailing, dtype):
        a = np.empty((self.rows, VL) + trailing, dtype=dtype)
        a[...] = (CONST[name] + 100 * np.arange(self.rows)).reshape((-1,) + (1,) * (a.ndim - 1))
        return a

    def _answer(self, name, args, kw):
        if name == 'fetch':
            return {k[len('want_'):]: self._array(k[len('want_'):], *FETCHED[k[len('want_'):]]) for k, v in kw.items()
                    if k.startswith('want_') and v}
        if name == 'fetch_beam_trace':
            return np.full(rc.NPTS, CONST['beam_trace'] + 100.0 * args[0])
        if name == 'fetch_families':               # family s holds every cell of recording s (row r = b * k + s)
            k = self.families_of
            family = np.repeat(np.arange(self.rows, dtype=np.int32) % k, VL).reshape(self.rows, VL)
            table = np.zeros((k, 8), dtype=np.int64)
            table[:, 5] = np.arange(k)
            return family, k, table
        if name == 'fetch_packed':
            z = np.zeros((self.rows, VL))
            return dict(vel=z, baz=z, mdccm=z, sigma_tau=z, mask=np.zeros((self.rows, VL, (P + 7) // 8), dtype=np.uint8))
        if name.startswith('fetch_'):
            fields = RETURNS[name]
            if name == 'fetch_capon_peaks':
                fields = tuple((('capon', 'bartlett')[args[0]] + f, t, d) for f, t, d in _PEAK)
            out = tuple(self._array(*f) for f in fields)
            return out[0] if name in BARE else out
        return None

    def __getattr__(self, name):
        if name.startswith('_'):
            raise AttributeError(name)

        def call(*args, **kw):
            self.log.append((name, args, kw))
            if name == self.refuse:
                self.refuse = None
                raise Refused(name)
            return self._answer(name, args, kw)
        return call


def _prep():
    data, rij = rc.recording()
    return engine.prepare(N, rc.NPTS, rc.FS, rij, rc.EDGES, rc.WINLENS, rc.OVERLAP, rc.ALPHA, *rc.FILTER)


def _all_on(**more):
    return Requests.check(N, 2, rc.FS, list(rc.WINDOWS), rij=rc.recording()[1], **dict(rc.ALL_ON, **more))


# ---- 1. what a launch sets and unsets ----------------------------------------------------------------------------------
# the order in which ``launch`` has always called the setters, and the order and the arguments with which it switches them off
SET_ORDER = ('set_beam', 'set_closure', 'set_lag_refinement', 'set_lag_limits', 'set_beam_grid', 'set_lag_seed',
             'set_beam_interpolation', 'set_kept_elements', 'set_element_delays', 'set_beam_trace', 'set_capon', 'set_capon_peaks',
             'set_capon_clean', 'set_capon_music', 'set_families')
UNSET = (('set_beam', (False,)), ('set_closure', (False,)), ('set_lag_refinement', (False,)), ('set_lag_limits', (None,)),
         ('set_beam_grid', (None,)), ('set_lag_seed', (None,)), ('set_beam_interpolation', (0,)), ('set_capon', (None,)),
         ('set_capon_peaks', (None,)), ('set_capon_clean', (0,)), ('set_capon_music', (None,)), ('set_families', (None,)),
         ('set_kept_elements', (0,)), ('set_element_delays', (None,)), ('set_beam_trace', (None,)))
# each request alone: the attributes of the everything-on record (``lag_limits``: of a call with ``min_velocity``) that make
# it, and the setters it calls
ALONE = {
    'beam': (('beam',), ('set_beam',)), 'closure': (('closure',), ('set_closure',)), 'subsample': (('subsample',), ('set_lag_refinement',)),
    'lag_limits': (('lag_limits',), ('set_lag_limits',)), 'beam_grid': (('beam_grid', 'beam_grid_map'), ('set_beam_grid',)),
    'lag_seed': (('lag_seed',), ('set_lag_seed',)), 'beam_taps': (('beam_taps',), ('set_beam_interpolation',)),
    'kept': (('kept',), ('set_kept_elements',)), 'element_delays': (('element_delays', 'element_delays_kept'), ('set_element_delays',)),
    'beam_trace': (('beam_trace',), ('set_beam_trace',)), 'capon': (('capon',), ('set_capon', 'set_capon_peaks')),
    'capon_clean': (('capon_clean',), ('set_capon_clean',)), 'capon_music': (('capon_music',), ('set_capon_music',)),
    'families': (('families',), ('set_families',)),
}


def _launch(req, h, **kw):
    """Band 1 of the two-band Prep, on a handle that has its trace and geometry."""
    engine.launch(h, None, _prep(), bands=[1], upload=False, requests=req, **kw)


def _around_plan(h):
    """The log between ``set_uncertainty`` and ``stream_results`` (or its end), cut at the plan -> (sets, unsets)."""
    names = h.names()
    start = names.index('set_uncertainty') + 1
    stop = names.index('stream_results') if 'stream_results' in names else len(names)
    calls = h.log[start:stop]
    at = [n for n, _, _ in calls].index('plan')
    return calls[:at], calls[at + 1:]


def _check_unsets(sets, unsets, refused=None):
    done = [n for n, _, _ in sets if n != refused]
    assert [(n, a) for n, a, kw in unsets] == [u for u in UNSET if u[0] in done], (done, unsets)
    assert all(not kw for _, _, kw in unsets)


def _check_band_1_tables(sets, req):
    """The per-band tables in the logged arguments are those of band 1 alone."""
    by = {n: (a, kw) for n, a, kw in sets}
    if 'set_lag_seed' in by:
        assert [int(v) for v in by['set_lag_seed'][0][0]] == rc.SEED_HALFWIDTHS[1:]
    if 'set_element_delays' in by:
        a = by['set_element_delays'][0]
        assert [int(v) for v in a[0]] == rc.SHIFTS[1:] and a[1] is req.element_delays_kept
    if 'set_beam_trace' in by:
        window, gate, kept = by['set_beam_trace'][0]
        assert len(window) == rc.WINDOWS[1] and gate is None and kept is True
        np.testing.assert_array_equal(window, req.beam_trace[0][1])
    if 'set_capon' in by:
        a, kw = by['set_capon']
        assert not a and sorted(kw) == ['freqs', 'grid', 'loading', 'snap_hop', 'snap_len', 'want_csdm', 'want_maps']
        assert [float(v) for v in kw['freqs']] == [float(rc.ALL_ON['capon_freqs'][1])]
        assert [int(v) for v in kw['snap_len']] == rc.SNAPSHOTS[0][1:] and [int(v) for v in kw['snap_hop']] == rc.SNAPSHOTS[1][1:]
    if 'set_capon_peaks' in by:
        cells, k, floor = by['set_capon_peaks'][0]
        assert k == K and floor == 0.0 and np.asarray(cells).shape == (G, 2)
    if 'set_beam_grid' in by:
        np.testing.assert_array_equal(by['set_beam_grid'][0][0], rc.GRID)
        assert by['set_beam_grid'][0][1] is req.beam_grid_map
    if 'set_kept_elements' in by:
        assert by['set_kept_elements'][0] == (N - 1, True, False)
    if 'set_capon_clean' in by:
        assert by['set_capon_clean'][0] == (I, 0.5, 0.02, True)
    if 'set_capon_music' in by:
        assert by['set_capon_music'][0] == (2, 0.05, True, True, True, 0.0)


def test_everything_on_is_set_in_order_and_unset_behind_the_plan():
    req, h = _all_on(), StubHandle()
    _launch(req, h)
    sets, unsets = _around_plan(h)
    assert [n for n, _, _ in sets] == [n for n in SET_ORDER if n != 'set_lag_limits']
    _check_band_1_tables(sets, req)
    _check_unsets(sets, unsets)
    assert h.names()[-2:] == ['stream_results', 'execute']
    plan = next(a for n, a, kw in h.log if n == 'plan')
    assert [int(w) for w in plan[4]] == [rc.WINDOWS[1]] and plan[0].shape[0] == 1          # the plan is band 1's too


@pytest.mark.parametrize('name', sorted(ALONE))
def test_each_request_alone(name):
    attrs, setters = ALONE[name]
    whole = _all_on() if name != 'lag_limits' else Requests.check(N, 2, rc.FS, list(rc.WINDOWS), rij=rc.recording()[1], min_velocity=0.3)
    req = Requests(**{a: getattr(whole, a) for a in attrs})
    for refuse in (None, 'plan'):
        h = StubHandle(refuse=refuse)
        if refuse:
            with pytest.raises(Refused):
                _launch(req, h)
        else:
            _launch(req, h)
        sets, unsets = _around_plan(h)
        assert [n for n, _, _ in sets] == list(setters)
        _check_band_1_tables(sets, req)
        _check_unsets(sets, unsets)
        assert ('execute' in h.names()) == (refuse is None)


def test_a_refused_plan_leaves_nothing_on_the_handle():
    h = StubHandle(refuse='plan')
    with pytest.raises(Refused):
        _launch(_all_on(), h)
    sets, unsets = _around_plan(h)
    assert len(sets) == len(SET_ORDER) - 1
    _check_unsets(sets, unsets)
    assert h.names()[-1] == 'set_beam_trace' and 'stream_results' not in h.names() and 'execute' not in h.names()
    # ... and with a window slice (which the beam trace and the families do not take: the other requests), the ranges go last
    req = _all_on().replace(beam_trace=None, families=None)
    for refuse in ('plan', 'set_capon_music', None):
        h = StubHandle(refuse=refuse)
        if refuse:
            with pytest.raises(Refused):
                _launch(req, h, window_slice=(1, 2))
        else:
            _launch(req, h, window_slice=(1, 2))
        names = h.names()
        assert names[0] == 'set_window_ranges' and names.count('set_window_ranges') == 2
        last = len(names) - 1 - names[::-1].index('set_window_ranges')
        assert h.log[last][1] == (None,) and names[last + 1:] == ([] if refuse else ['stream_results', 'execute'])
        assert all(n.startswith('set_') for n in names[names.index('set_uncertainty'):last] if n != 'plan')
    h = StubHandle(refuse='set_window_ranges')                # nothing was set: nothing is unset
    with pytest.raises(Refused):
        _launch(req, h, window_slice=(1, 2))
    assert h.names() == ['set_window_ranges']


@pytest.mark.parametrize('setter', SET_ORDER)
def test_a_refused_setter_unsets_what_was_set_before_it_and_nothing_else(setter):
    req = _all_on()
    if setter == 'set_lag_limits':             # (a seed does not combine with it: the everything-on record without the seed)
        req = req.replace(lag_seed=None, lag_limits=np.arange(P, dtype=np.int32) + 1)
    h = StubHandle(refuse=setter)
    with pytest.raises(Refused):
        _launch(req, h)
    names = h.names()
    assert names[:2] == ['reserve_results', 'set_uncertainty'] and 'plan' not in names and 'execute' not in names
    calls = h.log[2:]
    at = [n for n, _, _ in calls].index(setter)
    order = [n for n in SET_ORDER if n != ('set_lag_seed' if setter == 'set_lag_limits' else 'set_lag_limits')]
    assert [n for n, _, _ in calls[:at + 1]] == order[:order.index(setter) + 1]
    _check_unsets(calls[:at + 1], calls[at + 1:], refused=setter)


def test_launch_builds_the_same_record_from_its_keywords():
    """The explicit keywords of ``launch`` and a record of them make the same calls."""
    req = _all_on()
    a, b = StubHandle(), StubHandle()
    _launch(req, a)
    kw = {k: getattr(req, k) for k in Requests.DEFAULTS if not k.startswith('want_')}
    engine.launch(b, None, _prep(), bands=[1], upload=False, **kw)
    assert a.names() == b.names()
    for (n, x, xk), (_, y, yk) in zip(a.log, b.log):
        if n.startswith('set_') and n not in ('set_uncertainty', 'set_families'):
            assert repr((x, xk)) == repr((y, yk)), n


# ---- 2. every field arrives ----------------------------------------------------------------------------------------------
def _results(req, k=1, nchans=N):
    kw = req.result_keywords(rc.NPTS)
    return [engine.new_result(nchans, rc.ALPHA, rc.FS, np.array(rc.WINDOWS), np.array([32, 16]), np.array([VL, VL - 1]), VL, **kw)
            for _ in range(k)]


def _arrived(results, names, k):
    """Band 1 of recording j holds row 0 * k + j of the pass (constant + 100 j), band 0 nothing."""
    for j, res in enumerate(results):
        for name in names:
            a = getattr(res, name)
            assert a is not None, name
            assert not a[0].any(), (name, j)
            assert a[1].size and np.all(a[1] == np.asarray(CONST[name] + 100 * j).astype(a.dtype)), (name, j, a[1].ravel()[:3])


@pytest.mark.parametrize('k', [1, 2])
def test_every_field_arrives_in_its_rows(k):
    req = _all_on(**rc.LAGS)
    results = _results(req, k)
    assert all(getattr(results[0], name) is not None for name in BROUGHT)
    h = StubHandle(rows=k)
    h.families_of = k
    engine.fetch_groups(h, req, results, 1, 2)
    _arrived(results, BROUGHT, k)
    for j, res in enumerate(results):                       # the families: recording j's own, numbered from 0
        assert res.family.shape == (1, VL) and res.family.dtype == np.int32
        assert not res.family.any() and len(res.family_table) == 1 and res.family_table[0, 5] == 0
    # each group once per pass, the beam trace once per result row, the peaks once per spectrum
    names = h.names()
    for method in RETURNS:
        assert names.count(method) == (2 if method == 'fetch_capon_peaks' else 1), method
    assert [c for c in h.log if c[0] == 'fetch_capon_peaks'] == [('fetch_capon_peaks', (0,), {}), ('fetch_capon_peaks', (1,), {})]
    assert sorted(a[0] for n, a, kw in h.log if n == 'fetch_beam_trace') == list(range(k))
    assert names.count('fetch') == 1 and names.count('fetch_families') == 1
    assert set(names) == set(RETURNS) | {'fetch', 'fetch_beam_trace', 'fetch_families'}
    assert all(not kw for n, a, kw in h.log if n != 'fetch')
    assert next(kw for n, a, kw in h.log if n == 'fetch') == dict(grids=False, want_lag=True, want_cmax=True, want_z=True)


def test_an_estimator_index_reaches_the_groups_that_take_one():
    req = _all_on(**rc.LAGS)
    res = _results(req, nchans=N)[0]
    h = StubHandle()
    engine.fetch_groups(h, req, [res], 1, 2, est=1)
    assert h.names() == ['fetch'] + list(PER_ESTIMATOR)          # nothing of the plan's own estimator is fetched for another
    assert h.log[0][2] == dict(grids=False, want_lag=True, want_cmax=True, want_z=True, est=1)
    assert all(a == (1,) and not kw for n, a, kw in h.log[1:])
    mine = [f[0] for m in PER_ESTIMATOR for f in RETURNS[m]] + ['lag', 'cmax', 'z']
    _arrived([res], mine, 1)
    assert all(not getattr(res, name).any() for name in BROUGHT if name not in mine)


def test_the_fields_of_engine_are_those_of_the_handle():
    assert engine.CLEAN_FIELDS == tuple(f[0] for f in RETURNS['fetch_capon_clean'])
    assert engine.MUSIC_FIELDS == tuple(f[0] for f in RETURNS['fetch_capon_music'])
    assert engine.PEAK_FIELDS == tuple(f[0] for f in _PEAK)
    res = _results(_all_on(**rc.LAGS))[0]
    for fields in [r for r in RETURNS.values() if r] + [tuple((w + f, t, d) for f, t, d in _PEAK) for w in ('capon', 'bartlett')]:
        for name, trailing, dtype in fields:
            a = getattr(res, name)
            assert a.shape == (2, VL) + trailing and a.dtype == dtype, name
    assert res.beam_trace.shape == (2, rc.NPTS) and res.lag.shape == (2, VL, P) and res.lag.dtype == np.int32


# ---- 3. the calls of a pass --------------------------------------------------------------------------------------------------
# what ``launch`` + ``collect`` of a pass without any request made of the handle before the record existed (the parent of the
# commit that added it, run against this stand-in): an uploaded trace, not streamed
PLAIN_CALLS = [('set_trace_rows', 2), ('set_geometry', 3), ('reserve_results', 1), ('set_uncertainty', 1), ('plan', 7),
               ('stream_results', 1), ('execute', 0), ('fetch_packed', 0)]


def plain_calls(eng, *collect_more):
    """The (name, number of positional arguments) of every call ``eng.launch`` + ``eng.collect`` make for a plain pass."""
    data, rij = rc.recording()
    prep = eng.prepare(N, rc.NPTS, rc.FS, rij, rc.EDGES, rc.WINLENS, rc.OVERLAP, rc.ALPHA, *rc.FILTER)
    h = StubHandle(rows=2)
    eng.launch(h, list(data), prep)
    res = eng.new_result(N, rc.ALPHA, rc.FS, prep.W, prep.inc, prep.nwin, VL)
    eng.collect(res, h, 0, 2, False, eng._Notifier(res, None, None), *collect_more)
    return h, [(n, len(a)) for n, a, kw in h.log]


def test_a_plain_pass_makes_the_calls_it_always_made():
    h, calls = plain_calls(engine, Requests())
    assert calls == PLAIN_CALLS
    by = {n: (a, kw) for n, a, kw in h.log}
    assert by['set_uncertainty'] == ((None,), {}) and by['reserve_results'] == ((0,), {}) and by['stream_results'] == ((False,), {})
    assert by['execute'] == ((), dict(after=None)) and by['plan'][1] == dict(lts=by['plan'][1]['lts'], xcorr_impl=0)


# ---- 4. the refusals of the time-segmented path ------------------------------------------------------------------------------
_HEAD = ': a trace of 5 x 601 samples takes the time-segmented path (not even one filtered band fits the HBM budget of a pass, ' \
        'NBLS_MAX_FILTERED_GB)'
_HOST = ', which keeps the filtered band on the host: '
_SLICE = ', which correlates the band slice by slice: '
# in the order of precedence: ``process`` refuses the first two before the upload, ``process_segmented`` the others
REFUSALS = (
    ('kept', dict(kept=(None, False, False)), 'kept' + _HEAD + ': the kept elements are not available there'),
    ('capon_grid', {k: v for k, v in rc.ALL_ON.items() if k in ('capon_grid', 'capon_freqs', 'capon_snapshots')},
     'capon_grid' + _HEAD + _HOST + 'the Capon spectra are not available there'),
    ('element_max_shift', dict(element_max_shift=3), 'element_max_shift' + _HEAD + _HOST + 'the element delays are not available there'),
    ('beam_taps', dict(beam_taps=4, want_beam=True), 'beam_taps' + _HEAD + _HOST + 'fractional-sample steering is not available there'),
    ('want_beam_trace', dict(want_beam_trace=True), 'want_beam_trace' + _HEAD + _HOST + 'the beam trace is not available there'),
    ('want_consistency', dict(want_consistency=True), 'want_consistency' + _HEAD + _SLICE + 'closure results are not available there'),
    ('seed_halfwidths', dict(seed_halfwidths=3, slowness_grid=rc.GRID), 'seed_halfwidths' + _HEAD + _HOST + 'the seeded lag search is not available there'),
    ('slowness_grid', dict(slowness_grid=rc.GRID), 'slowness_grid' + _HEAD + _HOST + 'the slowness-grid search is not available there'),
    ('min_velocity', dict(min_velocity=0.3), 'min_velocity' + _HEAD + _SLICE + 'the bounded lag search is not available there'),
    ('want_subsample', dict(want_subsample=True), 'want_subsample' + _HEAD + _HOST + 'sub-sample lag refinement is not available there'),
    ('want_beam', dict(want_beam=True), 'want_beam' + _HEAD + _HOST + 'beam results are not available there'),
)


def _segmented(monkeypatch, **kw):
    """``process`` of a trace of which not one band fits; any use of the GPU fails the test."""
    def no_gpu(*a, **k):
        raise AssertionError('the refusal comes before any GPU work')
    monkeypatch.setattr(engine, 'get_handle', no_gpu)
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', repr(0.5 * 8.0 * N * (rc.NPTS + 64) / 2.0 ** 30))
    data, rij = rc.recording()
    assert engine.max_bands_per_pass(N, rc.NPTS, 1) == 0
    return engine.process(data, rc.FS, rc.T0, rij, rc.EDGES, rc.WINLENS, rc.OVERLAP, rc.ALPHA, *rc.FILTER, **kw)


@pytest.mark.parametrize('case', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_the_segmented_path_refuses_each_request_with_its_text(monkeypatch, case):
    keyword, kw, text = case
    with pytest.raises(ValueError) as e:
        _segmented(monkeypatch, **kw)
    assert str(e.value) == text
    if keyword not in ('kept', 'capon_grid', 'beam_taps', 'seed_halfwidths'):       # (alone: ``process_segmented`` takes these itself)
        data, rij = rc.recording()
        with pytest.raises(ValueError) as e:
            engine.process_segmented(data, rc.FS, rc.T0, rij, rc.EDGES, rc.WINLENS, rc.OVERLAP, rc.ALPHA, *rc.FILTER, None, **kw)
        assert str(e.value) == text


def test_the_earlier_refusal_wins(monkeypatch):
    for i in range(len(REFUSALS) - 1):
        (first, kw1, text), (second, kw2, _) = REFUSALS[i], REFUSALS[i + 1]
        with pytest.raises(ValueError) as e:
            _segmented(monkeypatch, **dict(kw2, **kw1))
        assert str(e.value) == text, (first, second)
    with pytest.raises(ValueError) as e:                                          # ... the first against the last
        _segmented(monkeypatch, want_beam=True, kept=(None, True, False))
    assert str(e.value) == REFUSALS[0][2]
