"""The results of the elements FAST-LTS kept (``nbls_set_kept_elements``, csrc/kept.hip and the KEPT instances of
csrc/beam.hip and csrc/capon.hip) on the GPU:

* ``dropped_mask`` / ``kept_count`` exactly the rule of tests/kept_truth.py applied to the weights the same pass returns, on
  lag tables designed with unit pulses whose intended set the oracle's LTS names on the CPU;
* where nothing is dropped (an OLS plan, LTS on a clean wave) every beam, Capon, map, CSDM and peak field equal to the plan
  without the feature, bit for bit;
* the kept beam against ``beam_truth`` on the GPU's own z and the kept spectra against ``capon_truth`` on the GPU's own R, both
  through ``kept_truth`` with those modules' bounds unchanged; the peaks bit-equal to ``peaks_truth`` on the fetched maps;
* the forms of a pass (single, streamed, a batch of recordings, window slices, seeded and bounded picks) bit for bit;
* what the library refuses."""
import os
import subprocess
import sys

import numpy as np
import pytest

import beam_truth
import capon_truth as ct
import kept_truth as kt
import peaks_truth as pt
import solve_truth as st
from narrow_band_least_squares_amd import (engine, planner, synthetic, _hip, ltsva_beam, ltsva_kept, ltsva_kept_batch,
                                           narrow_band_least_squares_kept)

pytestmark = pytest.mark.gpu

FS = 20.0
T0 = 17884.0729166667
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = planner.slowness_grid(3.07, 5)                       # 13 points of a 5 x 5 lattice
CELLS = planner.grid_cells(GRID)[0]
FREQ = 1.3
KEPT = ('dropped_mask', 'kept_count')
BEAM = ('beam_power', 'fstat')
CAPON = ('capon_index', 'capon_power', 'bartlett_index', 'bartlett_power', 'capon_map', 'bartlett_map', 'capon_csdm')
PEAKS = tuple(w + f for w in ('capon', 'bartlett') for f in engine.PEAK_FIELDS)
PLAIN = ('vel', 'baz', 'mdccm', 'sigma_tau', 'mask')


def _same(a, b, keys, label=''):
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        assert x is not None and y is not None, (label, k)
        assert pt.same_bits(x, y), (label, k)


class _options:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            engine.get_handle().set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            engine.get_handle().set_option(k, 0)


def _mistimed(N, npts, bad, seed=900, second=None, snr_db=10.0):
    """A 0.5 - 4 Hz plane wave over N elements with element ``bad`` 0.25 s late (5 samples) and, on request, element
    ``second`` 0.35 s early -> (data, centred rij)."""
    rij = synthetic.array_geometry(N, 1.0)
    data = synthetic.plane_wave(rij, npts, FS, 0.5, 4.0, baz_deg=60.0, snr_db=snr_db, seed=seed,
                                timing_error_s=0.25 if bad is not None else 0.0, bad_element=bad)
    if second is not None:
        data[second] = np.roll(data[second], -7)
    return np.ascontiguousarray(data), rij - rij.mean(axis=1, keepdims=True)


def _process(data, rij, W, alpha, kept, capon=False, peaks=0, overlap=0.5, Ls=16, Hs=8, grid=GRID, **kw):
    if capon:
        kw = dict(dict(capon_grid=grid, capon_freqs=[FREQ], capon_snapshots=(Ls, Hs), capon_loading=0.01, want_capon_maps=True,
                       want_capon_csdm=True, capon_peaks=peaks, capon_peak_floor=0.0), **kw)
    res = engine.process(data, FS, T0, rij, [(None, None)], [(W + 0.5) / FS], overlap, alpha, prefiltered=True, kept=kept, **kw)
    assert int(res.W[0]) == W
    return res


def _check_rule(res, N, q, band=0):
    """The mask and the count against the rule on the pass's own weights; zeros beyond the band's windows."""
    n = int(res.nwin[band])
    mask, count = kt.rule_table(np.asarray(res.weights)[band, :n], N, q)
    np.testing.assert_array_equal(res.dropped_mask[band, :n], mask)
    np.testing.assert_array_equal(res.kept_count[band, :n], count)
    assert res.dropped_mask.dtype == np.uint32 and res.kept_count.dtype == np.int32
    assert not res.dropped_mask[band, n:].any() and not res.kept_count[band, n:].any()
    return mask, count


# ---- designed weights ----

def _designed(N):
    """Windows of unit pulses on a plane-wave pattern with one or two elements' pulses displaced -> (tabs, intended sets)."""
    q = st.grid_units(N)
    s = st.SLOWNESS[0]
    p = st.CENTRE - (q[:, 0] * s[0] + q[:, 1] * s[1])
    rows = [('exact', p.copy(), ())]
    for e in (0, N // 2, N - 1):
        pk = p.copy()
        pk[e] += 7
        rows.append(('element %d' % e, pk, (e,)))
    pk = p.copy()
    pk[N - 1] += 7
    pk[0] -= 5
    rows.append(('elements 0 and %d' % (N - 1), pk, (0, N - 1)))
    if N == 16:                                                      # (the oracle's FAST-LTS takes seconds per window from here on)
        rows = [rows[2], rows[4]]
    if N == 32:
        rows = [rows[3]]
    # one mistimed element is within the breakdown point of ALPHA = 0.5 from 5 elements on, two from 8 on: below, LTS
    # cannot name them (solve_truth's module docstring)
    want = [tuple(e for e in bad if st.within_breakdown(N, len(bad))) for _, _, bad in rows]
    tabs = [(name, [[(int(v), 1.0)] for v in pk]) for name, pk, _ in rows]
    return tabs, want


@pytest.mark.parametrize('N', [4, 5, 8, 9, 16, 32])
def test_designed_weights(oracle, N):
    """Both FAST-LTS kernel families (registers up to 8 elements, buckets beyond), element 0, a middle one, the last, two at
    once; q = N - 1, N - 2 and 1, where every element that lost a pair is named and the kept set falls back to the array."""
    tabs, want = _designed(N)
    rij = st.grid_geometry(N)
    xij = planner.co_array(rij)[0]
    lag, _ = st.designed_lags(tabs)
    ref = st.oracle_lts(oracle, lag, xij, 0.5)
    intended = [sum(1 << e for e in w) for w in want]
    for w in range(len(tabs)):                                       # on the CPU: no case is vacuous
        assert kt.rule(ref['weights'][:, w], N, N - 1)[0] == intended[w], tabs[w][0]
    assert any(intended) or N == 4                                   # N = 4: LTS cannot name anyone
    x = st.pulse_trace(tabs)
    n = len(tabs)
    for q in sorted({N - 1, max(1, N - 2), 1}):
        res = engine.process(x, st.FS, T0, rij, [(None, None)], [st.W / st.FS], 0.0, 0.5, prefiltered=True, vector_len=n + 3,
                             kept=(q, False, False))
        assert int(res.nwin[0]) == n
        mask, count = _check_rule(res, N, q)
        if q == N - 1:
            assert mask.tolist() == intended
            assert count.tolist() == [N - len(w) if N - len(w) >= 3 else N for w in want]
        if q == 1 and N >= 5:
            # every pair of a mistimed element is at weight 0: each other element has lost one, all are named, M = N
            for w in range(n):
                if intended[w]:
                    assert mask[w] == (1 << N) - 1 and count[w] == N, tabs[w][0]
        assert res.beam_power is None and res.capon_index is None


# ---- nothing dropped: the plain plan's bits ----

@pytest.mark.parametrize('alpha', [1.0, 0.5])
def test_nothing_dropped_gives_the_plain_plans_bits(alpha):
    """An OLS plan (every weight 1), and an LTS plan on a clean wave (no element loses all of its pairs), on every route."""
    N = 8
    data, rij = _mistimed(N, 257 * 3, None)
    kw = dict(capon=True, peaks=3, want_beam=True)
    plain = _process(data, rij, 257, alpha, None, Ls=64, Hs=16, **kw)
    assert plain.dropped_mask is None
    for route in (0, 1, 2):
        with _options(capon_peak_route=route):
            on = _process(data, rij, 257, alpha, (N - 1, True, True), Ls=64, Hs=16, **kw)
            ref = plain if route == 0 else _process(data, rij, 257, alpha, None, Ls=64, Hs=16, **kw)
        n = int(on.nwin[0])
        assert n >= 4 and not on.dropped_mask.any() and np.all(on.kept_count[0, :n] == N)
        _same(on, ref, PLAIN + BEAM + CAPON + PEAKS, 'alpha %g route %d' % (alpha, route))


# ---- the kept beam ----

def _beam_against_truth(res, filt, N, band=0, label=''):
    n, W, inc = int(res.nwin[band]), int(res.W[band]), int(res.inc[band])
    refs = [kt.beam_reference(filt, FS, res.xij, res.z[band], W, inc, w, kt.kept_of_mask(res.dropped_mask[band, w], N))
            for w in range(n)]
    ref = {k: np.concatenate([r[k] for r in refs]) for k in refs[0]}
    on_f, skipped = beam_truth.compare(res.beam_power[band, :n], res.fstat[band, :n], ref)
    print('%s: %d windows, %d with a dropped element, %d compared on F, %d skipped at a delay tie'
          % (label, n, int(np.count_nonzero(res.dropped_mask[band, :n])), on_f, skipped))
    assert not res.beam_power[band, n:].any() and not res.fstat[band, n:].any()
    return on_f


@pytest.mark.parametrize('N,bad,second,W', [(8, 0, None, 257), (8, 4, None, 257), (8, 7, None, 129), (9, 0, 8, 257),
                                              (5, 4, None, 129), (6, 0, None, 513)])
def test_kept_beam_against_the_truth(N, bad, second, W):
    """Element 0 dropped moves the reference element; two elements at once; 9 elements (the bucket solver); 513 samples
    (all four waves of a workgroup sum one unit)."""
    data, rij = _mistimed(N, W * 6 + 1, bad, second=second)
    res = _process(data, rij, W, 0.5, (N - 1, True, False), want_beam=True, want_z=True)
    n = int(res.nwin[0])
    mask, _ = _check_rule(res, N, N - 1)
    named = sum(1 << e for e in (bad, second) if e is not None)
    assert np.count_nonzero(mask == named) >= n // 2, mask           # the input does what it was made for
    on_f = _beam_against_truth(res, data, N, label='N=%d bad=%s W=%d' % (N, (bad, second), W))
    assert on_f >= n // 2
    full = _process(data, rij, W, 0.5, None, want_beam=True)
    _same(res, full, PLAIN)
    hit = mask != 0
    assert np.all(res.fstat[0, :n][hit] != full.fstat[0, :n][hit])
    assert pt.same_bits(res.fstat[0, :n][~hit], full.fstat[0, :n][~hit])
    assert np.median(res.fstat[0, :n][hit]) > np.median(full.fstat[0, :n][hit])


# ---- the kept spectra ----

def _spectra_against_truth(res, N, delta=0.01, band=0, label='', grid=GRID, cells=CELLS, K=0, windows=None):
    n = int(res.nwin[band])
    _, steer = res.handle.fetch_capon_tables(band)
    worst = dict(B=0.0, C=0.0)
    for w in (range(n) if windows is None else windows):
        kept = kt.kept_of_mask(res.dropped_mask[band, w], N)
        assert len(kept) == res.kept_count[band, w]
        ref = kt.spectra_reference(res.capon_csdm[band, w], steer, delta, kept)
        assert ref['chol_ok'] and ref['kappa'] * len(kept) * ct.U < 1e-6, 'a condition on the inputs (%s, window %d)' % (label, w)
        worst['B'] = max(worst['B'], ct.check_spectrum('%s Bartlett w=%d' % (label, w), ref['PB'], ref['tolB'], ref['index_B'],
                                                       int(res.bartlett_index[band, w]), float(res.bartlett_power[band, w]),
                                                       res.bartlett_map[band, w]))
        worst['C'] = max(worst['C'], ct.check_spectrum('%s Capon w=%d' % (label, w), ref['PC'], ref['tolC'], ref['index_C'],
                                                       int(res.capon_index[band, w]), float(res.capon_power[band, w]),
                                                       res.capon_map[band, w]))
    print('%s: worst |d| / bound, Bartlett %.3g, Capon %.3g' % (label, worst['B'], worst['C']))
    if K:
        for name in ('capon', 'bartlett'):
            want = pt.peaks_of_maps(getattr(res, name + '_map')[band, :n], cells, K, 0.0)
            for field, exp in zip(engine.PEAK_FIELDS, want):
                assert pt.same_bits(getattr(res, name + field)[band, :n], exp), (label, name + field)
    return worst


@pytest.mark.parametrize('route', [1, 2])
@pytest.mark.parametrize('N,bad,second', [(8, 0, None), (8, 7, 3), (5, 2, None)])
def test_kept_spectra_against_the_truth(N, bad, second, route):
    W = 257
    data, rij = _mistimed(N, W * 4 + 1, bad, second=second)
    with _options(capon_peak_route=route):
        res = _process(data, rij, W, 0.5, (N - 1, False, True), capon=True, peaks=3, Ls=64, Hs=16)
        # (the plan's own tables are fetched while the plan stands: an option or another pass replaces it)
        _spectra_against_truth(res, N, label='N=%d bad=%s route %d' % (N, (bad, second), route), K=3)
        nomaps = _process(data, rij, W, 0.5, (N - 1, False, True), capon=True, peaks=3, Ls=64, Hs=16, want_capon_maps=False)
        full = _process(data, rij, W, 0.5, None, capon=True, peaks=3, Ls=64, Hs=16)
    n = int(res.nwin[0])
    mask, _ = _check_rule(res, N, N - 1)
    named = sum(1 << e for e in (bad, second) if e is not None)
    assert np.count_nonzero(mask == named) >= n // 2, mask
    _same(nomaps, res, KEPT + CAPON[:4] + PEAKS + PLAIN + ('capon_csdm',), 'without the maps')
    # R is the full array's, as without the feature; the spectra differ exactly where an element is dropped
    _same(res, full, PLAIN + ('capon_csdm',))
    hit = mask != 0
    assert np.all(res.capon_power[0, :n][hit] != full.capon_power[0, :n][hit])
    for k in CAPON[:6] + PEAKS:
        assert pt.same_bits(getattr(res, k)[0, :n][~hit], getattr(full, k)[0, :n][~hit]), k


def test_32_elements_and_a_grid_the_lds_route_refuses():
    """96 KiB of the kernel's own LDS and 128 KiB of maps: option capon_peak_route 1 is refused, the automatic choice takes
    the HBM route, and the KEPT instance runs with 31 of 32 elements."""
    N, W = 32, 129
    g0, g1 = np.meshgrid((np.arange(128) - 64) * 0.05, (np.arange(64) - 32) * 0.05, indexing='ij')
    grid = np.ascontiguousarray(np.stack([g0.ravel(), g1.ravel()], axis=1))
    cells = planner.grid_cells(grid)[0]
    data, rij = _mistimed(N, W * 2 + 1, N - 1)
    with _options(capon_peak_route=1):
        with pytest.raises(ValueError, match='capon_peak_route 1') as err:
            _process(data, rij, W, 0.5, (N - 1, False, True), capon=True, peaks=2, grid=grid, Ls=32, Hs=8)
        assert err.value.code == _hip.NBLS_ERR_UNSUPPORTED
    res = _process(data, rij, W, 0.5, (N - 1, False, True), capon=True, peaks=2, grid=grid, Ls=32, Hs=8)
    n = int(res.nwin[0])
    mask, count = _check_rule(res, N, N - 1)
    assert n >= 2 and np.any(mask == 1 << (N - 1)), mask
    w = int(np.flatnonzero(mask == 1 << (N - 1))[0])
    assert count[w] == N - 1
    _spectra_against_truth(res, N, label='N=32', grid=grid, cells=cells, K=2, windows=[w])


# ---- the forms of a pass ----

EDGES = [(0.5, 1.5), (1.5, 4.0)]
WINLENS = [257.5 / FS, 65.5 / FS]
FILTER = ('butter', 2, 0.01)
NF = 6
FORM_KW = dict(want_beam=True, capon_grid=GRID, capon_freqs=planner.capon_frequencies(EDGES), capon_snapshots=([64, 16], [16, 8]),
               capon_loading=0.01, want_capon_maps=True, want_capon_csdm=True, capon_peaks=3, capon_peak_floor=0.0,
               kept=(NF - 1, True, True))
FORM_FIELDS = PLAIN + KEPT + BEAM + CAPON + PEAKS


def _recordings(npts=2401, S=3):
    rij = synthetic.array_geometry(NF, 1.0)
    data = [np.ascontiguousarray(synthetic.plane_wave(rij, npts, FS, 0.5, 4.0, baz_deg=20.0 + 67.0 * i, snr_db=10.0, timing_error_s=0.25,
                                                      bad_element=(NF - 1, 0, 2)[i], seed=520 + i)) for i in range(S)]
    return data, rij - rij.mean(axis=1, keepdims=True), [T0 + 0.0173 * i for i in range(S)]


def _two_bands(data, rij, t0=T0, **kw):
    return engine.process(data, FS, t0, rij, EDGES, WINLENS, 0.5, 0.5, *FILTER, **dict(FORM_KW, **kw))


def _drops_something(res):
    for b in range(2):
        n = int(res.nwin[b])
        m = res.dropped_mask[b, :n]
        assert np.any(m != 0) and np.any(res.kept_count[b, :n] < NF), ('band', b, m)
        _check_rule(res, NF, NF - 1, band=b)


def test_batch_of_three_recordings_equals_three_single_calls():
    """Two bands of different W, three recordings with a different element mistimed in each: result row b * 3 + s."""
    recs, rij, t0s = _recordings()
    batch = engine.process_batch([list(d) for d in recs], FS, t0s, rij, EDGES, WINLENS, 0.5, 0.5, *FILTER, **FORM_KW)
    assert len(batch) == 3
    for s in range(3):
        single = _two_bands(recs[s], rij, t0s[s])
        assert [int(w) for w in single.W] == [257, 65] and single.nwin[0] < single.nwin[1]
        _drops_something(single)
        _same(batch[s], single, FORM_FIELDS, 'recording %d' % s)
    assert not np.array_equal(batch[0].dropped_mask, batch[1].dropped_mask)


def test_streamed_in_several_batches_equals_the_unstreamed_pass(monkeypatch):
    recs, rij, _ = _recordings(48001, 1)
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    whole = _two_bands(recs[0], rij)
    _drops_something(whole)
    h = engine.get_handle()
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '1')
    try:
        h.set_option('screen_batch_mb', 1)
        h.set_option('solve_min_units', 1)
        streamed = _two_bands(recs[0], rij)
        nbatches = h.result_batches()
    finally:
        h.set_option('screen_batch_mb', 192)
        h.set_option('solve_min_units', 0)
    assert nbatches >= 3, nbatches                                   # more batches than window groups: one cuts a band's rows
    _same(streamed, whole, FORM_FIELDS, 'streamed')


def test_window_slices_add_up_to_the_full_call():
    recs, rij, _ = _recordings(2401, 1)
    full = _two_bands(recs[0], rij)
    parts = [_two_bands(recs[0], rij, window_slice=(k, 3)) for k in range(3)]
    for k in KEPT + BEAM + CAPON + PEAKS:
        total = np.zeros_like(getattr(full, k))
        for p in parts:
            a = getattr(p, k)
            assert not np.any((a != 0) & (total != 0)), k           # rows outside a slice stay zero
            total = total + a
        np.testing.assert_array_equal(total, getattr(full, k), err_msg=k)


@pytest.mark.parametrize('picks', ['seeded', 'bounded'])
def test_seeded_and_bounded_picks(picks):
    """The feature reads the weights of whatever picks the plan makes; the beam and the spectra follow the mask it finds."""
    N, W = 8, 257
    data, rij = _mistimed(N, W * 4 + 1, 7)
    kw = dict(slowness_grid=planner.slowness_grid(3.5, 11), seed_halfwidths=6) if picks == 'seeded' else dict(min_velocity=0.3)
    res = _process(data, rij, W, 0.5, (N - 1, True, True), capon=True, peaks=2, Ls=64, Hs=16, want_beam=True, want_z=True, **kw)
    n = int(res.nwin[0])
    mask, _ = _check_rule(res, N, N - 1)
    assert np.count_nonzero(mask == 1 << 7) >= n // 2, mask
    assert _beam_against_truth(res, data, N, label=picks) >= n // 2
    _spectra_against_truth(res, N, label=picks, K=2)


# ---- refusals ----

def test_refusals_of_the_library():
    N = 5
    data, rij = _mistimed(N, 1201, 4)
    res = engine.process(data, FS, T0, rij, [(None, None)], [65.5 / FS], 0.5, 1.0, prefiltered=True)
    h = res.handle
    plan = lambda: h.plan(None, False, None, None, [65], [32], 40)
    with pytest.raises(_hip.NblsError) as err:                       # the plan did not ask
        h.fetch_kept_elements()
    assert err.value.code == _hip.NBLS_ERR_STATE
    for bad in ((-1, 0), (1, 4), (1, -1), (2, 8)):                   # a negative min_pairs, unknown flags: the handle is unchanged
        rc = h.lib.nbls_set_kept_elements(h._h, *bad)
        assert rc == _hip.NBLS_ERR_ARG, bad
    plan()
    with pytest.raises(_hip.NblsError):
        h.fetch_kept_elements()
    try:
        h.set_kept_elements(N)                                       # min_pairs > N - 1
        with pytest.raises(ValueError, match='min_pairs') as err:
            plan()
        assert err.value.code == _hip.NBLS_ERR_ARG
        h.set_kept_elements(N - 1, beam=True)                        # a flag without its feature
        with pytest.raises(_hip.NblsError, match='nbls_set_beam') as err:
            plan()
        assert err.value.code == _hip.NBLS_ERR_STATE
        h.set_kept_elements(N - 1, capon=True)
        with pytest.raises(_hip.NblsError, match='nbls_set_capon') as err:
            plan()
        assert err.value.code == _hip.NBLS_ERR_STATE
        h.set_kept_elements(N - 1)
        plan()                                                       # the mask alone: accepted
        assert not any(a.any() for a in h.fetch_kept_elements())     # zeros until a pass has run the solve stage
        h.execute(stages=3)
        assert not any(a.any() for a in h.fetch_kept_elements())
        h.execute()
        mask, count = h.fetch_kept_elements()
        assert not mask.any() and np.all(count[0, :int(res.nwin[0])] == N)      # an OLS plan: every weight is 1
        sub = [0, 1, 2, 3]                                           # further estimators are out of scope
        xs, ps, xp = planner.co_array(rij[:, sub])
        h.set_estimators([dict(kept=sub, xij=xs, pair_idx=ps, xpinv=xp, lts=None, eig6=None)])
        with pytest.raises(ValueError, match='nbls_set_estimators') as err:
            plan()
        assert err.value.code == _hip.NBLS_ERR_UNSUPPORTED
    finally:
        h.set_estimators(())
        h.set_kept_elements(0)
    plan()
    with pytest.raises(_hip.NblsError):                              # switched off again
        h.fetch_kept_elements()
    fresh = _hip.Handle(0)
    try:
        xij, pair_idx, xpinv = planner.co_array(rij)
        perm = np.arange(len(xij))
        perm[[0, 1]] = [1, 0]                                        # every pair, not in lexicographic order
        fresh.set_trace(data, FS)
        fresh.set_geometry(xij[perm], np.asarray(pair_idx)[perm], xpinv[:, perm])
        fresh.plan(None, False, None, None, [65], [32], 40)
        fresh.set_kept_elements(N - 1)
        with pytest.raises(_hip.NblsError, match='lexicographic') as err:
            fresh.plan(None, False, None, None, [65], [32], 40)
        assert err.value.code == _hip.NBLS_ERR_STATE
    finally:
        fresh.close()


def test_rccl_communicator_refuses_the_request_at_plan_time():
    """A communicator lives as long as its process: a child process over the tests' loopback transport."""
    src = os.path.join(ROOT, 'tests', 'c_caller', 'loopback_rccl.cpp')
    lib = os.path.join(ROOT, 'tests', 'c_caller', 'libloopback_rccl.so')
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.run(['/opt/rocm/bin/hipcc', '-O2', '-shared', '-fPIC', '--offload-arch=gfx950', src, '-o', lib], check=True,
                       timeout=300)
    env = dict(os.environ, NBLS_TEST_TRANSPORT=lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_kept_comm_worker.py')], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and 'KEPT_COMM_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the public calls ----

def _demonstration():
    from test_kept_truth import _band, NPTS, BAD
    rij = synthetic.array_geometry(8, 1.0)
    data = _band(synthetic.plane_wave(rij, NPTS, FS, 0.1, 5.0, snr_db=10.0, timing_error_s=0.25, bad_element=BAD))
    return synthetic.make_stream(np.ascontiguousarray(data), FS), rij, BAD


def test_public_call_on_the_demonstration_trace():
    st8, rij, bad = _demonstration()
    got = ltsva_kept(st8, None, None, 120.0, 0.5, alpha=0.5, rij=rij)
    beam = ltsva_beam(st8, None, None, 120.0, 0.5, alpha=0.5, rij=rij)
    assert len(got) == 9 and sorted(got[8]) == ['beam_power', 'dropped_elements', 'fstat', 'kept_count']
    for i in (0, 1, 2, 3, 5, 6, 7):
        np.testing.assert_array_equal(got[i], beam[i])
    assert sorted(got[4]) == sorted(beam[4]) and all(np.array_equal(got[4][k], beam[4][k]) for k in beam[4])
    dropped = got[8]['dropped_elements']
    assert dropped.shape == (20, 8) and dropped.dtype == bool
    only = np.zeros(8, dtype=bool)
    only[bad] = True
    exactly = int(np.sum(np.all(dropped == only, axis=1)))
    ratio = np.median(got[8]['fstat']) / np.median(beam[9])
    print('ltsva_kept on the demonstration trace: element %d alone in %d / 20 windows, median F %.1f against %.1f of ltsva_beam '
          '(%.2f x)' % (bad, exactly, np.median(got[8]['fstat']), np.median(beam[9]), ratio))
    assert exactly >= 18
    assert np.median(got[8]['fstat']) >= 2.0 * np.median(beam[9])
    assert np.array_equal(got[8]['kept_count'], 8 - dropped.sum(axis=1))


def test_public_batch_and_narrow_band_calls():
    recs, rij, t0s = _recordings()
    sts = [synthetic.make_stream(d, FS, starttime=t) for d, t in zip(recs, t0s)]
    kw = dict(alpha=0.5, rij=rij, slowness_grid=GRID, freq=FREQ, snapshots=(16, 8), maps=True, peaks=2)
    batch = ltsva_kept_batch(sts, None, None, 65.5 / FS, 0.5, **kw)
    assert len(batch) == 3
    for got, s8 in zip(batch, sts):
        exp = ltsva_kept(s8, None, None, 65.5 / FS, 0.5, **kw)
        assert len(got) == len(exp) == 9 and sorted(got[8]) == sorted(exp[8])
        for i in (0, 1, 2, 3, 5, 6, 7):
            np.testing.assert_array_equal(got[i], exp[i], err_msg='return %d' % i)
        for k in exp[8]:
            assert pt.same_bits(got[8][k], exp[8][k]), k
        assert {'dropped_elements', 'kept_count', 'fstat', 'capon_index', 'capon_map', 'capon_peak_slowness'} <= set(got[8])
    fr = np.logspace(-1, 0.5, 16)
    out = narrow_band_least_squares_kept([257.5 / FS, 65.5 / FS], 0.5, 0.5, sts[0], None, None, 2, np.zeros(16), np.zeros(16),
                                         np.array([0.5, 1.5, 4.0]), 'linear', fr, 'butter', 2, 0.01, rij=rij, slowness_grid=GRID)
    assert len(out) == 10
    d = out[9]
    nwin = out[6]
    VL = out[0].shape[1]                                             # (rows as long as vel_array's)
    assert VL >= max(nwin) and d['dropped_elements'].shape == (2, VL, NF)
    assert d['kept_count'].shape == d['fstat'].shape == d['capon_power'].shape == (2, VL)
    for b in range(2):
        assert not d['dropped_elements'][b, nwin[b]:].any() and not d['kept_count'][b, nwin[b]:].any()
        assert np.all(d['kept_count'][b, :nwin[b]] == NF - d['dropped_elements'][b, :nwin[b]].sum(axis=1))
        assert d['dropped_elements'][b, :nwin[b]].any()             # (as ``_drops_something`` finds for the same bands)
