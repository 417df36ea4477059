"""The opt-in per-window results in passes of several bands AND several recordings (``engine.process_batch``): the case of
tests/band_batch_cases.py, B = 2 bands x S = 3 recordings, whose two bands differ in every per-band table (window length,
Capon frequency and snapshots, seed half-width).  The result row is r = b * S + s and the tables stay per band; with one
band every formula for the band of a row gives 0, so the single-band batch tests of the other files cannot tell them apart.

Every comparison between two GPU runs is bit for bit (``_same``: the bytes).  The one comparison with the truths is the
single two-band call, band by band with that band's tables, through the checkers of the single-band files with their
bounds unchanged; the equalities carry it to the batch rows.  tests/test_band_batch_cases.py shows on the CPU that a
mix-up of the bands' tables moves the results by far more than those bounds."""
import numpy as np
import pytest

import band_batch_cases as bb
import filter_truth as ft
import grid_truth as gt
from test_gpu_beam import _against_reference as beam_check
from test_gpu_capon import _against_reference as capon_check
from test_gpu_closure import _check_refined as closure_check
from test_gpu_grid import _against_reference as grid_check
from test_gpu_peaks import _against_truth as peaks_check, _options
from test_gpu_seeded import _check_res as seeded_check
from test_gpu_subsample import _check_fractions as fractions_check
from narrow_band_least_squares_amd import engine, planner

pytestmark = pytest.mark.gpu

ROW_BYTES = 8.0 * bb.N * (bb.NPTS + 64)          # one recording's filtered band in HBM (``engine.max_bands_per_pass``)


def _single(s, data=None, **kw):
    recs, rij, t0s = bb.recordings()
    return engine.process((recs if data is None else data)[s], bb.FS, t0s[s], rij, bb.EDGES, bb.WINLENS, bb.OVERLAP, bb.ALPHA,
                          *bb.FILTER, **kw)


def _batch(data=None, **kw):
    recs, rij, t0s = bb.recordings()
    out = engine.process_batch([list(d) for d in (recs if data is None else data)], bb.FS, t0s, rij, bb.EDGES, bb.WINLENS,
                               bb.OVERLAP, bb.ALPHA, *bb.FILTER, **kw)
    assert len(out) == bb.S
    return out


def _same(got, exp, fields=bb.FIELDS, label=''):
    """The bytes of every field; a field is None in both or in neither."""
    for k in fields:
        a, b = getattr(got, k), getattr(exp, k)
        assert (a is None) == (b is None), (label, k)
        if a is None:
            continue
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (label, k, a.shape, b.shape, a.dtype, b.dtype)
        if a.tobytes() != b.tobytes():
            np.testing.assert_array_equal(a, b, err_msg='%s %s' % (label, k))         # (says where)
            raise AssertionError('%s %s: equal values in different bits' % (label, k))


def _all_same(got, exp, fields=bb.FIELDS, label=''):
    assert len(got) == len(exp) == bb.S
    for s in range(bb.S):
        _same(got[s], exp[s], fields, '%s recording %d' % (label, s))


def _present(res):
    return [k for k in bb.FIELDS if getattr(res, k) is not None]


def _check_shape_of_a_batch(batch, wanted):
    """Both bands have their own window count and zeros behind it; the fields the options ask for are there; the recordings
    differ in every one of them."""
    for res in batch:
        assert [int(w) for w in res.W] == list(bb.WINDOWS)
        assert res.vel.shape == (bb.B, int(max(res.nwin))) and min(res.nwin) < max(res.nwin)         # the shorter row has padding cells
        for k in wanted:
            assert getattr(res, k) is not None, k
        for k in _present(res):
            for b in range(bb.B):
                n = int(res.nwin[b])
                assert not getattr(res, k)[b, n:].any(), (k, b)
                assert getattr(res, k)[b, :n].any(), (k, b)
    for k in [k for k in _present(batch[0]) if getattr(batch[0], k).dtype.kind in 'fc']:          # (an integer row may well repeat)
        for i in range(bb.S):
            for j in range(i + 1, bb.S):
                for b in range(bb.B):
                    assert not np.array_equal(getattr(batch[i], k)[b], getattr(batch[j], k)[b]), (k, i, j, b)


@pytest.fixture(scope='module')
def all_on():
    """The plain batch with everything on, computed once and left unchanged."""
    return _batch(**bb.ALL_ON)


WANTED = {'beam': ('beam_power', 'fstat'), 'subsample': (), 'min_velocity': (), 'grid_map': ('grid_index', 'grid_fstat', 'grid_power', 'grid_map'),
          'grid_seed': ('grid_index', 'grid_fstat', 'grid_power'), 'consistency': ('consistency', 'closure_max', 'element_consistency'),
          'capon_maps': bb.CAPON_FIELDS, 'capon_peaks': bb.CAPON_FIELDS[:4] + bb.PEAK_FIELDS}


@pytest.mark.parametrize('extra', sorted(bb.EXTRAS))
def test_batch_equals_single_calls_one_extra_at_a_time(extra):
    kw = bb.EXTRAS[extra]
    batch = _batch(**kw)
    _check_shape_of_a_batch(batch, WANTED[extra])
    for s in range(bb.S):
        _same(batch[s], _single(s, **kw), label='%s recording %d' % (extra, s))
    if extra in ('subsample', 'min_velocity', 'grid_seed'):          # the option is in force: it moves the plain results
        plain = _batch()
        assert any(not np.array_equal(batch[s].vel, plain[s].vel) for s in range(bb.S))
    assert any(np.any(np.asarray(res.weights)[b, :int(res.nwin[b])] == 0) for res in batch for b in range(bb.B))    # LTS dropped pairs


def test_everything_at_once(all_on):
    """One batch with every option that combines: equal to the single calls with the same keywords, and each extra's
    fields equal to the batch with that extra alone beside the options that change the picks (seed, sub-sample)."""
    _check_shape_of_a_batch(all_on, bb.FIELDS)
    for s in range(bb.S):
        _same(all_on[s], _single(s, **bb.ALL_ON), label='all on, recording %d' % s)
    _all_same(_batch(**bb.PICKS), all_on, bb.PLAIN_FIELDS, 'picks alone')
    for name in sorted(bb.PARTS):
        kw, fields = bb.PARTS[name]
        fields = bb.CAPON_FIELDS + bb.PEAK_FIELDS if fields is None else fields
        _all_same(_batch(**kw), all_on, fields + bb.PLAIN_FIELDS, name + ' alone')


@pytest.mark.parametrize('s', range(bb.S))
def test_two_band_all_on_call_against_the_truths(all_on, s):
    """The single call of recording s with everything on: every band against the truths on ``fetch_filtered(b)`` and THAT
    band's tables, with the checkers, bounds and caps of the single-band files; the call equals the batch's rows, which
    holds rows b > 0, s > 0 of the batch to the truth."""
    rij = bb.recordings()[1]
    res = _single(s, want_lag=True, want_cmax=True, want_z=True, **bb.ALL_ON)
    _same(res, all_on[s], label='single with lags against the batch, recording %d' % s)
    h = res.handle
    xij = planner.co_array(rij)[0]
    np.testing.assert_array_equal(res.xij, xij)
    d, tau = gt.delay_table(xij, bb.SEED_GRID, bb.FS, bb.N)
    assert not gt.near_tie(tau)
    np.testing.assert_array_equal(h.fetch_beam_grid_delays(), d)
    cells = planner.grid_cells(bb.CAPON_GRID)[0]
    for b in range(bb.B):
        label = 'recording %d band %d' % (s, b)
        n, W = int(res.nwin[b]), int(res.W[b])
        filt = h.fetch_filtered(b)
        e = ft.rel_err(filt, bb.filtered_truth(s, b).astype(np.longdouble))
        print('%s: filtered samples against the long-double cascade, %.3g of the scale (stated %.3g)' % (label, e, ft.TOL))
        assert e <= ft.TOL
        grid_check(res, filt, bb.SEED_GRID, band=b, label=label)
        seeded_check(res, filt, K=bb.SEED_HALFWIDTHS[b], band=b)
        fractions_check(res, filt, label, band=b)
        _, on_f = beam_check(res, filt, band=b, label=label)
        assert on_f >= n // 2
        print('%s: closure of the refined lags, worst |d| / bound = %.3g' % (label, closure_check(res, band=b, label=label)))
        capon_check(res, filt, bb.CAPON_GRID, bb.CAPON_SNAPSHOTS[0][b], bb.CAPON_SNAPSHOTS[1][b], bb.CAPON_LOADING, label=label,
                    band=b, freq=bb.CAPON_FREQS[b])
        counts = peaks_check(res, cells, bb.PEAKS, bb.PEAK_FLOOR, label, band=b)
        assert np.all(counts['capon'] >= 1) and np.all(counts['bartlett'] >= 1)
        assert W == bb.WINDOWS[b]
    assert any(np.any(np.asarray(res.weights)[b, :int(res.nwin[b])] == 0) for b in range(bb.B))       # LTS dropped pairs


def test_hbm_rounds_of_one_band_equal_the_plain_batch(all_on, monkeypatch):
    """The second round starts at band 1: every per-band table is sliced with b0 = 1."""
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', repr(1.5 * bb.S * ROW_BYTES / 2.0 ** 30))
    assert engine.max_bands_per_pass(bb.S * bb.N, bb.NPTS) == 1
    _all_same(_batch(**bb.ALL_ON), all_on, label='HBM rounds')
    # ... and the single call in rounds of one band, which slices the tables in ``engine.launch_groups``
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', repr(1.5 * ROW_BYTES / 2.0 ** 30))
    assert engine.max_bands_per_pass(bb.N, bb.NPTS) == 1
    for s in (0, bb.S - 1):
        _same(_single(s, **bb.ALL_ON), all_on[s], label='single call in HBM rounds, recording %d' % s)


def test_sub_batches_of_two_and_one_recordings_equal_the_plain_batch(all_on, monkeypatch):
    """Not one band of the three recordings fits: sub-batches of 2 and 1 recordings, the first in rounds of one band."""
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', repr(2.5 * ROW_BYTES / 2.0 ** 30))
    assert engine.max_bands_per_pass(bb.S * bb.N, bb.NPTS) == 0 and engine.max_bands_per_pass(bb.N, bb.NPTS) == 2
    assert engine.max_bands_per_pass(2 * bb.N, bb.NPTS) == 1
    _all_same(_batch(**bb.ALL_ON), all_on, label='sub-batches')


def _streamed(monkeypatch, h, **kw):
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '1')
    try:
        h.set_option('screen_batch_mb', 1)
        h.set_option('solve_min_units', 1)
        out = _batch(**kw)
        nbatches = h.result_batches()
    finally:
        h.set_option('screen_batch_mb', 192)
        h.set_option('solve_min_units', 0)
        monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    return out, nbatches


def test_streamed_equals_unstreamed(all_on, monkeypatch):
    """A plan with a lag seed correlates every window group on the seeded correlator and solves the pass in one piece: its
    streamed form has ONE result batch whatever the trace's length.  So the seeded all-on batch is compared at the case's
    own length, and the several result batches are those of the same options without the half-widths (the grid search
    stays), on a trace ten times as long: 1 MiB of quantised windows holds 481 units of 257 samples and 1638 of 65, the
    bands have 3 x 186 and 3 x 748, so each band's units come in two batches that cut through its rows."""
    h = engine.get_handle()
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    seeded, nbatches = _streamed(monkeypatch, h, **bb.ALL_ON)
    assert nbatches >= 1
    _all_same(seeded, all_on, label='streamed, seeded')
    long = bb.recordings(10 * (bb.NPTS - 1) + 1)[0]
    kw = {k: v for k, v in bb.ALL_ON.items() if k != 'seed_halfwidths'}
    whole = _batch(long, **kw)
    nwin = whole[0].nwin
    assert 3 * nwin[0] > 2 ** 20 // (8 * 272) and 3 * nwin[1] > 2 ** 20 // (8 * 80)
    streamed, nbatches = _streamed(monkeypatch, h, data=long, **kw)
    print('streamed without the half-widths: %d result batches for %d + %d units' % (nbatches, 3 * nwin[0], 3 * nwin[1]))
    assert nbatches >= 2
    assert nbatches >= 3                                             # more batches than window groups: one cuts a band's rows
    _all_same(streamed, whole, label='streamed')
    _check_shape_of_a_batch(whole, [k for k in bb.FIELDS])


def test_peak_routes_in_a_batch(all_on, monkeypatch):
    """Peaks without the maps on the LDS route, then on the HBM route with so few slabs that one sub-launch of the peak
    kernel holds units of both bands (the unstreamed pass solves all its units in one range, and the units of band 0 come
    first: S * nwin[0] of them)."""
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    kw = dict(bb.ALL_ON, want_capon_maps=False)
    nwin = all_on[0].nwin
    assert not engine.stream_pays(bb.ALPHA, np.tile(nwin, bb.S), bb.N * (bb.N - 1) // 2)
    boundary, units = bb.S * int(nwin[0]), bb.S * int(np.sum(nwin))
    slabs = next(k for k in (8, 7, 6, 5) if boundary % k)
    first = boundary // slabs * slabs                                # the sub-launch [first, first + slabs) ...
    assert first < boundary < first + slabs <= units                # ... is a whole one and holds units of both bands
    fields = [k for k in bb.FIELDS if k not in ('capon_map', 'bartlett_map')]
    for route, nslabs in ((1, 0), (2, slabs)):
        with _options(capon_peak_route=route, capon_peak_slabs=nslabs):
            got = _batch(**kw)
        assert got[0].capon_map is None and got[0].capon_peak_count is not None
        _all_same(got, all_on, fields, 'route %d' % route)
    with _options(capon_peak_route=2, capon_peak_slabs=slabs):       # ... and where the slab is the unit's rows of the maps
        _all_same(_batch(**bb.ALL_ON), all_on, label='route 2 with the maps')
