"""The seeded lag search (``nbls_set_lag_seed``, csrc/xcorr_seeded.hip) on the GPU: both forms against
the NumPy statement of tests/seeded_truth.py evaluated on the GPU's OWN grid maxima and delay table — on noise, at the seams
of the range (one lag, the trips of 64 lanes, the clamp of the centre, ranges on either side of lag 0, the full search, the
LDS fit of the staged form), on ties, empty ranges, dead channels, units without a grid maximum and windows that are not
finite —, the grid results against those of the same plan without a seed, the bit-for-bit equalities between the forms of
a pass, the stage order, the error returns, and the public calls.  Every Handle pass is pre-filtered (``nsections == 0``):
the CPU holds the identical samples."""
import numpy as np
import pytest

import bounded_truth as bt
import refine_truth as rt
import seeded_truth as sdt
from narrow_band_least_squares_amd import (engine, planner, synthetic, _hip, ltsva, ltsva_grid, ltsva_seeded,
                                           narrow_band_least_squares, narrow_band_least_squares_grid,
                                           narrow_band_least_squares_seeded)

pytestmark = pytest.mark.gpu

FS = 20.0
T0 = 17884.0729166667
BIG = 2 ** 31 - 1


def _geometry(N, seed=5):
    rng = np.random.default_rng(seed)
    rij = rng.uniform(-1.0, 1.0, (2, N))
    return rij - rij.mean(axis=1, keepdims=True)


def _steered(delays, seed=6):
    """A geometry and a one-point grid whose delay table is ``delays`` (element 0: 0): x_i = -delays[i] / fs, s = (1, 0), so
    fs (r_0 - r_i) . s = delays[i]; the y coordinates keep the co-array well posed and do not enter."""
    d = np.asarray(delays, dtype=np.float64)
    assert d[0] == 0
    y = np.random.default_rng(seed).uniform(-0.5, 0.5, len(d))
    return np.stack([-d / FS, y]), np.array([[1.0, 0.0]])


def _pass(data, rij, W, inc, grid, K, want_map=False, refine=False, timings=False, xcorr_impl=0, again_stages=None):
    """One pre-filtered OLS pass of ``data`` (N, npts) through ``Handle`` with the slowness grid ``grid`` (None: none) and
    the half-width K (None: no seed) -> dict of lag, cmax (nwin, P), index, fstat, power (nwin,), delays (G, N) and on
    request map, frac, tim.  ``again_stages``: a second ``execute`` of these stages before the fetch."""
    data = np.ascontiguousarray(data, dtype=np.float64)
    N, npts = data.shape
    xij, pair_idx, xpinv = planner.co_array(rij)
    nwin = len(range(0, npts - W, inc))
    h = engine.get_handle()
    if getattr(h, 'est_npairs', None):
        h.set_estimators(())
    h.set_trace(data, FS)
    h.set_geometry(xij, pair_idx, xpinv)
    h.set_uncertainty(None)
    h.set_profiling(timings)
    h.set_beam_grid(grid, want_map)
    h.set_lag_seed(None if K is None else [K])
    h.set_lag_refinement(refine)
    try:
        h.plan(None, False, None, None, [W], [inc], nwin, xcorr_impl=xcorr_impl)
    finally:
        h.set_lag_seed(None)                       # (the handle is shared with calls that plan for themselves)
        h.set_beam_grid(None)
        h.set_lag_refinement(False)
    try:
        h.stream_results(False)
        h.execute()
        if again_stages is not None:
            h.execute(stages=again_stages)
        f = h.fetch(want_lag=True, want_cmax=True)
        out = dict(lag=f['lag'][0, :nwin].astype(np.int64), cmax=f['cmax'][0, :nwin], vel=f['vel'][0, :nwin],
                   baz=f['baz'][0, :nwin], mdccm=f['mdccm'][0, :nwin])
        if grid is not None:
            idx, fstat, power = h.fetch_beam_grid()
            out.update(index=idx[0, :nwin].copy(), fstat=fstat[0, :nwin].copy(), power=power[0, :nwin].copy(),
                       delays=h.fetch_beam_grid_delays())
            if want_map:
                out['map'] = h.fetch_beam_grid_map()[0, :nwin].copy()
        if refine:
            out['frac'] = h.fetch_lag_fraction()[0, :nwin].copy()
        if timings:
            out['tim'] = h.timings()
    finally:
        h.set_profiling(False)
    assert int(f['nwin'][0]) == nwin
    return out


def _noise(N, W, nwin=5, seed=0):
    inc = W // 2
    npts = W + (nwin - 1) * inc + 1
    return np.random.default_rng(5100 + 37 * N + W + seed).standard_normal((N, npts)), inc, [w * inc for w in range(nwin)]


def _truth(got, data, W, starts, K, exact=False):
    """seeded_truth on the GPU's own grid maxima and delay table -> (lag, cmax, centres); asserts the gap of every pair."""
    pairs = bt.pair_table(data.shape[0])
    c = sdt.centres(got['delays'], got['index'], pairs)
    with np.errstate(invalid='ignore'):
        lag, cmax = sdt.pick_windows(data, W, starts, pairs, c, K, exact=exact)
    return lag, cmax, c


def _check(got, data, W, starts, K, exact=False):
    lag, cmax, c = _truth(got, data, W, starts, K, exact)
    np.testing.assert_array_equal(got['lag'], lag)
    np.testing.assert_allclose(got['cmax'], cmax, rtol=0, atol=1e-12, equal_nan=True)
    return lag, cmax, c


# ---- 1. parity on noise, both forms ------------------------------------------------------------------------------------
GRID5 = planner.slowness_grid(3.0, 5)


def test_parity_on_noise_at_8_x_130_and_the_two_forms_agree():
    """8 elements x W = 130, 6 windows, a 5 x 5 grid (its 13 points within 3 s/km): lags exact and cmax to 1e-12 against the
    slice arg-max of NumPy around the GPU's own centres.  A 17-element pass (general form) whose first 8 rows and
    coordinates are those of the 8-element pass, steered by a one-point grid so that both passes have the same centres:
    the 28 shared pairs agree in lags exactly and in cmax to 1e-12."""
    W, K = 130, 9
    data8, inc, starts = _noise(8, W, nwin=6)
    assert _hip.lag_seed_form(8, W, K, 0) == 1 and GRID5.shape == (13, 2)
    got = _pass(data8, _geometry(8), W, inc, GRID5, K, timings=True)
    assert got['tim']['xcorr_impl'] == 5
    lag, cmax, c = _check(got, data8, W, starts, K)
    print('8 x 130: worst |d cmax| %.3g, centres %d .. %d' % (np.max(np.abs(got['cmax'] - cmax)), c.min(), c.max()))
    assert len(np.unique(got['index'])) > 1 and np.all(got['index'] >= 0)
    lo = np.maximum(np.clip(c, -(W - 1), W - 1) - K, -(W - 1))
    assert np.all(got['lag'] >= lo) and np.all(got['lag'] <= np.minimum(np.clip(c, -(W - 1), W - 1) + K, W - 1))
    plain = _pass(data8, _geometry(8), W, inc, None, None)
    assert np.any(plain['lag'] != got['lag'])
    # the two forms on shared rows
    delays = [0, 3, -7, 40, -40, 12, 90, -129] + [5, -5, 60, 1, -1, 20, -20, 33, 0]
    rij17, grid1 = _steered(delays)
    data17 = np.concatenate([data8, _noise(9, W, nwin=6, seed=1)[0]])
    p17 = bt.pair_table(17)
    shared = [k for k, (i, j) in enumerate(p17) if j < 8]
    assert [p17[k] for k in shared] == bt.pair_table(8)
    assert _hip.lag_seed_form(17, W, K, 0) == 2
    g8 = _pass(data8, np.ascontiguousarray(rij17[:, :8]), W, inc, grid1, K)
    g17 = _pass(data17, rij17, W, inc, grid1, K)
    np.testing.assert_array_equal(g8['delays'][0], delays[:8])
    np.testing.assert_array_equal(g17['delays'][0], delays)
    _check(g8, data8, W, starts, K)
    _check(g17, data17, W, starts, K)
    np.testing.assert_array_equal(g17['lag'][:, shared], g8['lag'])
    np.testing.assert_allclose(g17['cmax'][:, shared], g8['cmax'], rtol=0, atol=1e-12)


@pytest.mark.parametrize('N,W', [(3, 48), (16, 48), (17, 65), (32, 48)])
def test_parity_on_noise_at_other_element_counts(N, W):
    K = 7
    data, inc, starts = _noise(N, W, nwin=4)
    assert _hip.lag_seed_form(N, W, K, 0) == (1 if N <= 16 else 2)
    got = _pass(data, _geometry(N), W, inc, GRID5, K, timings=True)
    assert got['tim']['xcorr_impl'] == 5
    _check(got, data, W, starts, K)


# ---- 2. seams of the range ---------------------------------------------------------------------------------------------
STRADDLE = [0, 3, 40, -40, -1, 100, -100, 7]       # centres of the pairs (0, i); the others are their differences


@pytest.mark.parametrize('N,W', [(8, 130), (17, 65)])
@pytest.mark.parametrize('K', [0, 31, 32, 64])
def test_half_widths_at_the_trips_of_64_lanes(N, W, K):
    """2K + 1 = 1, 63, 65 and 129 lags (at W = 65: 129 is every lag) around centres that straddle 0, lie wholly on either
    side and reach the ends of the lag axis, where the clamp cuts the ranges to every length in between."""
    delays = (STRADDLE + [5, -5, 60, 1, -2, 20, -20, 33, 64])[:N]
    rij, grid = _steered(delays)
    data, inc, starts = _noise(N, W, nwin=3, seed=K)
    got = _pass(data, rij, W, inc, grid, K)
    np.testing.assert_array_equal(got['delays'][0], delays)
    assert np.all(got['index'] == 0)
    lag, _, c = _check(got, data, W, starts, K)
    if K == 0:
        np.testing.assert_array_equal(got['lag'], np.clip(c, -(W - 1), W - 1))
    sizes = {sdt.search_range(W, ck, K)[1] - sdt.search_range(W, ck, K)[0] + 1 for ck in c[0]}
    assert 2 * K + 1 in sizes or K == 64 and W == 65


def test_a_range_of_exactly_64_lags():
    """W = 33, K = 32: the centre 1 gives [-31, 32], 64 lags — one full trip of a wave and no second one."""
    W, K = 33, 32
    rij, grid = _steered([0, 1, 2, -3])
    data, inc, starts = _noise(4, W, nwin=3)
    assert sdt.search_range(W, 1, K) == (-31, 32)
    _check(_pass(data, rij, W, inc, grid, K), data, W, starts, K)


@pytest.mark.parametrize('sign', [1, -1])
@pytest.mark.parametrize('N', [4, 17])
def test_centres_at_and_beyond_the_last_lag_are_clamped(N, sign):
    """W = 65: the pairs (0, 1), (0, 2), (0, 3) have centres +-64 = +-(W-1), +-68 and -+70; pair (1, 3) -+134."""
    W, K = 65, 3
    delays = [0, 64 * sign, 68 * sign, -70 * sign] + [2, -2, 30, -30, 9, -9, 50, -50, 1, 64, -64, 13, -13]
    rij, grid = _steered(delays[:N])
    data, inc, starts = _noise(N, W, nwin=3)
    got = _pass(data, rij, W, inc, grid, K)
    lag, _, c = _check(got, data, W, starts, K)
    assert c[0, 0] == 64 * sign and c[0, 1] == 68 * sign and c[0, 2] == -70 * sign
    assert np.all(np.abs(got['lag'][:, :2] - 64 * sign) <= K) and np.all(np.abs(got['lag'][:, 2] + 64 * sign) <= K)
    got0 = _pass(data, rij, W, inc, grid, 0)                       # one lag: the clamped centre itself
    np.testing.assert_array_equal(got0['lag'], np.clip(c, -(W - 1), W - 1))
    _check(got0, data, W, starts, 0)


@pytest.mark.parametrize('N,W', [(8, 130), (17, 65), (4, 16)])
@pytest.mark.parametrize('K', ['2(W-1)', BIG])
def test_a_half_width_of_twice_the_window_is_the_plain_pass(N, W, K):
    K = 2 * (W - 1) if K == '2(W-1)' else K
    delays = (STRADDLE + [5, -5, 60, 1, -2, 20, -20, 33, 64])[:N]
    rij, grid = _steered(delays)
    data, inc, starts = _noise(N, W, nwin=4)
    got = _pass(data, rij, W, inc, grid, K, timings=True)
    plain = _pass(data, rij, W, inc, None, None, timings=True)
    assert got['tim']['xcorr_impl'] == 5 and plain['tim']['xcorr_impl'] in (1, 2, 3)
    np.testing.assert_array_equal(got['lag'], plain['lag'])
    np.testing.assert_allclose(got['cmax'], plain['cmax'], rtol=0, atol=1e-12)
    _check(got, data, W, starts, K)
    np.testing.assert_array_equal(got['lag'], rt.pick_lags(data, W, starts, bt.pair_table(N)))


def test_the_largest_window_of_the_staged_form_and_the_next():
    """16 elements: 16 (W + 1) doubles fit 156 KiB up to W = 1247.  Both sides of the fit, the same samples in the window
    both share: the same picks."""
    N, K = 16, 5
    last = (156 * 1024 // 8) // N - 1
    assert last == 1247 and _hip.lag_seed_form(N, last, K, 0) == 1 and _hip.lag_seed_form(N, last + 1, K, 0) == 2
    delays = [0, 3, -7, 40, -40, 12, 90, -129, 5, -5, 60, 1, -1, 20, -20, 33]
    rij, grid = _steered(delays)
    data = np.random.default_rng(77).standard_normal((N, 2 * (last + 1) + 1))
    for W in (last, last + 1):
        _check(_pass(data, rij, W, W, grid, K), data, W, [0, W], K)


# ---- 3. ties, empty ranges, dead channels ------------------------------------------------------------------------------
def _tie_trace(N, W):
    """Integer-valued unit pulses (all sums exact).  Windows: 0 two equal pulses inside the range (lags 3, -5); 1 one inside
    (4), one outside (20); 2 both outside (20, -30); 3 as window 0 with element 1 dead."""
    cases = [(3, -5), (4, 20), (20, -30), (3, -5)]
    data = np.zeros((N, len(cases) * W + 1))
    for w, (m1, m2) in enumerate(cases):
        data[0, w * W + 32] = 1.0
        data[1:, w * W + 32 + m1] = 1.0
        data[1:, w * W + 32 + m2] = 1.0
    data[1, 3 * W:4 * W] = 0.0
    return data, len(cases)


@pytest.mark.parametrize('N', [4, 17])
def test_ties_take_the_largest_lag_and_empty_ranges_hi(N):
    """Every pair (0, j) has the centre -1 and K = 9: the range [-10, 8]."""
    W, K = 64, 9
    data, n = _tie_trace(N, W)
    rij, grid = _steered([0] + [-1] * (N - 1), seed=8)
    got = _pass(data, rij, W, W, grid, K)
    assert np.all(got['index'] == 0)
    _, _, c = _check(got, data, W, [w * W for w in range(n)], K, exact=True)
    first = slice(0, N - 1)                                  # the pairs (0, j)
    assert np.all(c[:, first] == -1)
    np.testing.assert_array_equal(got['lag'][0, first], 3)   # equal maxima: the larger lag
    np.testing.assert_array_equal(got['lag'][1, first], 4)   # the one inside
    np.testing.assert_array_equal(got['lag'][2, first], 8)   # nothing inside: hi, cmax 0
    np.testing.assert_array_equal(got['cmax'][2, first], 0.0)
    assert got['lag'][3, 0] == 8 and np.isnan(got['cmax'][3, 0])      # pair (0, 1) with element 1 dead
    assert got['lag'][3, 1] == 3 and got['cmax'][3, 1] > 0


@pytest.mark.parametrize('N,W', [(4, 65), (17, 48)])
def test_units_without_a_grid_maximum_and_windows_that_are_not_finite(N, W):
    """A zero-slowness grid point reads every window where it lies.  Window 1 is all zero in every element, window 2 holds
    one NaN sample, window 3 one +Inf sample: no grid point has a ratio there, the index is -1 and the centre 0.  The
    all-zero window gives lag = hi = K and cmax = NaN for every pair; the pairs of the NaN / Inf element likewise; the
    other pairs of those windows the pick around 0."""
    K = 6
    data = np.random.default_rng(5200 + N).standard_normal((N, 4 * W + 1))
    data[:, W:2 * W] = 0.0
    data[1, 2 * W + W // 3] = np.nan
    data[2, 3 * W + W - 5] = np.inf
    got = _pass(data, _geometry(N), W, W, np.array([[0.0, 0.0]]), K)
    np.testing.assert_array_equal(got['index'], [0, -1, -1, -1])
    assert not got['delays'].any()
    pairs = bt.pair_table(N)
    _, _, c = _check(got, data, W, [0, W, 2 * W, 3 * W], K)
    assert not c.any()
    np.testing.assert_array_equal(got['lag'][1], K)
    assert np.all(np.isnan(got['cmax'][1]))
    for w, e in ((2, 1), (3, 2)):
        touched = np.array([e in p for p in pairs])
        np.testing.assert_array_equal(got['lag'][w, touched], K)
        np.testing.assert_array_equal(np.isnan(got['cmax'][w]), touched)
        assert np.all(np.abs(got['lag'][w, ~touched]) <= K)
    assert np.all(np.isfinite(got['cmax'][0]))


# ---- 4. the grid results are those of the plan without a seed ----------------------------------------------------------
@pytest.mark.parametrize('N,W', [(8, 130), (17, 65)])
def test_grid_outputs_are_bit_equal_to_the_plan_without_a_seed(N, W):
    data, inc, _ = _noise(N, W, nwin=6)
    seeded = _pass(data, _geometry(N), W, inc, GRID5, 9, want_map=True)
    grid_only = _pass(data, _geometry(N), W, inc, GRID5, None, want_map=True, timings=True)
    assert grid_only['tim']['xcorr_impl'] in (1, 2, 3)
    for k in ('index', 'fstat', 'power', 'map', 'delays'):
        np.testing.assert_array_equal(seeded[k], grid_only[k], err_msg=k)
    assert np.all(np.isfinite(seeded['map']))
    plain = _pass(data, _geometry(N), W, inc, None, None)
    for k in ('lag', 'cmax', 'vel', 'baz', 'mdccm'):                   # a grid alone changes no pick
        np.testing.assert_array_equal(grid_only[k], plain[k], err_msg=k)


# ---- 5. stages ---------------------------------------------------------------------------------------------------------
def test_the_solve_stage_alone_leaves_picks_and_grid_results_as_they_are():
    W = 65
    data, inc, starts = _noise(4, W, nwin=4)
    once = _pass(data, _geometry(4), W, inc, GRID5, 5)
    _check(once, data, W, starts, 5)
    # (a fetch gives zeros for what a stage that did not run would have written: the solve's rows, recomputed from the
    #  picks in HBM — MdCCM from cmax, the slowness from the lags —, are the witness that those were left alone)
    again = _pass(data, _geometry(4), W, inc, GRID5, 5, again_stages=4)
    for k in ('index', 'fstat', 'power', 'vel', 'baz', 'mdccm'):
        np.testing.assert_array_equal(again[k], once[k], err_msg=k)
    assert np.all(once['index'] >= 0) and once['vel'].all()
    # the correlation stage alone writes picks and grid results (the grids of the solve stage are then zeros)
    corr = _pass(data, _geometry(4), W, inc, GRID5, 5, again_stages=2)
    for k in ('lag', 'cmax', 'index', 'fstat', 'power'):
        np.testing.assert_array_equal(corr[k], once[k], err_msg=k)
    assert not corr['vel'].any()


# ---- 6. the forms of a pass, bit for bit -------------------------------------------------------------------------------
KW = int(planner.seed_halfwidths([1.1], FS)[0])
GRIDW = planner.slowness_grid(4.0, 5)


def _wave(N, W, npts, seed, radius=0.15, snr_db=6.0):
    """A narrow-band (1.0-1.1 Hz) plane wave over a compact array: the picks of the full search skip cycles."""
    rij = synthetic.array_geometry(N, radius, seed=seed)
    data = synthetic.plane_wave(rij, npts, FS, 1.0, 1.1, snr_db=snr_db, seed=seed + 1)
    return np.ascontiguousarray(data), np.ascontiguousarray(rij - rij.mean(axis=1, keepdims=True))


def _process(data, rij, W, alpha, overlap=0.5, K=KW, **kw):
    res = engine.process(data, FS, T0, rij, [(None, None)], [(W + 0.5) / FS], overlap, alpha, prefiltered=True, want_lag=True,
                         want_cmax=True, want_z=True, slowness_grid=GRIDW, seed_halfwidths=K, **kw)
    assert int(res.W[0]) == W
    return res


def _check_res(res, data, K=KW, band=0):
    n, W, inc = int(res.nwin[band]), int(res.W[band]), int(res.inc[band])
    pairs = [tuple(p) for p in res.pair_idx]
    c = sdt.centres(res.handle.fetch_beam_grid_delays(), res.grid_index[band, :n], pairs)
    lag, cmax = sdt.pick_windows(data, W, [w * inc for w in range(n)], pairs, c, K)
    np.testing.assert_array_equal(res.lag[band, :n], lag)
    np.testing.assert_allclose(res.cmax[band, :n], cmax, rtol=0, atol=1e-12)
    return lag


GRID_KEYS = ('grid_index', 'grid_fstat', 'grid_power')
ROW_KEYS = ('vel', 'baz', 'mdccm', 'sigma_tau', 'z', 'lag', 'cmax', 'mask')


def test_half_a_period_at_the_test_rate():
    assert KW == 9 and GRIDW.shape == (13, 2)


def test_streamed_equals_unstreamed(monkeypatch):
    data, rij = _wave(8, 130, 2601, 310)
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    whole = _process(data, rij, 130, 0.5)
    _check_res(whole, data)
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '1')
    streamed = _process(data, rij, 130, 0.5)
    assert streamed.handle.result_batches() >= 1
    for k in ROW_KEYS + GRID_KEYS:
        np.testing.assert_array_equal(getattr(streamed, k), getattr(whole, k), err_msg=k)
    plain = engine.process(data, FS, T0, rij, [(None, None)], [130.5 / FS], 0.5, 0.5, prefiltered=True, want_lag=True)
    assert not np.array_equal(plain.lag, whole.lag)


def test_batch_of_two_recordings_equals_two_single_calls():
    recs = [_wave(6, 65, 1301, 320 + i) for i in range(2)]
    rij = recs[0][1]
    batch = engine.process_batch([list(d) for d, _ in recs], FS, [T0, T0 + 1.0], rij, [(None, None)], [65.5 / FS], 0.5, 0.5,
                                 prefiltered=True, slowness_grid=GRIDW, seed_halfwidths=KW)
    assert len(batch) == 2
    for got, (d, _) in zip(batch, recs):
        single = _process(d, rij, 65, 0.5)
        _check_res(single, d)
        for k in ('vel', 'baz', 'mdccm', 'sigma_tau', 'mask') + GRID_KEYS:
            np.testing.assert_array_equal(getattr(got, k), getattr(single, k), err_msg=k)


def test_two_window_slices_add_up_to_the_full_call():
    data, rij = _wave(4, 65, 2401, 330)
    full = _process(data, rij, 65, 0.5)
    _check_res(full, data)
    parts = [_process(data, rij, 65, 0.5, window_slice=(k, 2)) for k in range(2)]
    n = int(full.nwin[0])
    for k in ('mdccm', 'sigma_tau', 'vel', 'baz', 'grid_fstat', 'grid_power'):
        a, b = getattr(parts[0], k), getattr(parts[1], k)
        assert not np.any((a != 0) & (b != 0))                     # rows outside a slice stay zero
        np.testing.assert_array_equal(a + b, getattr(full, k), err_msg=k)
    half = n // 2
    for k in ('lag', 'cmax', 'grid_index'):
        np.testing.assert_array_equal(getattr(parts[0], k)[0, :half], getattr(full, k)[0, :half], err_msg=k)
        np.testing.assert_array_equal(getattr(parts[1], k)[0, half:n], getattr(full, k)[0, half:n], err_msg=k)


def test_refinement_and_beam_follow_the_seeded_picks():
    N, W = 6, 200
    data, rij = _wave(N, W, 2001, 350)
    res = _process(data, rij, W, 0.5, want_subsample=True, want_beam=True, want_uncert=True)
    n = int(res.nwin[0])
    lag = _check_res(res, data)
    ref = rt.refine_windows(data, W, [w * int(res.inc[0]) for w in range(n)], [tuple(p) for p in res.pair_idx], lag)
    ok = np.abs(ref['D']) >= 2.0 ** 20 * ref['E']
    assert ok.sum() >= ok.size // 2
    assert np.all(np.abs(res.lag_frac[0, :n] - ref['frac'])[ok] <= ref['bound'][ok])
    assert np.count_nonzero(res.lag_frac[0, :n]) > 0
    assert np.all(np.isfinite(res.fstat[0, :n])) and np.any(np.isfinite(res.vel_uncert[0, :n]))   # (an interval may be NaN)
    coarse = _process(data, rij, W, 0.5)
    np.testing.assert_array_equal(coarse.lag, res.lag)
    assert not np.array_equal(coarse.vel, res.vel)


def test_sub_array_estimator_against_the_call_on_the_sub_array():
    """7 of 8 elements under a one-point grid (the same centres for the full array and the sub-array, whatever their beams
    prefer): the estimator reads the full array's picks, the separate call correlates 7 elements: lags and weights exact."""
    N, W, K = 8, 130, 9
    data, rij = _wave(N, W, 1301, 340)
    grid = np.array([[1.5, -1.0]])
    inc = W // 2
    nwin = len(range(0, data.shape[1] - W, inc))
    sub_rij = np.ascontiguousarray(rij[:, :7])
    xij7, pidx7, xpinv7 = planner.co_array(sub_rij)
    lts8, lts7 = planner.lts_plan(planner.co_array(rij)[0], 0.5), planner.lts_plan(xij7, 0.5)
    h = engine.get_handle()

    def run(d, r, lts, ests):
        xij, pair_idx, xpinv = planner.co_array(r)
        h.set_trace(np.ascontiguousarray(d), FS)
        h.set_geometry(xij, pair_idx, xpinv)
        h.set_estimators(ests)
        h.set_uncertainty(None)
        h.set_beam_grid(grid)
        h.set_lag_seed([K])
        try:
            h.plan(None, False, None, None, [W], [inc], nwin, lts=lts)
        finally:
            h.set_lag_seed(None)
            h.set_beam_grid(None)
        h.stream_results(False)
        h.execute()
        return [h.fetch(want_lag=True, want_cmax=True, want_weights=True, est=e) for e in range(len(ests) + 1)]
    try:
        full, est = run(data, rij, lts8, [dict(kept=np.arange(7), xij=xij7, pair_idx=pidx7, xpinv=xpinv7, lts=lts7, eig6=None)])
        d8 = h.fetch_beam_grid_delays()
        (sub,) = run(data[:7], sub_rij, lts7, [])
        d7 = h.fetch_beam_grid_delays()
    finally:
        h.set_estimators(())
    np.testing.assert_array_equal(d8[:, :7], d7)
    m = engine.kept_pair_map(8, (7,))
    np.testing.assert_array_equal(est['lag'], full['lag'][..., m])
    np.testing.assert_array_equal(est['lag'], sub['lag'])
    np.testing.assert_array_equal(est['weights'], sub['weights'])
    np.testing.assert_allclose(est['cmax'], sub['cmax'], rtol=0, atol=1e-12)
    np.testing.assert_allclose(est['vel'], sub['vel'], rtol=1e-9)
    assert np.any(sub['weights'][0, :nwin] == 0)


# ---- 7. errors ---------------------------------------------------------------------------------------------------------
def test_error_returns_and_switching_off():
    N, W = 4, 65
    data, inc, starts = _noise(N, W)
    rij = _geometry(N)
    seeded = _pass(data, rij, W, inc, GRID5, 5)
    plain = _pass(data, rij, W, inc, None, None)
    assert np.any(seeded['lag'] != plain['lag'])
    h = engine.get_handle()
    ip = _hip.C.POINTER(_hip.C.c_int32)
    wl, wi = np.array([W], dtype=np.int32), np.array([inc], dtype=np.int32)

    def raw_plan(nbands=1, impl=0):
        w2, i2 = np.repeat(wl, nbands), np.repeat(wi, nbands)
        return h.lib.nbls_plan(h._h, nbands, None, 0, 0, None, None, 0, w2.ctypes.data_as(ip), i2.ctypes.data_as(ip), 5, None, impl)
    try:
        h.set_lag_seed([5])
        with pytest.raises(ValueError, match='negative half-width of band 1'):
            h.set_lag_seed([3, -1])
        neg = np.array([3, -1], dtype=np.int32)
        assert h.lib.nbls_set_lag_seed(h._h, neg.ctypes.data_as(ip), 2) == _hip.NBLS_ERR_ARG
        assert h.lib.nbls_set_lag_seed(h._h, neg.ctypes.data_as(ip), 0) == _hip.NBLS_ERR_ARG
        assert h.lib.nbls_set_lag_seed(h._h, neg.ctypes.data_as(ip), -1) == _hip.NBLS_ERR_ARG
        # a seed without a grid
        with pytest.raises(_hip.NblsError, match='needs a slowness grid'):
            h.plan(None, False, None, None, [W], [inc], 5)
        assert raw_plan() == _hip.NBLS_ERR_STATE
        # the handle is unchanged by the failed setters: with a grid the next plan takes the table of one
        h.set_beam_grid(GRID5)
        h.plan(None, False, None, None, [W], [inc], 5)
        h.execute()
        np.testing.assert_array_equal(h.fetch(want_lag=True)['lag'][0, :5], seeded['lag'])
        for impl in (1, 2, 3):                                       # a forced correlator searches every lag
            with pytest.raises(ValueError, match='xcorr_impl'):
                h.plan(None, False, None, None, [W], [inc], 5, xcorr_impl=impl)
            assert raw_plan(impl=impl) == _hip.NBLS_ERR_UNSUPPORTED
        h.set_lag_limits(np.full(6, 5))                              # one restriction at a time
        with pytest.raises(ValueError, match='lag limits'):
            h.plan(None, False, None, None, [W], [inc], 5)
        assert raw_plan() == _hip.NBLS_ERR_UNSUPPORTED
        h.set_lag_limits(None)
        h.set_lag_seed([5, 5])                                       # two half-widths for one band
        with pytest.raises(ValueError, match='2 seed half-widths'):
            h.plan(None, False, None, None, [W], [inc], 5)
        assert raw_plan() == _hip.NBLS_ERR_ARG
    finally:
        h.set_lag_limits(None)
        h.set_lag_seed(None)
        h.set_beam_grid(None)
    h.plan(None, False, None, None, [W], [inc], 5)                   # NULL restores the plain pass
    h.execute()
    np.testing.assert_array_equal(h.fetch(want_lag=True)['lag'][0, :5], plain['lag'])


# ---- 8. the public functions -------------------------------------------------------------------------------------------
def _same(got, exp, skip=()):
    assert len(got) == len(exp)
    for i, (a, b) in enumerate(zip(got, exp)):
        if i in skip:
            continue
        if isinstance(b, dict):
            assert list(a.keys()) == list(b.keys())
            for k in b:
                np.testing.assert_array_equal(a[k], b[k], err_msg='return %d key %s' % (i, k))
        else:
            np.testing.assert_array_equal(a, b, err_msg='return %d' % i)


@pytest.mark.parametrize('alpha', [1.0, 0.5])
def test_ltsva_seeded(alpha):
    N, W = 6, 200
    rij0 = synthetic.array_geometry(N, 0.15, seed=360)
    rij = np.ascontiguousarray(rij0 - rij0.mean(axis=1, keepdims=True))
    data = synthetic.plane_wave(rij0, 2001, FS, 1.0, 1.1, seed=361)
    s = synthetic.make_stream(data, FS, starttime=T0)
    got = ltsva_seeded(s, None, None, (W + 0.5) / FS, 0.5, GRIDW, KW, alpha=alpha, rij=rij, grid_map=True)
    res = _process(data, rij, W, alpha, want_uncert=True, want_grid_map=True)
    n = int(res.nwin[0])
    _check_res(res, data)
    assert len(got) == 14 and all(len(got[i]) == n for i in (0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13))
    assert got[13].shape == (n, len(GRIDW)) and got[12].dtype == np.int32
    for i, k in ((0, 'vel'), (1, 'baz'), (3, 'mdccm'), (5, 'sigma_tau'), (6, 'vel_uncert'), (7, 'baz_uncert'), (10, 'grid_fstat'),
                 (11, 'grid_power'), (12, 'grid_index'), (13, 'grid_map')):
        np.testing.assert_array_equal(got[i], getattr(res, k)[0, :n], err_msg=k)
    assert (got[4] == {}) if alpha == 1.0 else (got[4]['size'] == N)
    grid_only = ltsva_grid(s, None, None, (W + 0.5) / FS, 0.5, GRIDW, alpha=alpha, rij=rij, grid_map=True)
    _same(got[8:], grid_only[8:])                                    # the grid returns are ltsva_grid's
    assert len(ltsva_seeded(s, None, None, (W + 0.5) / FS, 0.5, GRIDW, KW, alpha=alpha, rij=rij)) == 13
    # the full search: ltsva's values
    full = ltsva_seeded(s, None, None, (W + 0.5) / FS, 0.5, GRIDW, 2 * (W - 1), alpha=alpha, rij=rij)
    plain = ltsva(s, None, None, (W + 0.5) / FS, 0.5, alpha=alpha, rij=rij)
    for i in (0, 1, 5, 6, 7):
        np.testing.assert_allclose(full[i], plain[i], rtol=1e-9, equal_nan=True, err_msg='return %d' % i)
    np.testing.assert_allclose(full[3], plain[3], rtol=0, atol=1e-12)
    np.testing.assert_array_equal(full[2], plain[2])
    assert list(full[4].keys()) == list(plain[4].keys())


def test_narrow_band_least_squares_seeded():
    """Two bands, OLS: the documented tuple and shapes; the first nine values equal a direct engine pass with the
    half-widths of the bands' upper edges, as one band group or as two; a direct pass at the full search's half-width gives
    the values of ``narrow_band_least_squares`` itself."""
    N, WL = 6, 10.0
    rij0 = synthetic.array_geometry(N, 0.15, seed=360)
    rij = np.ascontiguousarray(rij0 - rij0.mean(axis=1, keepdims=True))
    data = synthetic.plane_wave(rij0, 2001, FS, 0.5, 2.0, seed=361)
    s = synthetic.make_stream(data, FS, starttime=T0)
    fr = np.logspace(-2, 1, 16)
    freqlist = [0.5, 1.0, 2.0]
    args = ([WL, WL], 0.5, 1.0, s, None, None, 2, np.zeros(16), np.zeros(16), freqlist, 'linear', fr, 'butter', 2, 0.01)
    got = narrow_band_least_squares_seeded(*args, rij=rij, slowness_grid=GRIDW, grid_map=True)
    grid_only = narrow_band_least_squares_grid(*args, rij=rij, slowness_grid=GRIDW, grid_map=True)
    plain = narrow_band_least_squares(*args, rij=rij)
    assert len(got) == 15 and len(plain) == 9
    VL = plain[0].shape[1]
    for i in (0, 1, 2, 3, 5, 9, 10, 11, 12, 13):
        assert got[i].shape == (2, VL), i
    assert got[14].shape == (2, VL, len(GRIDW)) and got[13].dtype == np.int32
    np.testing.assert_array_equal(got[3], plain[3], err_msg='t')
    assert got[6] == plain[6] and got[4] is None
    _same(got[9:], grid_only[9:])
    _same(got[7:9], plain[7:9])
    K = planner.seed_halfwidths([1.0, 2.0], FS)
    assert K.tolist() == [10, 5]
    rows, fs, t0 = engine.stream_rows(s)
    res = engine.process(rows, fs, t0, rij, [(0.5, 1.0), (1.0, 2.0)], [WL, WL], 0.5, 1.0, 'butter', 2, 0.01, vector_len=VL,
                         want_lag=True, slowness_grid=GRIDW, seed_halfwidths=K)
    for i, k in ((0, 'vel'), (1, 'baz'), (2, 'mdccm'), (5, 'sigma_tau')):
        np.testing.assert_array_equal(got[i], getattr(res, k), err_msg=k)
    W = int(WL * FS)
    n = got[6][0]
    d = res.handle.fetch_beam_grid_delays()
    for b in range(2):                                               # every pick lies within K_b of its centre
        c = np.clip(sdt.centres(d, res.grid_index[b, :n], [tuple(p) for p in res.pair_idx]), -(W - 1), W - 1)
        assert np.all(np.abs(res.lag[b, :n] - c) <= K[b])
    # two band groups, each a plan of its own with its own band's half-width: the same rows
    split = engine.process(rows, fs, t0, rij, [(0.5, 1.0), (1.0, 2.0)], [WL, WL], 0.5, 1.0, 'butter', 2, 0.01, vector_len=VL,
                           want_lag=True, slowness_grid=GRIDW, seed_halfwidths=K, groups=2)
    for k in ('vel', 'baz', 'mdccm', 'sigma_tau', 'lag') + GRID_KEYS:
        np.testing.assert_array_equal(getattr(split, k), getattr(res, k), err_msg=k)
    # (a clean broad-band wave: the seeded picks may well be the plain ones; the picks that differ are tested above)
    # K_b = fs / fmax_b at period_fraction 1 is still not the full search; a direct pass with K = 2 (W-1) is the plain call
    full = engine.process(rows, fs, t0, rij, [(0.5, 1.0), (1.0, 2.0)], [WL, WL], 0.5, 1.0, 'butter', 2, 0.01, vector_len=VL,
                          slowness_grid=GRIDW, seed_halfwidths=2 * (W - 1))
    np.testing.assert_allclose(full.vel, plain[0], rtol=1e-9)
    np.testing.assert_allclose(full.baz, plain[1], rtol=1e-9)
    np.testing.assert_allclose(full.mdccm, plain[2], rtol=0, atol=1e-12)
