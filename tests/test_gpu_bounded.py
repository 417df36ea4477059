"""The bounded lag search (``nbls_set_lag_limits``, csrc/xcorr_bounded.hip) on the GPU: both forms
against the NumPy statement of tests/bounded_truth.py — on noise, on unit pulses at the tile edges of the matrix-core form,
on ties, empty ranges, dead channels and windows that are not finite —, the bit-for-bit equalities between the forms of a
pass, the public calls against the picks composed with the oracle's solvers, and the argument checks.  All passes are
pre-filtered (``nsections == 0``): the CPU holds the identical samples."""
import numpy as np
import pytest

import bounded_truth as bt
import refine_truth as rt
from narrow_band_least_squares_amd import (engine, planner, synthetic, _hip, ltsva_bounded, ltsva_batch, ltsva_multi,
                                           narrow_band_least_squares_bounded)

pytestmark = pytest.mark.gpu

FS = 20.0
T0 = 17884.0729166667
BIG = 10 ** 6


def _geometry(N, seed=5):
    rng = np.random.default_rng(seed)
    rij = rng.uniform(-1.0, 1.0, (2, N))
    return rij - rij.mean(axis=1, keepdims=True)


def _pass(data, W, inc, limits=None, xcorr_impl=0, timings=False):
    """One pre-filtered OLS pass of ``data`` (N, npts) through ``Handle`` with the given limit table (None: the plain pass)
    -> (lag (nwin, P), cmax (nwin, P)[, timings])."""
    data = np.ascontiguousarray(data, dtype=np.float64)
    N, npts = data.shape
    xij, pair_idx, xpinv = planner.co_array(_geometry(N))
    nwin = len(range(0, npts - W, inc))
    h = engine.get_handle()
    if getattr(h, 'est_npairs', None):
        h.set_estimators(())
    h.set_trace(data, FS)
    h.set_geometry(xij, pair_idx, xpinv)
    h.set_uncertainty(None)
    h.set_profiling(timings)
    h.set_lag_limits(limits)
    try:
        h.plan(None, False, None, None, [W], [inc], nwin, xcorr_impl=xcorr_impl)
    finally:
        h.set_lag_limits(None)                     # (the handle is shared with calls that plan for themselves)
    try:
        h.stream_results(False)
        h.execute()
        out = h.fetch(want_lag=True, want_cmax=True)
        tim = h.timings() if timings else None
    finally:
        h.set_profiling(False)
    assert int(out['nwin'][0]) == nwin
    res = (out['lag'][0, :nwin].astype(np.int64), out['cmax'][0, :nwin])
    return res + (tim,) if timings else res


def _noise(N, W, nwin=5, seed=0):
    inc = W // 2
    npts = W + (nwin - 1) * inc + 1
    return np.random.default_rng(4100 + 37 * N + W + seed).standard_normal((N, npts)), inc, [w * inc for w in range(nwin)]


def _mixed_limits(P, W, shift):
    cyc = [0, 1, W // 3, W - 1, BIG]
    return np.array([cyc[(k + shift) % 5] for k in range(P)], dtype=np.int64)


# ---- 1. parity on noise ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shift', [0, 3])
@pytest.mark.parametrize('N,W,form', [(3, 16, 1), (4, 65, 1), (8, 130, 1), (16, 64, 1), (17, 48, 2)])
def test_parity_on_noise(N, W, form, shift):
    """Lags exact and cmax to 1e-12 against the slice arg-max of NumPy; the limit table mixes 0, 1, W // 3, W-1 and 10^6
    across the pairs (two rotations, so that 3 pairs see all five too)."""
    data, inc, starts = _noise(N, W)
    pairs = bt.pair_table(N)
    lim = _mixed_limits(len(pairs), W, shift)
    assert _hip.lag_limit_form(N, W, int(lim.min())) == form
    exp_lag, exp_cmax = bt.pick_windows(data, W, starts, pairs, lim)
    lag, cmax = _pass(data, W, inc, lim)
    print('N=%d W=%d: worst |d cmax| %.3g' % (N, W, np.max(np.abs(cmax - exp_cmax))))
    np.testing.assert_array_equal(lag, exp_lag)
    np.testing.assert_allclose(cmax, exp_cmax, rtol=0, atol=1e-12)
    assert np.all(np.abs(lag) <= np.minimum(lim, W - 1)[None, :])
    full = lim >= W - 1                                     # these pairs are searched over every lag: the plain pick
    plain_lag, _ = _pass(data, W, inc)
    np.testing.assert_array_equal(lag[:, full], plain_lag[:, full])
    assert np.any(lag[:, ~full] != plain_lag[:, ~full])


def test_the_two_forms_agree_at_8_x_130():
    """A 17-element pass (general form) whose first 8 rows are the data of the 8-element pass (matrix-core form): the 28
    shared pairs have equal lags and cmax within 1e-12."""
    W = 130
    data8, inc, starts = _noise(8, W)
    data17 = np.concatenate([data8, _noise(9, W, seed=1)[0]])
    lim8 = _mixed_limits(28, W, 1)
    p17 = bt.pair_table(17)
    lim17 = np.full(len(p17), W // 4, dtype=np.int64)
    shared = [k for k, (i, j) in enumerate(p17) if j < 8]
    assert [p17[k] for k in shared] == bt.pair_table(8)
    lim17[shared] = lim8
    assert _hip.lag_limit_form(8, W, int(lim8.min())) == 1 and _hip.lag_limit_form(17, W, int(lim17.min())) == 2
    bt.pick_windows(data17, W, starts, p17, lim17)          # (the gap of every pair)
    lag8, cmax8 = _pass(data8, W, inc, lim8)
    lag17, cmax17 = _pass(data17, W, inc, lim17)
    np.testing.assert_array_equal(lag17[:, shared], lag8)
    np.testing.assert_allclose(cmax17[:, shared], cmax8, rtol=0, atol=1e-12)


# ---- 2. tile edges with unit pulses ------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [8, 4])
@pytest.mark.parametrize('L', [15, 16, 17, 31, 32, 33, 79, 80, 81])
def test_pulses_at_the_tile_edges(N, L):
    """W = 130; 8 elements step their lag blocks by 32, 4 elements by 80.  Element 0 holds a unit pulse, every other
    element a unit pulse at lag m and a 0.5 pulse at lag 2 (all sums exact); one window per m in {L, L+1, -L, -L-1}:
    inside the range the pick is m, outside it is 2."""
    W = 130
    assert _hip.route(N, W, xcorr_impl=2)['S'] * 16 == {8: 32, 4: 80}[N]
    ms = [L, L + 1, -L, -L - 1]
    data = np.zeros((N, len(ms) * W + 1))
    for w, m in enumerate(ms):
        pa = 10 if m > 0 else 110
        data[0, w * W + pa] = 1.0
        data[1:, w * W + pa + m] = 1.0
        data[1:, w * W + pa + 2] = 0.5
    pairs = bt.pair_table(N)
    lim = np.full(len(pairs), L)
    assert _hip.lag_limit_form(N, W, L) == 1
    exp_lag, exp_cmax = bt.pick_windows(data, W, [w * W for w in range(len(ms))], pairs, lim, exact=True)
    lag, cmax = _pass(data, W, W, lim)
    np.testing.assert_array_equal(lag, exp_lag)
    np.testing.assert_allclose(cmax, exp_cmax, rtol=0, atol=1e-12)
    for w, m in enumerate(ms):
        inside = abs(m) <= L
        np.testing.assert_array_equal(lag[w, :N - 1], m if inside else 2, err_msg='m = %d' % m)
        np.testing.assert_allclose(cmax[w, :N - 1], (1.0 if inside else 0.5) / np.sqrt(1.25), rtol=0, atol=1e-15)


# ---- 3. ties and empties -----------------------------------------------------------------------------------------------
def _tie_trace(N, W):
    """Windows: 0 two equal pulses inside the range (lags 3, -5); 1 one inside (4), one outside (20); 2 both outside
    (20, -30); 3 as window 0 with element 1 dead."""
    cases = [(3, -5), (4, 20), (20, -30), (3, -5)]
    data = np.zeros((N, len(cases) * W + 1))
    for w, (m1, m2) in enumerate(cases):
        data[0, w * W + 32] = 1.0
        data[1:, w * W + 32 + m1] = 1.0
        data[1:, w * W + 32 + m2] = 1.0
    data[1, 3 * W:4 * W] = 0.0
    return data, len(cases)


@pytest.mark.parametrize('N,form', [(4, 1), (17, 2)])
def test_ties_empty_ranges_and_a_dead_channel(N, form):
    W, L = 64, 10
    data, n = _tie_trace(N, W)
    pairs = bt.pair_table(N)
    lim = np.full(len(pairs), L)
    assert _hip.lag_limit_form(N, W, L) == form
    with np.errstate(invalid='ignore'):
        exp_lag, exp_cmax = bt.pick_windows(data, W, [w * W for w in range(n)], pairs, lim, exact=True)
    lag, cmax = _pass(data, W, W, lim)
    np.testing.assert_array_equal(lag, exp_lag)
    np.testing.assert_allclose(cmax, exp_cmax, rtol=0, atol=1e-12, equal_nan=True)
    first = slice(0, N - 1)                                  # the pairs (0, j)
    np.testing.assert_array_equal(lag[0, first], 3)          # equal maxima: the larger lag
    np.testing.assert_array_equal(lag[1, first], 4)          # the one inside
    np.testing.assert_array_equal(lag[2, first], L)          # nothing inside: +L, cmax 0
    np.testing.assert_array_equal(cmax[2, first], 0.0)
    assert lag[3, 0] == L and np.isnan(cmax[3, 0])           # pair (0, 1) with element 1 dead
    assert lag[3, 1] == 3 and cmax[3, 1] > 0
    # L = 0: the zero lag alone
    lag0, cmax0 = _pass(data, W, W, np.zeros(len(pairs), dtype=np.int64))
    assert not lag0.any()
    e0 = bt.pick_windows(data, W, [w * W for w in range(n)], pairs, np.zeros(len(pairs)), exact=True)[1]
    np.testing.assert_allclose(cmax0, e0, rtol=0, atol=1e-12, equal_nan=True)


# ---- 4. windows that are not finite ------------------------------------------------------------------------------------
@pytest.mark.parametrize('N,W,form', [(4, 65, 1), (17, 48, 2)])
def test_nan_and_inf_windows_take_the_first_nan_of_the_slice(N, W, form):
    """One NaN (window 0), one +Inf (window 1), -Inf and +Inf (window 2): cmax NaN and lag == min(plain pass's lag, L) for
    every pair that touches such an element — what NumPy gives on the slice —, the other pairs as on clean data."""
    data, inc, starts = _noise(N, W, seed=2)
    W2 = 2 * inc
    data = data[:, :2 * W2 + W + 1]
    starts = [0, W2, 2 * W2]                                 # hop of two half-windows: the windows do not share bad samples
    data[1, W // 3] = np.nan
    data[2, W2 + W - 5] = np.inf
    data[0, 2 * W2 + 7] = -np.inf
    data[3, 2 * W2 + W // 2] = np.inf
    pairs = bt.pair_table(N)
    lim = _mixed_limits(len(pairs), W, 2)
    assert _hip.lag_limit_form(N, W, int(lim.min())) == form
    with np.errstate(invalid='ignore'):
        exp_lag, exp_cmax = bt.pick_windows(data, W, starts, pairs, lim)
    lag, cmax = _pass(data, W, W2, lim)
    plain_lag, plain_cmax = _pass(data, W, W2)
    bad = np.isnan(exp_cmax)
    touched = np.array([[(w == 0 and 1 in p) or (w == 1 and 2 in p) or (w == 2 and (0 in p or 3 in p)) for p in pairs]
                        for w in range(3)])
    np.testing.assert_array_equal(bad, touched)
    np.testing.assert_array_equal(np.isnan(cmax), bad)
    np.testing.assert_array_equal(np.isnan(plain_cmax), bad)
    np.testing.assert_array_equal(lag, exp_lag)
    np.testing.assert_array_equal(lag[bad], np.minimum(plain_lag, np.minimum(lim, W - 1)[None, :])[bad])
    np.testing.assert_allclose(cmax[~bad], exp_cmax[~bad], rtol=0, atol=1e-12)


# ---- 5. every limit reaches W-1: the ordinary route --------------------------------------------------------------------
@pytest.mark.parametrize('N,W', [(8, 130), (4, 16)])
def test_limits_that_reach_the_window_take_the_ordinary_route(N, W):
    data, inc, _ = _noise(N, W)
    P = N * (N - 1) // 2
    lim = np.array([W - 1 if k % 2 else BIG for k in range(P)])
    assert _hip.lag_limit_form(N, W, int(lim.min())) == 0
    lag, cmax, tim = _pass(data, W, inc, lim, timings=True)
    plain_lag, plain_cmax, plain_tim = _pass(data, W, inc, timings=True)
    np.testing.assert_array_equal(lag, plain_lag)
    np.testing.assert_array_equal(cmax, plain_cmax)
    assert tim['xcorr_impl'] == plain_tim['xcorr_impl'] and plain_tim['xcorr_impl'] in (1, 2, 3)
    lim[0] = W - 2                                            # one pair short of it: the bounded correlator
    assert _pass(data, W, inc, lim, timings=True)[2]['xcorr_impl'] == 4


# ---- 6. invariance, bit for bit ----------------------------------------------------------------------------------------
VMIN = 0.25


def _wave(N, W, npts, seed, radius=0.15, snr_db=6.0):
    """A narrow-band (1.0-1.1 Hz) plane wave over a compact array: the picks of the full search skip cycles."""
    rij = synthetic.array_geometry(N, radius, seed=seed)
    data = synthetic.plane_wave(rij, npts, FS, 1.0, 1.1, snr_db=snr_db, seed=seed + 1)
    return np.ascontiguousarray(data), np.ascontiguousarray(rij - rij.mean(axis=1, keepdims=True))


def _process(data, rij, W, alpha, overlap=0.5, v=VMIN, **kw):
    res = engine.process(data, FS, T0, rij, [(None, None)], [(W + 0.5) / FS], overlap, alpha, prefiltered=True, want_lag=True,
                         want_cmax=True, want_z=True, min_velocity=v, **kw)
    assert int(res.W[0]) == W
    return res


def _same_tuple(got, exp, n=8):
    assert len(got) == len(exp) == n
    for i in [i for i in range(n) if i != 4]:
        np.testing.assert_array_equal(got[i], exp[i], err_msg='return %d' % i)
    assert list(got[4].keys()) == list(exp[4].keys())
    for k in exp[4]:
        np.testing.assert_array_equal(got[4][k], exp[4][k], err_msg=k)


def _check_against_truth(res, data):
    n, W, inc = int(res.nwin[0]), int(res.W[0]), int(res.inc[0])
    lim = planner.lag_limits(res.xij, FS, VMIN)
    np.testing.assert_array_equal(lim, bt.limits(res.xij, FS, VMIN))
    assert lim.max() < W - 1
    exp_lag, exp_cmax = bt.pick_windows(data, W, [w * inc for w in range(n)], [tuple(p) for p in res.pair_idx], lim)
    np.testing.assert_array_equal(res.lag[0, :n], exp_lag)
    np.testing.assert_allclose(res.cmax[0, :n], exp_cmax, rtol=0, atol=1e-12)
    return lim


def test_streamed_equals_unstreamed(monkeypatch):
    data, rij = _wave(8, 130, 2601, 310)
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    whole = _process(data, rij, 130, 0.5)
    _check_against_truth(whole, data)
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '1')
    streamed = _process(data, rij, 130, 0.5)
    assert streamed.handle.result_batches() >= 1
    for k in ('vel', 'baz', 'mdccm', 'sigma_tau', 'z', 'lag', 'cmax', 'mask'):
        np.testing.assert_array_equal(getattr(streamed, k), getattr(whole, k), err_msg=k)
    plain = engine.process(data, FS, T0, rij, [(None, None)], [130.5 / FS], 0.5, 0.5, prefiltered=True, want_lag=True)
    assert not np.array_equal(plain.lag, whole.lag)


def test_two_window_lengths_stream_a_screened_and_a_bounded_group(monkeypatch):
    """Two bands of two window lengths over a 1 km square at v_min = 0.25 km/s (limits 81 and 115 samples): every limit
    reaches the 64-sample windows of band 0, which keep the screening route, and none the 400-sample windows of band 1,
    which run the bounded correlator — as a result batch of its own behind the screened one in a streamed pass.  Streamed
    against unstreamed bit for bit; ``xcorr_impl`` is 4.  (Two bands need the filter stage: the one pass here that is not
    pre-filtered; nothing is compared with the CPU.)"""
    rij = np.array([[0.0, 1.0, 1.0, 0.0], [0.0, 0.0, 1.0, 1.0]]) - 0.5
    data = synthetic.plane_wave(rij, 4001, FS, 0.5, 2.0, seed=380)
    lim = planner.lag_limits(planner.co_array(rij)[0], FS, VMIN)
    assert sorted(set(lim.tolist())) == [81, 115]
    assert _hip.lag_limit_form(4, 64, int(lim.min())) == 0 and _hip.lag_limit_form(4, 400, int(lim.min())) == 1
    assert _hip.route(4, 64)['correlator'] == _hip.ROUTE_SCREEN

    def run(v, **kw):
        return engine.process(data, FS, T0, rij, [(0.5, 1.0), (1.0, 2.0)], [64.5 / FS, 400.5 / FS], 0.5, 0.5, 'butter', 2, 0.01,
                              want_lag=True, want_cmax=True, want_z=True, min_velocity=v, **kw)
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    whole = run(VMIN, groups=1)
    plain = run(None, groups=1)
    assert [int(w) for w in whole.W] == [64, 400]
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '1')
    h = engine.get_handle()
    h.set_profiling(True)
    try:
        streamed = run(VMIN)
        assert streamed.handle is h and h.result_batches() >= 2
        assert h.timings()['xcorr_impl'] == 4
    finally:
        h.set_profiling(False)
    for k in ('vel', 'baz', 'mdccm', 'sigma_tau', 'z', 'lag', 'cmax', 'mask'):
        np.testing.assert_array_equal(getattr(streamed, k), getattr(whole, k), err_msg=k)
    n0, n1 = int(whole.nwin[0]), int(whole.nwin[1])
    np.testing.assert_array_equal(whole.lag[0], plain.lag[0])                    # form 0: the plain pass's picks
    np.testing.assert_array_equal(whole.cmax[0], plain.cmax[0])
    assert np.all(np.abs(whole.lag[1, :n1]) <= lim[None, :])
    inside = np.abs(plain.lag[1, :n1]) <= lim[None, :]                           # a full-search pick inside the range is the bounded pick
    np.testing.assert_array_equal(whole.lag[1, :n1][inside], plain.lag[1, :n1][inside])
    assert n0 > n1 >= 8 and np.isfinite(whole.vel[1, :n1]).all()


def test_batch_of_two_recordings_equals_two_single_calls():
    recs = [_wave(6, 65, 1301, 320 + i) for i in range(2)]
    rij = recs[0][1]
    sts = [synthetic.make_stream(d, FS, starttime=T0 + i) for i, (d, _) in enumerate(recs)]
    batch = ltsva_batch(sts, None, None, 65.5 / FS, 0.5, alpha=0.5, rij=rij, min_velocity=VMIN)
    assert len(batch) == 2
    for got, s in zip(batch, sts):
        _same_tuple(got, ltsva_bounded(s, None, None, 65.5 / FS, 0.5, VMIN, alpha=0.5, rij=rij))
    plain = ltsva_batch(sts, None, None, 65.5 / FS, 0.5, alpha=0.5, rij=rij)
    assert not np.array_equal(plain[0][3], batch[0][3])                         # MdCCM follows the bounded picks


def test_two_window_slices_add_up_to_the_full_call():
    data, rij = _wave(4, 65, 2401, 330)
    full = _process(data, rij, 65, 0.5)
    parts = [_process(data, rij, 65, 0.5, window_slice=(k, 2)) for k in range(2)]
    n = int(full.nwin[0])
    for k in ('mdccm', 'sigma_tau', 'vel', 'baz'):
        a, b = getattr(parts[0], k), getattr(parts[1], k)
        assert not np.any((a != 0) & (b != 0))                     # rows outside a slice stay zero
        np.testing.assert_array_equal(a + b, getattr(full, k), err_msg=k)
    half = n // 2
    np.testing.assert_array_equal(parts[0].lag[0, :half], full.lag[0, :half])
    np.testing.assert_array_equal(parts[1].lag[0, half:n], full.lag[0, half:n])
    np.testing.assert_array_equal(parts[0].cmax[0, :half], full.cmax[0, :half])
    np.testing.assert_array_equal(parts[1].cmax[0, half:n], full.cmax[0, half:n])


def test_sub_array_estimator_against_the_call_on_the_sub_array():
    """7 of 8 elements: the estimator reads the full array's picks, the separate call correlates 7 elements (other tile
    origins): lags and weights exact, cmax 1e-12, vel / baz 1e-9."""
    data, rij = _wave(8, 130, 2601, 340)
    ests = engine.normalize_estimators([(0.5, ()), (0.5, (7,))], 8)
    rijs = [rij, np.ascontiguousarray(rij[:, :7])]
    multi = engine.process_multi(list(data), FS, [T0] * 2, rijs, [(None, None)], [130.5 / FS], 0.5, ests, prefiltered=True,
                                 want_lag=True, want_cmax=True, min_velocity=VMIN)
    sub = _process(np.ascontiguousarray(data[:7]), rijs[1], 130, 0.5)
    m = engine.kept_pair_map(8, (7,))
    np.testing.assert_array_equal(multi[1].lag, multi[0].lag[..., m])
    np.testing.assert_array_equal(multi[1].lag, sub.lag)
    np.testing.assert_array_equal(multi[1].mask, sub.mask)
    assert np.any(np.unpackbits(sub.mask[0, :int(sub.nwin[0])], axis=-1, bitorder='little')[:, :21] == 0)
    np.testing.assert_allclose(multi[1].cmax, sub.cmax, rtol=0, atol=1e-12)
    np.testing.assert_allclose(multi[1].vel, sub.vel, rtol=1e-9)
    np.testing.assert_allclose(multi[1].baz, sub.baz, rtol=1e-9)
    s = synthetic.make_stream(data, FS, starttime=T0)
    pub = ltsva_multi(s, None, None, 130.5 / FS, 0.5, [(0.5, ()), (0.5, (7,))], rij=rij, min_velocity=VMIN)
    exp = ltsva_bounded(synthetic.make_stream(data[:7], FS, starttime=T0), None, None, 130.5 / FS, 0.5, VMIN, alpha=0.5,
                        rij=rijs[1])
    np.testing.assert_allclose(pub[1][0], exp[0], rtol=1e-9)
    np.testing.assert_allclose(pub[1][1], exp[1], rtol=1e-9)
    np.testing.assert_allclose(pub[1][3], exp[3], rtol=0, atol=1e-12)
    assert list(pub[1][4].keys()) == list(exp[4].keys())


# ---- 7. end to end -----------------------------------------------------------------------------------------------------
def _oracle_rows(oracle, xij, lag, alpha, fs=FS):
    tau = np.ascontiguousarray((lag.astype(np.float64) / fs).T)
    if alpha == 1.0:
        z, _, _, sig = oracle.ols_solve(xij, tau)
        w = np.ones(tau.shape, dtype=np.uint8)
    else:
        z, w, sig = oracle.lts_post_process(tau, xij, oracle.fast_lts(tau, xij, alpha), alpha)
    vel, baz = oracle.vel_baz(z)
    return vel, baz, sig, w


@pytest.mark.parametrize('alpha', [1.0, 0.5])
def test_ltsva_bounded_against_the_picks_composed_with_the_oracle(oracle, alpha):
    N, W = 6, 200
    data, rij = _wave(N, W, 2001, 350)
    res = _process(data, rij, W, alpha, want_uncert=True)
    n = int(res.nwin[0])
    lim = _check_against_truth(res, data)
    plain = engine.process(data, FS, T0, rij, [(None, None)], [(W + 0.5) / FS], 0.5, alpha, prefiltered=True, want_lag=True)
    assert bt.outside(plain.lag[0, :n], lim) > 0 and bt.outside(res.lag[0, :n], lim) == 0
    xij, pairs, _ = planner.co_array(rij)
    vel_o, baz_o, sig_o, w_o = _oracle_rows(oracle, xij, res.lag[0, :n], alpha)
    got = ltsva_bounded(synthetic.make_stream(data, FS, starttime=T0), None, None, (W + 0.5) / FS, 0.5, VMIN, alpha=alpha, rij=rij)
    assert len(got) == 8
    np.testing.assert_allclose(got[0], vel_o, rtol=1e-9, equal_nan=True)
    np.testing.assert_allclose(got[1], baz_o, rtol=1e-9, equal_nan=True)
    np.testing.assert_allclose(got[5], sig_o, rtol=1e-9, atol=1e-12, equal_nan=True)
    np.testing.assert_array_equal(got[3], res.mdccm[0, :n])
    np.testing.assert_array_equal(got[3], np.median(res.cmax[0, :n], axis=1))
    if alpha == 1.0:
        assert got[4] == {}
    else:
        np.testing.assert_array_equal(res.weights[0, :n], w_o.T)
        exp = oracle.stdict_from_weights(w_o, pairs, got[2], N)
        assert set(got[4].keys()) == set(exp.keys()) and got[4]['size'] == N
        for k, v in exp.items():
            np.testing.assert_array_equal(got[4][k], v, err_msg=k)


def test_narrow_band_least_squares_bounded_against_the_picks_composed_with_the_oracle(oracle):
    """One band 1.0-1.1 Hz, OLS: the picks of NumPy on the band the GPU filtered, composed with the oracle's ``ols_solve``."""
    from narrow_band_least_squares_amd import narrow_band_least_squares
    N, WL = 6, 10.0
    rij0 = synthetic.array_geometry(N, 0.15, seed=360)
    rij = np.ascontiguousarray(rij0 - rij0.mean(axis=1, keepdims=True))
    data = synthetic.plane_wave(rij0, 2001, FS, 1.0, 1.1, seed=361)
    s = synthetic.make_stream(data, FS, starttime=T0)
    fr = np.logspace(-2, 1, 16)
    args = ([WL], 0.5, 1.0, s, None, None, 1, np.zeros(16), np.zeros(16), [1.0, 1.1], 'linear', fr, 'butter', 2, 0.01)
    got = narrow_band_least_squares_bounded(*args, rij=rij, min_velocity=VMIN)
    plain = narrow_band_least_squares(*args, rij=rij)
    assert len(got) == len(plain) == 9
    np.testing.assert_array_equal(got[3], plain[3], err_msg='t')
    assert got[6] == plain[6] and got[4] is None
    n, W = got[6][0], int(WL * FS)
    filt = engine.get_handle().fetch_filtered(0)
    xij, pairs, _ = planner.co_array(rij)
    lim = bt.limits(xij, FS, VMIN)
    lag, cmax = bt.pick_windows(filt, W, [w * (W // 2) for w in range(n)], [tuple(p) for p in pairs], lim)
    vel_o, baz_o, sig_o, _ = _oracle_rows(oracle, xij, lag, 1.0)
    np.testing.assert_allclose(got[0][0, :n], vel_o, rtol=1e-9)
    np.testing.assert_allclose(got[1][0, :n], baz_o, rtol=1e-9)
    np.testing.assert_allclose(got[5][0, :n], sig_o, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(got[2][0, :n], np.median(cmax, axis=1), rtol=0, atol=1e-12)
    assert not np.array_equal(got[0], plain[0])


def test_batch_with_beam_and_subsample_refines_the_bounded_picks():
    N, W = 6, 200
    data, rij = _wave(N, W, 2001, 350)
    s = synthetic.make_stream(data, FS, starttime=T0)
    both = ltsva_batch([s], None, None, (W + 0.5) / FS, 0.5, alpha=0.5, rij=rij, beam=True, subsample=True, min_velocity=VMIN)[0]
    assert len(both) == 10
    res = _process(data, rij, W, 0.5, want_subsample=True, want_beam=True, want_uncert=True)
    n = int(res.nwin[0])
    _check_against_truth(res, data)
    for i, k in ((0, 'vel'), (1, 'baz'), (3, 'mdccm'), (5, 'sigma_tau'), (8, 'beam_power'), (9, 'fstat')):
        np.testing.assert_array_equal(both[i], getattr(res, k)[0, :n], err_msg=k)
    ref = rt.refine_windows(data, W, [w * int(res.inc[0]) for w in range(n)], [tuple(p) for p in res.pair_idx], res.lag[0, :n])
    ok = np.abs(ref['D']) >= 2.0 ** 20 * ref['E']
    assert ok.sum() >= ok.size // 2
    assert np.all(np.abs(res.lag_frac[0, :n] - ref['frac'])[ok] <= ref['bound'][ok])
    assert np.count_nonzero(res.lag_frac[0, :n]) > 0


# ---- 8. errors ---------------------------------------------------------------------------------------------------------
def test_argument_checks_and_switching_off():
    N, W = 4, 65
    data, inc, _ = _noise(N, W)
    lim = np.full(6, 5)
    lag, _ = _pass(data, W, inc, lim)
    plain_lag, _ = _pass(data, W, inc)
    assert np.all(np.abs(lag) <= 5) and np.any(np.abs(plain_lag) > 5)
    h = engine.get_handle()
    ip = _hip.C.POINTER(_hip.C.c_int32)
    try:
        h.set_lag_limits(lim)
        with pytest.raises(ValueError, match='negative limit of pair 2'):
            h.set_lag_limits([3, 3, -1, 3, 3, 3])
        neg = np.array([3, 3, -1, 3, 3, 3], dtype=np.int32)
        assert h.lib.nbls_set_lag_limits(h._h, neg.ctypes.data_as(ip), 6) == _hip.NBLS_ERR_ARG
        assert h.lib.nbls_set_lag_limits(h._h, neg.ctypes.data_as(ip), 0) == _hip.NBLS_ERR_ARG
        # the handle is unchanged by the failures: the next plan still takes the table of six
        h.plan(None, False, None, None, [W], [inc], 5)
        h.execute()
        np.testing.assert_array_equal(h.fetch(want_lag=True)['lag'][0, :5], lag)
        with pytest.raises(ValueError, match='xcorr_impl'):          # a forced correlator searches every lag
            h.plan(None, False, None, None, [W], [inc], 5, xcorr_impl=1)
        wl, wi = np.array([W], dtype=np.int32), np.array([inc], dtype=np.int32)
        assert h.lib.nbls_plan(h._h, 1, None, 0, 0, None, None, 0, wl.ctypes.data_as(ip), wi.ctypes.data_as(ip), 5, None,
                               2) == _hip.NBLS_ERR_UNSUPPORTED
        h.set_lag_limits(np.full(5, 5))                              # 5 limits for 6 pairs
        with pytest.raises(ValueError, match='5 lag limits'):
            h.plan(None, False, None, None, [W], [inc], 5)
        assert h.lib.nbls_plan(h._h, 1, None, 0, 0, None, None, 0, wl.ctypes.data_as(ip), wi.ctypes.data_as(ip), 5, None,
                               0) == _hip.NBLS_ERR_ARG
    finally:
        h.set_lag_limits(None)
    h.plan(None, False, None, None, [W], [inc], 5)                   # NULL restores the plain pass
    h.execute()
    np.testing.assert_array_equal(h.fetch(want_lag=True)['lag'][0, :5], plain_lag)


def test_min_velocity_is_checked_before_any_gpu_work():
    data, rij = _wave(4, 65, 601, 370)
    s = synthetic.make_stream(data, FS, starttime=T0)
    for bad in (0.0, -0.3, np.nan, np.inf, True, '0.3', None):
        with pytest.raises(ValueError):
            ltsva_bounded(s, None, None, 65.5 / FS, 0.5, bad, rij=rij)
    for bad in (0.0, True, np.nan):
        with pytest.raises(ValueError):
            ltsva_batch([s, s], None, None, 65.5 / FS, 0.5, rij=rij, min_velocity=bad)
        with pytest.raises(ValueError):
            ltsva_multi(s, None, None, 65.5 / FS, 0.5, [1.0, (1.0, (0,))], rij=rij, min_velocity=bad)
