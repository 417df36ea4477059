"""tests/bounded_truth.py (the NumPy statement of the bounded lag search) against brute-force loops,
the clamp rule for windows that are not finite, and the experiment that shows what the bounded search buys.  CPU only."""
import numpy as np
import pytest

import bounded_truth as bt


@pytest.mark.parametrize('W', [2, 3, 16, 65])
def test_pick_equals_the_brute_force_loops(W):
    rng = np.random.default_rng(50 + W)
    for L in (0, 1, 3, W - 1, W + 5):
        for _ in range(3):
            a, b = rng.standard_normal(W), rng.standard_normal(W)
            lag, cmax, gap = bt.pick(a, b, L)
            blag, bcmax = bt.pick_brute(a, b, L)
            assert lag == blag and abs(cmax - bcmax) <= 1e-14
            assert abs(lag) <= min(L, W - 1) and gap > 0
            if L >= W - 1:                                   # the full search: lag = W-1-argmax
                c = np.correlate(a, b, 'full')
                assert lag == W - 1 - int(np.argmax(c))


def test_ties_take_the_largest_lag_and_empty_ranges_plus_L():
    W = 32
    a, b = np.zeros(W), np.zeros(W)
    a[10] = 1.0
    b[10 + 3] = b[10 - 5] = 1.0                              # R(3) = R(-5) = 1
    assert bt.pick(a, b, 8)[:2] == (3, 1.0 / np.sqrt(2.0))
    assert bt.pick(a, b, 4)[0] == 3 and bt.pick(a, b, 2)[:2] == (2, 0.0)      # nothing inside: +L, cmax 0
    assert bt.pick_brute(a, b, 8)[0] == 3 and bt.pick_brute(a, b, 2)[0] == 2
    lag, cmax, _ = bt.pick(a, np.zeros(W), 6)                # dead channel
    assert lag == 6 and np.isnan(cmax)
    assert bt.pick(a, b, 0)[:2] == (0, 0.0)


@pytest.mark.parametrize('W', [2, 3, 16, 65])
@pytest.mark.parametrize('case', ['nan', 'inf', 'minus_inf_and_inf'])
def test_non_finite_windows_clamp_the_plain_lag(W, case):
    """cmax = NaN and lag = min(the full search's lag, L): the first NaN of the slice."""
    rng = np.random.default_rng(60 + W)
    for L in (0, 1, 3, W - 1, W + 5):
        for trial in range(4):
            a, b = rng.standard_normal(W), rng.standard_normal(W)
            x = a if trial % 2 else b
            x[rng.integers(W)] = np.nan if case == 'nan' else np.inf
            if case == 'minus_inf_and_inf':
                (b if trial % 2 else a)[rng.integers(W)] = -np.inf
            full = bt.pick(a, b, W - 1)
            lag, cmax, gap = bt.pick(a, b, L)
            assert np.isnan(cmax) and np.isnan(full[1]) and (np.isnan(gap) or L == 0)     # (one lag: no second-best)
            assert lag == min(full[0], min(L, W - 1))
            assert bt.pick_brute(a, b, L)[0] == lag


def test_limits_and_pick_windows():
    xij = np.array([[0.3, 0.4], [0.0, 0.0], [1.0, 0.0], [0.1, 0.0]])
    np.testing.assert_array_equal(bt.limits(xij, 40.0, 0.25), [81, 1, 161, 17])
    data = np.random.default_rng(3).standard_normal((3, 100))
    lag, cmax = bt.pick_windows(data, 16, [0, 8, 16], bt.pair_table(3), [0, 4, 100])
    assert lag.shape == cmax.shape == (3, 3) and not lag[:, 0].any() and np.all(np.abs(lag[:, 1]) <= 4)
    assert bt.outside(np.array([[3, -5, 0]]), [3, 4, 0]) == 1
    with pytest.raises(AssertionError):                       # an exact tie is refused unless the case says it is one
        tie = np.zeros((2, 20))
        tie[0, 10] = tie[1, 13] = tie[1, 5] = 1.0
        bt.pick_windows(tie, 20, [0], [(0, 1)], [8])


def test_what_the_bounded_search_buys(oracle):
    """8 elements in a 0.15 km disc at 40 Hz, a 6 dB plane wave (225 deg, 0.34 km/s) band-passed to 1.0-1.1 Hz (2nd-order
    Butterworth, zero phase), 40 windows of 1200 samples, v_min = 0.25 km/s: the full search leaves picks outside the
    physical range, the bounded search none, and plain OLS on the picks puts strictly more windows within 5 degrees and
    10 % of the truth (DESIGN.md section 14 quotes the counts)."""
    from scipy import signal
    from narrow_band_least_squares_amd import planner, synthetic
    fs, W, N, nwin = 40.0, 1200, 8, 40
    inc = W // 2
    rij = synthetic.array_geometry(N, 0.15)
    data = synthetic.plane_wave(rij, W + (nwin - 1) * inc + 1, fs, 0.1, 10.0, snr_db=6.0)
    filt = signal.sosfiltfilt(signal.butter(2, [1.0, 1.1], btype='bandpass', fs=fs, output='sos'), data, axis=1)
    xij, pairs, _ = planner.co_array(rij)
    lim = bt.limits(xij, fs, 0.25)
    np.testing.assert_array_equal(planner.lag_limits(xij, fs, 0.25), lim)
    assert (lim.min(), int(np.median(lim)), lim.max()) == (5, 15, 39)
    pl, starts = [tuple(p) for p in pairs], [w * inc for w in range(nwin)]
    got = {}
    for name, L in (('full', np.full(len(pl), W - 1)), ('bounded', lim)):
        lag, _ = bt.pick_windows(filt, W, starts, pl, L, exact=True)
        vel, baz = oracle.vel_baz(oracle.ols_solve(xij, np.ascontiguousarray((lag / fs).T))[0])
        dbaz = np.abs((baz - 225.0 + 180.0) % 360.0 - 180.0)
        got[name] = (bt.outside(lag, lim), int(np.count_nonzero((dbaz <= 5.0) & (np.abs(vel - 0.34) <= 0.034))))
    print('picks outside the range (of %d), windows within 5 deg / 10 %% (of %d): %r' % (nwin * len(pl), nwin, got))
    assert got['full'][0] > 0 and got['bounded'][0] == 0
    assert got['bounded'][1] > got['full'][1]
