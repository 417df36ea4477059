"""tests/seeded_truth.py (the NumPy statement of the seeded lag search) against brute-force loops, the
rules for empty, dead and non-finite windows, and the experiment that shows what the seeded search buys.  CPU only."""
import numpy as np
import pytest

import bounded_truth as bdt
import grid_truth as gt
import seeded_truth as sdt


def _centres(W):
    return [-(W + 3), -(W - 1), -1, 0, 1, W - 1, W + 3]


def _halfwidths(W):
    return [0, 1, 3, W - 1, 2 * W]


@pytest.mark.parametrize('W', [2, 3, 16, 65])
def test_pick_equals_the_brute_force_loops(W):
    rng = np.random.default_rng(70 + W)
    for c in _centres(W):
        for K in _halfwidths(W):
            a, b = rng.standard_normal(W), rng.standard_normal(W)
            lag, cmax, gap = sdt.pick(a, b, c, K)
            blag, bcmax = sdt.pick_brute(a, b, c, K)
            lo, hi = sdt.search_range(W, c, K)
            assert -(W - 1) <= lo <= hi <= W - 1 and lo <= min(max(c, -(W - 1)), W - 1) <= hi
            assert lag == blag and abs(cmax - bcmax) <= 1e-14
            assert lo <= lag <= hi and gap > 0
            full = np.correlate(a, b, 'full') / np.sqrt(np.sum(a * a) * np.sum(b * b))
            assert cmax == full[W - 1 - lag] and cmax == full[W - 1 - hi:W - lo].max()


@pytest.mark.parametrize('W', [2, 3, 16, 65])
def test_a_half_width_of_twice_the_window_is_the_full_search(W):
    rng = np.random.default_rng(80 + W)
    for c in _centres(W):
        for K in (2 * (W - 1), 2 * W, 2 ** 31 - 1):
            a, b = rng.standard_normal(W), rng.standard_normal(W)
            assert sdt.search_range(W, c, K) == (-(W - 1), W - 1)
            assert sdt.pick(a, b, c, K)[0] == W - 1 - int(np.argmax(np.correlate(a, b, 'full')))
            assert sdt.pick(a, b, c, K)[:2] == bdt.pick(a, b, W - 1)[:2]


def test_ties_take_the_largest_lag_and_empty_ranges_hi():
    W = 32
    a, b = np.zeros(W), np.zeros(W)
    a[10] = 1.0
    b[10 + 3] = b[10 - 5] = 1.0                              # R(3) = R(-5) = 1
    assert sdt.pick(a, b, -1, 4)[:2] == (3, 1.0 / np.sqrt(2.0))          # [-5, 3]: both inside, the largest lag
    assert sdt.pick(a, b, -3, 2)[:2] == (-5, 1.0 / np.sqrt(2.0))         # [-5, -1]
    assert sdt.pick(a, b, 0, 2)[:2] == (2, 0.0)                          # nothing inside: hi, cmax 0
    assert sdt.pick(a, b, 40, 3)[:2] == (31, 0.0)                        # clamped centre: [28, 31]
    assert sdt.pick(a, b, -40, 0)[:2] == (-31, 0.0)
    assert sdt.pick_brute(a, b, -1, 4)[0] == 3 and sdt.pick_brute(a, b, 0, 2) == (2, 0.0)
    lag, cmax, _ = sdt.pick(a, np.zeros(W), 2, 6)            # dead channel
    assert lag == 8 and np.isnan(cmax)
    assert sdt.pick_brute(a, np.zeros(W), 2, 6)[0] == 8 and np.isnan(sdt.pick_brute(a, np.zeros(W), 2, 6)[1])
    lag, cmax, _ = sdt.pick(np.zeros(W), np.zeros(W), 0, 5)  # an all-zero window of both
    assert lag == 5 and np.isnan(cmax)


@pytest.mark.parametrize('W', [2, 3, 16, 65])
@pytest.mark.parametrize('case', ['nan', 'inf', 'minus_inf', 'minus_inf_and_inf'])
def test_non_finite_windows_give_hi_and_nan(W, case):
    """lag = hi, cmax = NaN.  For NaN samples that is what np.argmax of the slice answers."""
    rng = np.random.default_rng(90 + W)
    for c in _centres(W):
        for K in _halfwidths(W):
            a, b = rng.standard_normal(W), rng.standard_normal(W)
            x = a if (c + K) % 2 else b
            x[rng.integers(W)] = {'nan': np.nan, 'inf': np.inf}.get(case, -np.inf)
            if case == 'minus_inf_and_inf':
                (b if x is a else a)[rng.integers(W)] = np.inf
            lo, hi = sdt.search_range(W, c, K)
            lag, cmax, gap = sdt.pick(a, b, c, K)
            assert lag == hi and np.isnan(cmax) and np.isnan(gap)
            assert sdt.pick_brute(a, b, c, K)[0] == hi and np.isnan(sdt.pick_brute(a, b, c, K)[1])
            if case == 'nan':
                with np.errstate(invalid='ignore'):
                    cij = np.correlate(a, b, 'full') / np.sqrt(np.sum(a * a) * np.sum(b * b))
                assert hi - int(np.argmax(cij[W - 1 - hi:W - lo])) == hi


def test_centres_and_pick_windows():
    d = np.array([[0, 3, -2], [0, -100, 7]])
    pairs = bdt.pair_table(3)
    np.testing.assert_array_equal(sdt.centres(d, [0, 1, -1], pairs), [[3, -2, -5], [-100, 7, 107], [0, 0, 0]])
    data = np.random.default_rng(3).standard_normal((3, 100))
    c = sdt.centres(d, [0, 1, -1], pairs)
    lag, cmax = sdt.pick_windows(data, 16, [0, 8, 16], pairs, c, 2)
    assert lag.shape == cmax.shape == (3, 3)
    assert np.all(np.abs(lag[0] - c[0]) <= 2) and lag[1, 0] in (-15, -14, -13) and lag[1, 2] in (13, 14, 15)
    with pytest.raises(AssertionError):                       # an exact tie is refused unless the case says it is one
        tie = np.zeros((2, 20))
        tie[0, 10] = tie[1, 13] = tie[1, 5] = 1.0
        sdt.pick_windows(tie, 20, [0], [(0, 1)], [[0]], 8)


def _setup(radius, snr_db):
    from scipy import signal
    from narrow_band_least_squares_amd import planner, synthetic
    fs, W, N, nwin = 40.0, 1200, 8, 40
    inc = W // 2
    rij = synthetic.array_geometry(N, radius)
    data = synthetic.plane_wave(rij, W + (nwin - 1) * inc + 1, fs, 0.1, 10.0, snr_db=snr_db)
    filt = signal.sosfiltfilt(signal.butter(2, [1.0, 1.1], btype='bandpass', fs=fs, output='sos'), data, axis=1)
    xij, pairs, _ = planner.co_array(rij)
    return fs, W, N, nwin, filt, xij, [tuple(p) for p in pairs], [w * inc for w in range(nwin)]


def _counts(oracle, radius, snr_db, halfwidths):
    """Windows (of 40) whose OLS estimate lies within 5 degrees and 10 % of the truth (225 deg, 0.34 km/s), for the full
    search, the bounded search (v_min = 0.25 km/s), the grid maximum and the seeded search at every K of ``halfwidths``."""
    from narrow_band_least_squares_amd import planner
    from narrow_band_least_squares_amd.lts_array import grid_slowness
    fs, W, N, nwin, filt, xij, pl, starts = _setup(radius, snr_db)

    def hits(vel, baz):
        dbaz = np.abs((baz - 225.0 + 180.0) % 360.0 - 180.0)
        return int(np.count_nonzero((dbaz <= 5.0) & (np.abs(vel - 0.34) <= 0.034)))

    def ols(lag):
        return hits(*oracle.vel_baz(oracle.ols_solve(xij, np.ascontiguousarray((lag / fs).T))[0]))
    got = {}
    for name, L in (('full', np.full(len(pl), W - 1)), ('bounded', bdt.limits(xij, fs, 0.25))):
        got[name] = ols(bdt.pick_windows(filt, W, starts, pl, L, exact=True)[0])
    grid = planner.slowness_grid(4.0, 41)
    d, _ = gt.delay_table(xij, grid, fs, N)
    gidx = np.argmax(gt.grid_fstat_fast(filt, W, starts, d), axis=1)
    got['grid'] = hits(*grid_slowness(grid, gidx))
    c = sdt.centres(d, gidx, pl)
    for K in halfwidths:
        got['seeded K=%d' % K] = ols(sdt.pick_windows(filt, W, starts, pl, c, K, exact=True)[0])
    return got


def test_what_the_seeded_search_buys(oracle):
    """DESIGN.md section 15's setup — 8 elements at 40 Hz, a plane wave (225 deg, 0.34 km/s) band-passed to 1.0-1.1 Hz, 40
    windows of 1200 samples, the 1257-point grid of +-4 s/km — with the lag of every pair searched within K samples of the
    delay the grid maximum predicts (K = 18: half a period of 1.1 Hz, ``planner.seed_halfwidths``).  In a 1 km disc at -6 dB
    plain OLS on the seeded picks puts more windows within 5 degrees and 10 % of the truth than on the full-search picks
    and than on the bounded picks; in a 0.15 km disc at 6 dB more than on the bounded picks (DESIGN.md section 16 quotes
    the counts)."""
    from narrow_band_least_squares_amd import planner
    assert planner.seed_halfwidths([1.1], 40.0).tolist() == [18]
    big = _counts(oracle, 1.0, -6.0, (4, 9, 18))
    print('1.0 km, -6 dB: windows within 5 deg / 10 %% of the truth (of 40): %r' % (big,))
    small = _counts(oracle, 0.15, 6.0, (4, 9, 18))
    print('0.15 km, 6 dB: windows within 5 deg / 10 %% of the truth (of 40): %r' % (small,))
    low = _counts(oracle, 0.15, -6.0, (4, 9, 18))                    # (nothing helps there, and nothing is claimed)
    print('0.15 km, -6 dB: windows within 5 deg / 10 %% of the truth (of 40): %r' % (low,))
    assert big['seeded K=18'] > big['full'] and big['seeded K=18'] > big['bounded']
    assert small['seeded K=18'] > small['bounded']
