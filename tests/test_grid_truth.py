"""The CPU reference of the slowness-grid search (tests/grid_truth.py) against cases worked by hand,
and the count that says what the search buys at low SNR."""
import numpy as np

import bounded_truth as bdt
import grid_truth as gt


def test_delay_table_by_hand():
    """Three elements, fs = 20, xij rows of the pairs (0, 1), (0, 2) = (-1.3, 0.2), (0.45, 0.9).  s = (0.5, -0.25):
    tau = 20 (-0.65 - 0.05) = -14 and 20 (0.225 - 0.225) = 0.  s = 0: no delay.  Ties go to even: xij (0.125, 0), (0.175, 0)
    at s = (1, 0) give 2.5 -> 2 and 3.5 -> 4."""
    xij = np.array([[-1.3, 0.2], [0.45, 0.9], [1.75, 0.7]])
    d, tau = gt.delay_table(xij, [[0.5, -0.25], [0.0, 0.0], [-0.5, 0.25]], 20.0, 3)
    assert d.tolist() == [[0, -14, 0], [0, 0, 0], [0, 14, 0]] and not gt.near_tie(tau)
    d, tau = gt.delay_table(np.array([[0.125, 0.0], [0.175, 0.0], [0.05, 0.0]]), [[1.0, 0.0]], 20.0, 3)
    assert d.tolist() == [[0, 2, 4]] and gt.near_tie(tau)


def _shifted(N, npts, D, seed=5):
    """Identical channels at whole-sample delays: x_i[n] = s[n - D_i] (integers: every sum is exact)."""
    s = np.random.default_rng(seed).integers(-1000, 1000, npts).astype(np.float64)
    return np.stack([np.roll(s, int(k)) for k in D])


def test_identical_channels_put_the_maximum_on_their_own_delays():
    fs, W, inc = 20.0, 64, 32
    rij = np.array([[0.0, 0.30, -0.20, 0.10], [0.0, 0.10, 0.40, -0.35]])
    xij = np.array([rij[:, 0] - rij[:, j] for j in range(1, 4)])        # pairs (0, i): r_0 - r_i
    grid = np.array([[0.0, 0.0], [-2.0, -1.0], [2.0, 1.0], [1.0, 2.0], [2.0, 1.0]])
    d, tau = gt.delay_table(xij, grid, fs, 4)
    assert d[2].tolist() == [0, -14, 0, 3] and not gt.near_tie(tau)
    data = _shifted(4, 600, d[2])
    ref = gt.grid_reference(data, fs, xij, grid, W, inc, 8, first=2)     # interior windows
    assert np.all(ref['index'] == 2)                                     # ... and of the duplicate 2 / 4 the lower index wins
    assert np.all(ref['fstat'] == np.inf) and np.all(ref['F'][:, 4] == np.inf)
    assert np.all(ref['F'][:, [0, 1, 3]] < 10.0)
    for k in range(8):
        s0 = (2 + k) * inc
        assert ref['power'][k] == np.mean(data[0, s0:s0 + W] ** 2)


def test_all_zero_window_and_nan_sample():
    fs, W = 20.0, 50
    xij = np.array([[0.1, 0.0], [0.0, 0.1], [-0.1, 0.1]])
    grid = np.array([[0.0, 0.0], [2.0, 0.0], [0.0, 2.0]])
    d, _ = gt.delay_table(xij, grid, fs, 3)
    assert d.tolist() == [[0, 0, 0], [0, 4, 0], [0, 0, 4]]
    x = np.random.default_rng(6).standard_normal((3, 200))
    x[:, 100:] = 0.0
    ref = gt.grid_reference(x, fs, xij, grid, W, 100, 2)
    assert ref['index'][0] >= 0 and np.isfinite(ref['fstat'][0])
    assert ref['index'][1] == -1 and np.isnan(ref['fstat'][1]) and np.isnan(ref['power'][1]) and np.all(np.isnan(ref['F'][1]))
    # a NaN at sample 52 of element 1: window [0, 50) reads it only where element 1 is read 4 samples later
    x[1, 52] = np.nan
    ref = gt.grid_reference(x, fs, xij, grid, W, 100, 1)
    assert np.isnan(ref['F'][0]).tolist() == [False, True, False]
    assert ref['index'][0] in (0, 2)


def test_fast_form_agrees_with_the_reference():
    fs, W, inc, N = 20.0, 65, 32, 4
    rij = np.array([[0.0, 0.30, -0.20, 0.10], [0.0, 0.10, 0.40, -0.35]])
    xij = np.array([rij[:, 0] - rij[:, j] for j in range(1, 4)])
    grid = np.array([[a, b] for a in (-1.0, 0.0, 1.0) for b in (-1.0, 0.0, 1.0)])
    x = np.random.default_rng(7).standard_normal((N, 400))
    ref = gt.grid_reference(x, fs, xij, grid, W, inc, 10)
    F = gt.grid_fstat_fast(x, W, [w * inc for w in range(10)], ref['d'])
    assert np.all(np.abs(F - ref['F']) <= ref['tol_fstat'])


def test_what_the_grid_search_buys(oracle):
    """8 elements in a 1 km disc at 40 Hz, a plane wave (225 deg, 0.34 km/s) at -6 dB band-passed to 1.0-1.1 Hz (2nd-order
    Butterworth, zero phase), 40 windows of 1200 samples: OLS on the full-search picks and on the bounded picks
    (v_min = 0.25 km/s) put no window within 5 degrees and 10 % of the truth, the maximum of F over the 41 x 41 grid of
    +-4 s/km (1257 points) puts most of them there (DESIGN.md section 15 quotes the counts)."""
    from scipy import signal
    from narrow_band_least_squares_amd import planner, synthetic
    from narrow_band_least_squares_amd.lts_array import grid_slowness
    fs, W, N, nwin = 40.0, 1200, 8, 40
    inc = W // 2
    rij = synthetic.array_geometry(N, 1.0)
    data = synthetic.plane_wave(rij, W + (nwin - 1) * inc + 1, fs, 0.1, 10.0, snr_db=-6.0)
    filt = signal.sosfiltfilt(signal.butter(2, [1.0, 1.1], btype='bandpass', fs=fs, output='sos'), data, axis=1)
    xij, pairs, _ = planner.co_array(rij)
    lim = bdt.limits(xij, fs, 0.25)
    pl, starts = [tuple(p) for p in pairs], [w * inc for w in range(nwin)]

    def hits(vel, baz):
        dbaz = np.abs((baz - 225.0 + 180.0) % 360.0 - 180.0)
        return int(np.count_nonzero((dbaz <= 5.0) & (np.abs(vel - 0.34) <= 0.034)))
    got = {}
    for name, L in (('full', np.full(len(pl), W - 1)), ('bounded', lim)):
        lag, _ = bdt.pick_windows(filt, W, starts, pl, L, exact=True)
        got[name] = hits(*oracle.vel_baz(oracle.ols_solve(xij, np.ascontiguousarray((lag / fs).T))[0]))
    grid = planner.slowness_grid(4.0, 41)
    assert grid.shape == (1257, 2)
    d, _ = gt.delay_table(xij, grid, fs, N)
    assert int(np.abs(d).max()) == 128
    F = gt.grid_fstat_fast(filt, W, starts, d)
    got['grid'] = hits(*grid_slowness(grid, np.argmax(F, axis=1)))
    print('windows within 5 deg / 10 %% of the truth (of %d): %r' % (nwin, got))
    assert got['grid'] > got['full'] and got['grid'] > got['bounded']
