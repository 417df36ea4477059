"""The CPU truth of the fractional-sample steering (tests/steer_truth.py) against itself: the float64
restatement lies within the long-double bounds, the coefficient identities, ``planner.steering_error`` against the table of
the design, and the small-aperture demonstration.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import beam_truth as bt          # noqa: E402
import grid_truth as gt          # noqa: E402
import steer_truth as stt        # noqa: E402

from narrow_band_least_squares_amd import planner   # noqa: E402


@pytest.mark.parametrize('taps', stt.TAPS)
def test_float64_restatement_lies_within_the_long_double_bounds(taps):
    """(a) within (b) on random data for N = 3 .. 32: windows at both ends of the trace read taps outside it."""
    rng = np.random.default_rng(220 + taps)
    cells = 0
    for N in range(3, 33):
        npts, W = 300, int(rng.integers(16, 120))
        filt = rng.standard_normal((N, npts))
        tau = np.concatenate(([0.0], rng.uniform(-9.0, 9.0, N - 1)))
        n, mu = stt.split(tau)
        c = stt.coefficients(taps, mu)
        for s0 in (0, int(rng.integers(1, npts - W)), npts - W):
            ref = stt.cell(filt, s0, W, n, mu, taps)
            P, F = stt.outputs64(stt.rows64(filt, s0, W, n, c))
            assert ref['tol_power'] > 0 and abs(P - ref['power']) <= ref['tol_power'], (N, s0, P, ref['power'], ref['tol_power'])
            assert np.isfinite(ref['tol_fstat']) and not ref['power_only'], (N, s0)
            assert abs(F - ref['fstat']) <= ref['tol_fstat'], (N, s0, F, ref['fstat'], ref['tol_fstat'])
            # the bound is a rounding bound, not a loose one: far below the value
            assert ref['tol_power'] < 1e-9 * ref['power'] and ref['tol_fstat'] < 1e-6 * max(ref['fstat'], 1.0)
            cells += 1
    assert cells == 90


@pytest.mark.parametrize('taps', stt.TAPS)
def test_coefficient_identities(taps):
    K = taps // 2
    mu = np.concatenate(([0.0, 0.5, 1.0 - 2.0 ** -53, 2.0 ** -60], np.random.default_rng(1).uniform(0, 1, 500)))
    c = stt.coefficients(taps, mu)
    assert np.all(np.abs(c.sum(axis=1) - 1.0) <= 8 * 2.0 ** -52)                  # a partition of unity within a few ulp
    exact = stt.coefficients(taps, mu, stt.LD)
    assert np.all(np.abs(c - exact) <= 2 * taps * 2.0 ** -53 * np.abs(exact))     # the bound steer_truth charges for c
    unit = stt.coefficients(taps, 0.0)
    assert unit[K - 1] == 1.0 and np.all(np.delete(unit, K - 1) == 0.0)           # mu = 0: the unit tap, every other +-0
    # the planner's helper is the same sequence of operations, and the denominators are those of the header
    assert np.array_equal(planner.steering_coefficients(taps, mu), c)
    assert max(abs(D) for D in stt.denominators(taps)) == {4: 6, 6: 120, 8: 5040}[taps]
    # the polynomial property: samples of a polynomial of degree < taps are interpolated exactly (up to rounding)
    k = np.arange(-K + 1, K + 1, dtype=np.float64)
    for deg in range(taps):
        assert np.allclose(c @ k ** deg, mu ** deg, rtol=0, atol=1e-9)


@pytest.mark.parametrize('taps', stt.TAPS)
def test_integer_delays_reproduce_the_whole_sample_truth_bit_for_bit(taps):
    rng = np.random.default_rng(7)
    N, npts, W = 6, 200, 64
    filt = rng.standard_normal((N, npts))
    filt[2, 50] = -0.0
    d = np.array([0, 3, -4, 7, 0, -9])
    n, mu = stt.split(d.astype(np.float64))
    assert np.array_equal(n, d) and np.all(mu == 0.0)
    c = stt.coefficients(taps, mu)
    for s0 in (0, 70, npts - W):
        x = stt.rows64(filt, s0, W, n, c)
        whole = np.zeros((N, W))
        for i in range(N):
            idx = s0 + np.arange(W) + d[i]
            ok = (idx >= 0) & (idx < npts)
            whole[i, ok] = filt[i, idx[ok]]
        assert np.array_equal(x, whole)
        assert stt.outputs64(x) == stt.outputs64(whole)
        # ... and the long-double truth is beam_truth's
        S_b, S_t = bt.window_sums(filt, s0, W, d)
        ref = stt.cell(filt, s0, W, n, mu, taps)
        assert ref['S_b'] == S_b and ref['S_t'] == S_t
    # a NaN sample under a zero coefficient still propagates
    filt[1, 100] = np.nan
    x = stt.rows64(filt, 90, 16, n, c)
    K = taps // 2
    hit = [t for t in range(16) if 90 + t + 3 - K + 1 <= 100 <= 90 + t + 3 + K]
    assert np.array_equal(np.flatnonzero(np.isnan(x[1])), hit)


def test_grid_tables_floor_and_halo():
    xij = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 1.0]])
    grid = np.array([[0.05, 0.1], [-0.025, 0.0], [-1e-9 / 20.0, 0.0], [0.0, 0.0]])
    n, c, tau, halo = stt.grid_tables(xij, grid, 20.0, 3, 4)
    assert np.array_equal(n, [[0, 1, 2], [0, -1, 0], [0, -1, 0], [0, 0, 0]])
    assert tau[1, 1] == -0.5 and c[1, 1].tolist() == stt.coefficients(4, 0.5).tolist()
    assert 0.999 < tau[2, 1] - n[2, 1] < 1.0
    assert halo == 4                                            # max(|n - K + 1|, |n + K|) = 2 + 2
    assert np.all(c[3] == stt.coefficients(4, 0.0))


def test_steering_error_reproduces_the_table():
    table = {4: ('2.3e-04', '3.5e-03', '5.1e-02', '2.2e-01'),
             6: ('4.6e-06', '2.8e-04', '1.5e-02', '1.3e-01'),
             8: ('9.9e-08', '2.4e-05', '4.6e-03', '7.4e-02')}
    for taps, row in table.items():
        assert tuple('%.1e' % planner.steering_error(taps, f) for f in (0.05, 0.1, 0.2, 0.3)) == row
    for bad in (0, 5, 10, 8.0, True, None):
        with pytest.raises(ValueError):
            planner.steering_error(bad, 0.1)


def demonstration_statements(grid, true, F0, F8, rows):
    """The three statements of the demonstration on the maps of the whole-sample (F0) and the 8-tap (F8) search -> the
    figures (ties per window, median errors)."""
    ties0 = [int((f == np.nanmax(f)).sum()) for f in F0]
    ties8 = [int((f == np.nanmax(f)).sum()) for f in F8]
    assert min(ties0) >= 2 and rows < len(grid), (ties0, rows)
    assert ties8 == [1] * len(F8), ties8
    err0 = np.median([np.hypot(*(grid[int(np.nanargmax(f))] - true)) for f in F0])
    err8 = np.median([np.hypot(*(grid[int(np.nanargmax(f))] - true)) for f in F8])
    assert err8 < 0.5 * err0 and err8 <= 0.2 * np.sqrt(2.0), (err0, err8)
    return ties0, ties8, err0, err8


def test_demonstration_on_the_small_aperture_array():
    """100 m of aperture at 20 Hz: 213 distinct delay rows under 1681 grid points, every whole-sample maximum a plateau of
    18 - 38 points (median slowness error 1.17 s/km of 2.94); with 8 taps the maximum is unique in all eight windows and the
    median error 0.17 s/km, less than a grid step."""
    d = stt.demonstration()
    N = d['filt'].shape[0]
    whole, tau = gt.delay_table(d['xij'], d['grid'], d['fs'], N)
    assert 4.0 < np.abs(tau).max() < 5.0
    rows = len({tuple(r) for r in whole})
    F0 = stt.grid_fstat64(d['filt'], d['W'], d['starts'], whole, None)
    n, c, _, _ = stt.grid_tables(d['xij'], d['grid'], d['fs'], N, 8)
    F8 = stt.grid_fstat64(d['filt'], d['W'], d['starts'], n, c)
    demonstration_statements(d['grid'], d['true'], F0, F8, rows)
    assert np.median(F8.max(axis=1)) > np.median(F0.max(axis=1))
