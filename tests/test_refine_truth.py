"""tests/refine_truth.py — the long-double statement of the sub-sample lag refinement — against
closed forms, and the physical property the refinement exists for: on a noise-free plane wave the residual of the
slowness fit leaves the quantisation floor 1 / (fs sqrt(12)) of whole-sample lags.  CPU only."""
import math

import numpy as np

import refine_truth as rt

W = 64


def _pulse(pos, amp=1.0, n=W):
    x = np.zeros(n)
    x[pos] = amp
    return x


def test_one_unit_pulse_per_channel_gives_zero_exactly():
    for p, q in ((10, 30), (30, 10), (5, 5), (1, 62)):
        a, b = _pulse(p), _pulse(q)
        lag = int(rt.pick_lags(np.stack([a, b]), W, [0], [(0, 1)])[0, 0])
        assert lag == q - p
        r = rt.refine_pair(a, b, lag)
        assert r['frac'] == 0.0 and float(r['Nn']) == 0.0 and float(r['D']) == -2.0


def test_the_sign_is_pinned_by_a_pulse_with_a_shoulder():
    """a: unit pulse at p; b: 1.0 at q and 0.5 at q + 1 -> R(l) = 1 at l = q - p, R(l+1) = 0.5, R(l-1) = 0:
    Nn = -0.5, D = 0 - 2 + 0.5 = -1.5, frac = 1/2 * (-0.5) / (-1.5) = +1/6: b is later than the whole-sample lag says.
    The mirrored table (shoulder at q - 1) gives -1/6."""
    p, q = 20, 33
    a = _pulse(p)
    b = _pulse(q) + _pulse(q + 1, 0.5)
    lag = int(rt.pick_lags(np.stack([a, b]), W, [0], [(0, 1)])[0, 0])
    assert lag == q - p
    r = rt.refine_pair(a, b, lag)
    assert float(r['Nn']) == -0.5 and float(r['D']) == -1.5
    assert r['frac'] == float(np.longdouble(1) / 6)
    b = _pulse(q) + _pulse(q - 1, 0.5)
    r = rt.refine_pair(a, b, q - p)
    assert r['frac'] == float(-np.longdouble(1) / 6)
    # the shoulder on a instead: a later a is a smaller lag
    r = rt.refine_pair(_pulse(p) + _pulse(p + 1, 0.5), _pulse(q), q - p)
    assert r['frac'] == float(-np.longdouble(1) / 6)


def test_ends_of_the_lag_range_dead_channel_and_nan_give_zero():
    a, b = _pulse(0), _pulse(W - 1)
    assert rt.refine_pair(a, b, W - 1)['frac'] == 0.0 and rt.refine_pair(b, a, -(W - 1))['frac'] == 0.0
    assert rt.refine_pair(a, b, W - 1)['D'] is None
    # one short of the end the three values exist: R(W-1) is the single product a[0] b[W-1]
    r = rt.refine_pair(_pulse(0) + _pulse(1, 0.5), _pulse(W - 1), W - 2)
    assert [float(v) for v in rt.corr3(_pulse(0) + _pulse(1, 0.5), _pulse(W - 1), W - 2)] == [0.0, 0.5, 1.0]
    assert r['frac'] == 0.0                                      # D = 0 - 1 + 1 = 0: no strict maximum
    dead = np.zeros(W)
    r = rt.refine_pair(dead, _pulse(9), 0)
    assert r['frac'] == 0.0 and float(r['D']) == 0.0
    plateau = np.ones(W)
    assert rt.refine_pair(plateau, _pulse(9), 3)['frac'] == 0.0   # R = 1, 1, 1: D = 0
    bad = _pulse(20)
    bad[40] = np.nan
    assert rt.refine_pair(bad, _pulse(30), 10)['frac'] == 0.0
    assert rt.refine_pair(_pulse(30), bad, -10)['frac'] == 0.0
    inf = _pulse(20)
    inf[21] = np.inf
    assert rt.refine_pair(inf, _pulse(30) + _pulse(31), 10)['frac'] == 0.0


def test_clamp_and_bound():
    a = _pulse(20)
    b = _pulse(30) + _pulse(29, 0.99)           # R(l-1) = 0.99 at l = 10: Nn = 0.99, D = 0.99 - 2 = -1.01, frac = -0.4901
    r = rt.refine_pair(a, b, 10)
    assert abs(r['frac'] - (-0.5 * 0.99 / 1.01)) < 1e-16 and -0.5 < r['frac'] < 0
    E = 2.0 * W * 2.0 ** -53 * 1.0 * math.sqrt(1 + 0.99 ** 2)
    assert abs(r['E'] - E) <= 1e-15 * E
    assert abs(r['bound'] - ((E + 2 * abs(r['frac']) * E) / (1.01 - 4 * E) + 4 * 2.0 ** -53)) <= 1e-12 * r['bound']
    # a lag that is not the maximum (the contract takes the lag as given): the vertex lies outside, the clamp holds it
    r = rt.refine_pair(_pulse(20), _pulse(30) + _pulse(31, 3.0), 10)      # R = (0, 1, 3): Nn = -3, D = 1 >= 0 -> 0
    assert r['frac'] == 0.0
    # |Nn| > |D|: R = (-5, 0, 1): Nn = -6, D = -4 -> 0.75, clamped to 1/2; the mirror image to -1/2
    assert rt.refine_pair(_pulse(20), _pulse(29, -5.0) + _pulse(31), 10)['frac'] == 0.5
    assert rt.refine_pair(_pulse(20), _pulse(29) + _pulse(31, -5.0), 10)['frac'] == -0.5


def test_refined_lags_leave_the_quantisation_floor(oracle):
    """6 elements x 200 samples per window at fs = 20, 4 windows, noise-free; 40 sinusoids at 0.4 .. 2 Hz at fractional
    delays over radii of 0.05 .. 0.3 km.  With whole-sample lags sigma_tau lies within a factor 2 of 1 / (fs sqrt(12));
    with refined lags every window's sigma_tau is below half that floor."""
    N, Wp, fs, nwin = 6, 200, 20.0, 4
    floor = 1.0 / (fs * math.sqrt(12.0))
    for seed in (11, 12, 13):
        data, rij, _ = rt.sinusoid_wave(N, nwin * Wp + 1, fs, seed)
        xij, pairs = oracle.co_array(rij)
        _, _, starts = oracle.window_plan(data.shape[1], fs, Wp / fs, 0.0)
        assert len(starts) == nwin
        tau, _, _ = oracle.correlate_windows(np.ascontiguousarray(data.T), Wp, starts, pairs, fs)
        lag = np.rint(tau.T * fs).astype(np.int64)
        np.testing.assert_array_equal(lag, rt.pick_lags(data, Wp, starts, pairs))
        sig_int = oracle.ols_solve(xij, tau)[3]
        ref = rt.refine_windows(data, Wp, starts, pairs, lag)
        assert np.any(ref['frac'] != 0) and np.all(np.abs(ref['frac']) <= 0.5)
        tau_ref = np.ascontiguousarray(((lag + ref['frac']) / fs).T)
        sig_ref = oracle.ols_solve(xij, tau_ref)[3]
        print('seed %d: sigma_tau / floor with whole-sample lags %s, with refined lags %s'
              % (seed, np.round(sig_int / floor, 3), np.round(sig_ref / floor, 3)))
        assert np.all(sig_int > floor / 2) and np.all(sig_int < 2 * floor)
        assert np.all(sig_ref < floor / 2)
