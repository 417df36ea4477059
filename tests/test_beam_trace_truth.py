"""The CPU truths of the beam trace (tests/beam_trace_truth.py; ``nbls_set_beam_trace``) against each
other and on designed cases, the synthesis window table, and the demonstration: at low SNR the residual of the beam trace
against the noise-free signal of element 0 is 1 / N of element 0's own."""
import numpy as np
import pytest

import beam_trace_cases as cases
import beam_trace_truth as bt
from narrow_band_least_squares_amd import planner

FS = cases.FS


def _random_row(N, npts, W, inc, seed, zscale=0.5):
    rng = np.random.default_rng(seed)
    rij = rng.uniform(-1.0, 1.0, size=(2, N))
    xij = planner.co_array(rij)[0]
    nwin = 1 + (npts - W) // inc
    filt = rng.standard_normal((N, npts)) * np.exp(rng.uniform(-3, 3, size=(N, 1)))
    z = rng.uniform(-zscale, zscale, size=(nwin + 2, 2))
    mdccm = rng.uniform(0.0, 1.0, size=nwin + 2)
    return filt, z, mdccm, nwin, xij


@pytest.mark.parametrize('N,W,inc,npts', [(3, 16, 8, 301), (8, 200, 20, 1500), (9, 257, 128, 2049), (32, 64, 64, 700)])
def test_restatement_within_the_derived_bound(N, W, inc, npts):
    filt, z, mdccm, nwin, xij = _random_row(N, npts, W, inc, 100 + N)
    for kind, gate, masked in (('hann', None, False), ('boxcar', 0.4, False), ('hann', None, True)):
        g = planner.beam_trace_window(W, kind)
        mask = None
        if masked:
            mask = np.random.default_rng(N).integers(0, 1 << N, size=len(z), dtype=np.uint64).astype(np.uint32) & np.uint32(0x24924925)
        a = bt.restate(filt, z, mdccm, nwin, mask, xij, FS, W, inc, g, gate)
        b, bound, cover = bt.reference(filt, z, mdccm, nwin, mask, xij, FS, W, inc, g, gate)
        err = np.abs(a.astype(np.longdouble) - b).astype(np.float64)
        assert np.all(err <= bound), (kind, float(np.max(err / np.maximum(bound, 1e-300))))
        assert cover.max() == -(-W // inc) or gate is not None
        assert np.all(a[cover == 0] == 0.0)
        worst = float(np.max(err[cover > 0] / bound[cover > 0]))
        print('N=%d W=%d inc=%d %s gate=%s kept=%s: worst |a - b| / bound = %.3f, constant up to %d'
              % (N, W, inc, kind, gate, masked, worst, bt.bound_constant(N, int(cover.max()))))
        assert worst > 1e-4                                  # the bound is a rounding bound, not a tolerance of convenience


def test_bound_constant_counts_the_operations():
    # N - 1 additions, one product and C - 1 additions in acc; one product and C - 1 additions in den; one division
    for N, C in ((3, 1), (8, 2), (32, 10)):
        assert bt.bound_constant(N, C) == (N - 1) + 1 + (C - 1) + 1 + (C - 1) + 1


def test_window_table():
    for W in (1, 2, 16, 257, 2400):
        g = planner.beam_trace_window(W)
        t = np.arange(W)
        np.testing.assert_array_equal(g, np.sin(np.pi * (t + 0.5) / W) ** 2)
        assert g.shape == (W,) and g.dtype == np.float64 and np.all(g > 0) and np.all(g <= 1)
        np.testing.assert_allclose(g, g[::-1], rtol=0, atol=1e-15)
        assert np.array_equal(planner.beam_trace_window(W, 'boxcar'), np.ones(W))
    # at half overlap the sin^2 windows add up to one: the weights of the two windows over a sample are a partition
    g = planner.beam_trace_window(200)
    np.testing.assert_allclose(g[:100] + g[100:], 1.0, rtol=0, atol=1e-15)
    for bad in (0, -3, 2.0, True, '16'):
        with pytest.raises(ValueError):
            planner.beam_trace_window(bad)
    with pytest.raises(ValueError):
        planner.beam_trace_window(16, 'hamming')


def _designed(N=4, W=40, inc=20, nwin=6, npts=None, seed=3):
    """Integer traces x_m = roll(s, D_m) and the slowness that lines them up in every window."""
    npts = npts or W + (nwin - 1) * inc
    data, rij, s, D = cases.exact_trace(N, npts, 1, seed)
    xij = planner.co_array(rij)[0]
    _, slow, _ = cases.exact_geometry(N, 1)
    z = np.tile(-slow, (nwin, 1))                          # (the co-array's row of pair (0, m) is r_0 - r_m)
    for w in range(nwin):
        assert np.array_equal(bt.window_delays(xij, FS, z[w], N), D)
    return data, z, xij, s, D


def _interior(npts, D):
    n = np.arange(npts)
    return (n + D.min() >= 0) & (n + D.max() < npts)


def test_gate_on_off_and_nan_mdccm():
    N, W, inc, nwin = 4, 40, 20, 6
    data, z, xij, s, D = _designed(N, W, inc, nwin)
    npts = data.shape[1]
    g = np.ones(W)
    mdccm = np.array([0.9, 0.2, 0.9, np.nan, np.nan, 0.9])
    off = bt.restate(data, z, mdccm, nwin, None, xij, FS, W, inc, g, None)
    nan_gate = bt.restate(data, z, mdccm, nwin, None, xij, FS, W, inc, g, float('nan'))
    np.testing.assert_array_equal(off, nan_gate)                      # the gate is off iff mdccm_min is NaN
    ok = _interior(npts, D)
    np.testing.assert_array_equal(off[ok], s[ok])
    on = bt.restate(data, z, mdccm, nwin, None, xij, FS, W, inc, g, 0.5)
    used = [0, 2, 5]                                                  # 0.2 and the NaNs fail the gate
    cover = np.zeros(npts, dtype=int)
    for w in used:
        cover[w * inc:w * inc + W] += 1
    assert np.all(on[cover == 0] == 0.0) and np.any(cover == 0)       # samples only rejected windows cover: exactly 0.0
    np.testing.assert_array_equal(on[(cover > 0) & ok], s[(cover > 0) & ok])
    every = bt.restate(data, z, mdccm, nwin, None, xij, FS, W, inc, g, -1.0)      # a gate everyone passes but the NaNs
    assert np.all(every[80:100] == 0.0) and np.all(every[60:80] == s[60:80])      # windows 3 and 4 alone cover [80, 100); window 2 reaches [60, 80)


def test_an_unusable_window_in_the_middle():
    N, W, inc, nwin = 4, 40, 20, 6
    data, z, xij, s, D = _designed(N, W, inc, nwin)
    g = planner.beam_trace_window(W)
    for bad in (np.array([np.nan, 0.1]), np.array([0.1, np.inf]), np.array([1e12, 0.0])):      # not finite; a delay of 2^30 and more
        zz = z.copy()
        zz[2] = bad
        got = bt.restate(data, zz, np.ones(nwin), nwin, None, xij, FS, W, inc, g)
        assert np.all(np.isfinite(got))
        ok = _interior(data.shape[1], D)
        np.testing.assert_allclose(got[ok], s[ok], rtol=0, atol=1e-12)             # its neighbours cover its samples
        skipped = [w for w, _ in bt.usable_windows(zz, np.ones(nwin), nwin, xij, FS, N)]
        assert skipped == [0, 1, 3, 4, 5]
    assert bt.window_delays(xij, FS, np.array([2.0 ** 30 / FS / abs(xij[0][0]), 0.0]), N) is None


def test_an_uncovered_tail_and_windows_beyond_nwin():
    N, W, inc, nwin = 4, 40, 40, 3
    data, z, xij, s, D = _designed(N, W, inc, nwin + 2, npts=nwin * W + 17)
    g = np.ones(W)
    got = bt.restate(data, z, np.ones(len(z)), nwin, None, xij, FS, W, inc, g)
    assert np.all(got[nwin * W:] == 0.0)                                   # no window reaches the tail; w >= nwin is not used
    b, bound, cover = bt.reference(data, z, np.ones(len(z)), nwin, None, xij, FS, W, inc, g)
    assert np.all(cover[nwin * W:] == 0) and np.all(bound[nwin * W:] == 0.0) and np.all(b[nwin * W:] == 0)


def test_element_0_dropped_keeps_the_time_base():
    """The kept set of a window without element 0: the other elements are still read at their delays against element 0's
    position, so the window lands where its neighbours do."""
    N, W, inc, nwin = 5, 40, 20, 6
    data, z, xij, s, D = _designed(N, W, inc, nwin)
    g = planner.beam_trace_window(W)
    mask = np.zeros(nwin, dtype=np.uint32)
    mask[2] = 1                                                       # element 0
    mask[4] = (1 << 1) | (1 << 4)
    mask[5] = 0b11110                                                 # fewer than 3 would remain: the whole array
    assert bt.kept_bits(mask[5], N)[1] == N and bt.kept_bits(mask[2], N)[1] == N - 1
    got = bt.restate(data, z, np.ones(nwin), nwin, mask, xij, FS, W, inc, g)
    ok = _interior(data.shape[1], D)
    np.testing.assert_allclose(got[ok], s[ok], rtol=0, atol=1e-12)     # every element carries s: any kept set gives s back
    noisy = data.copy()
    noisy[0] += 100.0                                                 # ... and the dropped element's samples are not read
    got2 = bt.restate(noisy, z, np.ones(nwin), nwin, np.full(nwin, 1, dtype=np.uint32), xij, FS, W, inc, g)
    np.testing.assert_allclose(got2[ok], s[ok], rtol=0, atol=1e-12)


# ---- the demonstration ----

@pytest.fixture(scope='module')
def demo(oracle):
    d = cases.DEMO
    noisy, clean, rij = cases.demo_traces()
    xij, idx = oracle.co_array(rij)
    _, _, intervals = oracle.window_plan(d['npts'], FS, d['W'] / FS, 1.0 - d['hop'] / d['W'])
    assert len(intervals) == d['nwin']
    tau, mdccm, _ = oracle.correlate_windows(np.ascontiguousarray(noisy.T), d['W'], intervals, idx, FS)
    z, _, _ = oracle.lts_post_process(tau, xij, oracle.fast_lts(tau, xij, 0.5), 0.5)
    _, mdccm_noise, _ = oracle.correlate_windows(np.ascontiguousarray(cases.demo_noise().T), d['W'], intervals, idx, FS)
    return dict(noisy=noisy, clean=clean, rij=rij, xij=xij, z=np.ascontiguousarray(z.T), mdccm=mdccm, mdccm_noise=mdccm_noise)


def test_demonstration_residual_is_one_nth_of_an_elements(demo):
    d = cases.DEMO
    z = demo['z']
    vel = 1.0 / np.hypot(z[:, 0], z[:, 1])
    baz = np.mod(np.degrees(np.arctan2(z[:, 0], z[:, 1])), 360.0)
    solved = int(np.sum((np.abs((baz - d['baz'] + 180.0) % 360.0 - 180.0) <= 5.0) & (np.abs(vel - d['vel']) <= 0.1 * d['vel'])))
    assert solved >= 0.9 * d['nwin'], solved                           # LTS solves the windows: within 5 degrees and 10 %
    g = planner.beam_trace_window(d['W'])
    trace = bt.restate(demo['noisy'], z, np.ones(d['nwin']), d['nwin'], None, demo['xij'], FS, d['W'], d['hop'], g)
    ratio = cases.residual_ratio(trace, demo['noisy'][0], demo['clean'][0])
    snr_band = 10.0 * np.log10(np.mean(demo['clean'][0] ** 2) / np.mean((demo['noisy'][0] - demo['clean'][0]) ** 2))
    print('demonstration: %d of %d windows solved, in-band SNR of an element %.1f dB, residual ratio %.3f (1 / N = %.3f)'
          % (solved, d['nwin'], snr_band, ratio, 1.0 / d['N']))
    assert snr_band < 0.0
    assert ratio <= 2.0 / d['N']


def test_demonstration_gate_separates_wave_from_noise(demo):
    d = cases.DEMO
    print('MdCCM of the demonstration windows %.3f .. %.3f, of noise alone %.3f .. %.3f, gate %.3f'
          % (demo['mdccm'].min(), demo['mdccm'].max(), demo['mdccm_noise'].min(), demo['mdccm_noise'].max(), d['mdccm_min']))
    assert demo['mdccm'].min() > d['mdccm_min'] + 0.005 and demo['mdccm_noise'].max() < d['mdccm_min'] - 0.005
    g = planner.beam_trace_window(d['W'])
    args = (demo['xij'], FS, d['W'], d['hop'], g)
    gated = bt.restate(demo['noisy'], demo['z'], demo['mdccm'], d['nwin'], None, *args, d['mdccm_min'])
    plain = bt.restate(demo['noisy'], demo['z'], demo['mdccm'], d['nwin'], None, *args)
    np.testing.assert_array_equal(gated, plain)                       # every window of the wave passes
    noise = bt.restate(cases.demo_noise(), demo['z'], demo['mdccm_noise'], d['nwin'], None, *args, d['mdccm_min'])
    assert not noise.any()                                            # ... and none of the noise
