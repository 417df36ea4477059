"""The element-delay truth of tests/element_delay_truth.py (``nbls_set_element_delays``) on the CPU: the
float64 restatement inside the long-double bounds, constructed cases whose answer is known, the planner's shift ranges, and
the demonstration that motivates the feature."""
import numpy as np
import pytest

import element_delay_cases as cases
import element_delay_truth as edt
from narrow_band_least_squares_amd import planner, synthetic

FS = cases.FS


def _judge(filt, xij, z, W, inc, nwin, K, dropped=None, first=0):
    """(a) through ``check_units`` against (b) -> (values, near-ties, worst fraction of a bound)."""
    refs = edt.row_reference(filt, FS, xij, z, W, inc, nwin, K, dropped, first)
    return edt.check_units(refs, *edt.row64(filt, FS, xij, z, W, inc, nwin, K, dropped, first))


@pytest.mark.parametrize('N', list(range(3, 33)))
def test_float64_within_the_bounds(N):
    W, K, nwin = 50, 3, 4
    data, rij = cases.trace(N, W, 'wave')
    xij = planner.co_array(rij)[0]
    n, ties, worst = _judge(data, xij, cases.cpu_slowness('wave', nwin, N), W, W // 2, nwin, K)
    assert n == nwin * N and ties == 0 and worst < 1.0


@pytest.mark.parametrize('kind', ['noise', 'wave'])
@pytest.mark.parametrize('shape', cases.SHAPES + cases.BOUNDARY, ids=lambda s: 'N%d-W%d-K%d' % s)
def test_no_input_of_the_gpu_tests_needs_the_near_tie_licence(shape, kind):
    """Every input set of tests/test_gpu_element_delay.py: (a) against (b) is judged without one accepted near-tie.  (The
    slowness is not a solved one here; three windows per set: the first, a middle and the last.)"""
    N, W, K = shape
    data, rij = cases.trace(N, W, kind)
    xij = planner.co_array(rij)[0]
    nwin = planner.window_plan(data.shape[1], FS, (W + 0.5) / FS, 0.0)[2]
    z = cases.cpu_slowness(kind, nwin)
    for w in (0, nwin // 2, nwin - 1):
        n, ties, worst = _judge(data, xij, z, W, W, 1, K, first=w)
        assert ties == 0 and worst < 1.0


def _smooth(npts, seed=3):
    x = np.random.default_rng(seed).standard_normal(npts + 8)
    return np.convolve(x, np.hanning(9) / np.hanning(9).sum(), mode='valid')


@pytest.mark.parametrize('K', [1, 4])
def test_exact_shifts_are_found(K):
    """Every element the same smoothed noise, element m displaced by an exact s samples, z = 0: shift[m] == s, cc is 1 within
    its bound for the others... and for m itself, and frac == 0 at |s| == K."""
    N, W, npts = 5, 96, 400
    base = _smooth(npts + 2 * K)
    xij = planner.co_array(synthetic.array_geometry(N, 1.0))[0]
    for m in (0, 2, N - 1):
        for s in sorted({-K, -1, 0, 1, K}):
            filt = np.stack([base[K:K + npts]] * N)
            filt[m] = base[K - s:K - s + npts]                    # element m records the waveform s samples late
            ref = edt.unit(filt, FS, xij, (0.0, 0.0), 100, W, K)
            delay, cc, shift, _ = edt.unit64(filt, FS, xij, (0.0, 0.0), 100, W, K)
            assert shift[m] == s and ref['shift'][m] == s
            assert abs(cc[m] - 1.0) <= float(ref['e_c'][m][s + K]) + 2.0 ** -52
            if abs(s) == K:
                assert delay[m] == s / FS                          # no fraction at the edge of the range
            else:
                assert abs(delay[m] - s / FS) <= 0.5 / FS
            for o in range(N):
                edt.check_element(ref, o, delay[o], cc[o], shift[o])


def test_zero_range_zero_channel_and_nan():
    N, W, npts, K = 4, 64, 300, 3
    rng = np.random.default_rng(11)
    filt = rng.standard_normal((N, npts))
    xij = planner.co_array(synthetic.array_geometry(N, 1.0))[0]
    z = (0.01, -0.02)
    # K = 0: one candidate, no fraction
    delay, cc, shift, c = edt.unit64(filt, FS, xij, z, 50, W, 0)
    tau, d = edt.taus(xij, z, FS, N)
    assert not shift.any() and c.shape == (N, 1) and np.array_equal(delay, (d.astype(np.float64) - tau) / FS)
    # a zero channel: its own results NaN, shift 0; the others finite
    dead = filt.copy()
    dead[2] = 0.0
    delay, cc, shift, _ = edt.unit64(dead, FS, xij, z, 50, W, K)
    assert np.isnan(delay[2]) and np.isnan(cc[2]) and shift[2] == 0
    assert np.isfinite(np.delete(delay, 2)).all() and np.isfinite(np.delete(cc, 2)).all()
    ref = edt.unit(dead, FS, xij, z, 50, W, K)
    assert ref['shift'][2] is None
    edt.check_units([ref], [delay], [cc], [shift])
    # a NaN sample in element 1's halo, outside its window: only the shifts that read it drop out
    s0 = 100
    tau, d = edt.taus(xij, z, FS, N)
    poisoned = filt.copy()
    poisoned[1, s0 + d[1] + W + 1] = np.nan                        # read by k = 2 and k = 3 alone
    delay, cc, shift, c = edt.unit64(poisoned, FS, xij, z, s0, W, K)
    assert np.isnan(c[1, K + 2:]).all() and np.isfinite(c[1, :K + 2]).all() and np.isfinite(delay).all() and shift[1] <= 1
    assert np.isfinite(np.delete(c, 1, axis=0)).all()
    edt.check_units([edt.unit(poisoned, FS, xij, z, s0, W, K)], [delay], [cc], [shift])
    # ... inside the window: that element and everybody's beam
    poisoned[1, s0 + d[1] + 5] = np.nan
    delay, cc, shift, _ = edt.unit64(poisoned, FS, xij, z, s0, W, K)
    assert np.isnan(delay).all() and np.isnan(cc).all() and not shift.any()
    # NaN z, a delay of 2^30: a bad unit
    for bad in ((np.nan, 0.0), (0.0, np.inf), (2.0 ** 30 / FS / np.abs(xij[:N - 1, 0]).max() * 1.01, 0.0)):
        delay, cc, shift, _ = edt.unit64(filt, FS, xij, bad, 50, W, K)
        assert np.isnan(delay).all() and np.isnan(cc).all() and not shift.any()
        assert edt.unit(filt, FS, xij, bad, 50, W, K)['bad']


def test_windows_that_read_off_both_ends():
    N, W, K = 4, 40, 6
    filt = np.random.default_rng(12).standard_normal((N, 3 * W))
    xij = planner.co_array(synthetic.array_geometry(N, 1.0))[0]
    z = np.array([[0.3, -0.2], [0.0, 0.0], [-0.3, 0.25]])         # delays of several samples either way
    n, ties, worst = _judge(filt, xij, z, W, W, 3, K)
    assert n == 3 * N and ties == 0
    d = edt.taus(xij, z[0], FS, N)[1]
    assert (d - K).min() < 0 and (edt.taus(xij, z[2], FS, N)[1] + K).max() > 0


def test_kept_sets():
    N, W, K = 6, 64, 3
    filt = np.random.default_rng(13).standard_normal((N, 300)) + _smooth(300)[None, :]
    xij = planner.co_array(synthetic.array_geometry(N, 0.1))[0]
    z = (0.01, 0.02)
    assert list(edt.kept_bits(0, N)) == [True] * N
    assert list(edt.kept_bits(0b001001, N)) == [False, True, True, False, True, True]
    assert list(edt.kept_bits(0b011011, N)) == [True] * N          # two would remain: the whole array
    for m in (0, 3, N - 1):
        keep = edt.kept_bits(1 << m, N)
        ref = edt.unit(filt, FS, xij, z, 40, W, K, keep)
        delay, cc, shift, _ = edt.unit64(filt, FS, xij, z, 40, W, K, keep)
        edt.check_units([ref], [delay], [cc], [shift])
        # the dropped element is measured against the beam of the others: its row is that of the full set, because
        # b - y_m over everybody is the sum of the others too — up to the order of the additions
        full = edt.unit64(filt, FS, xij, z, 40, W, K)
        assert shift[m] == full[2][m] and abs(cc[m] - full[1][m]) < 1e-12
        # ... and the others lose its share of their beam
        assert any(cc[o] != full[1][o] for o in range(N) if o != m)


def test_element_shifts_follow_the_formula():
    f = [0.55, 1.1, 0.01, 40.0]
    got = planner.element_shifts(f, 20.0)
    assert got.dtype == np.int32 and list(got) == [18, 9, 256, 1]
    assert list(planner.element_shifts(f, 20.0, 0.25)) == [9, 4, 256, 1]
    np.testing.assert_array_equal(got, np.minimum(planner.seed_halfwidths(f, 20.0), 256))
    assert list(planner.check_element_shifts(4, 3)) == [4, 4, 4] and planner.check_element_shifts([0, 256], 2).dtype == np.int32
    for bad in (-1, 257, 2.0, True, None, [1, 2, 3], 'x', [[1, 2]]):
        with pytest.raises(ValueError):
            planner.check_element_shifts(bad, 2)


# ---- the demonstration: the case of section 20.4 ----

W, HOP, NWIN, BAD, LATE = 2400, 1200, 20, 7, 0.25
NPTS = W + (NWIN - 1) * HOP + 1


def _band(data):
    from scipy import signal
    return signal.sosfiltfilt(signal.butter(2, [0.45, 0.55], 'bandpass', fs=FS, output='sos'), data, axis=1)


def _lts(oracle, data, rij):
    """The oracle's full-lag picks and FAST-LTS (alpha 0.5) of the 20 windows -> (z (nwin, 2), dropped masks (nwin,))."""
    import kept_truth as kt
    xij, idx = oracle.co_array(rij)
    _, _, intervals = oracle.window_plan(data.shape[1], FS, W / FS, 1.0 - HOP / W)
    assert len(intervals) == NWIN
    tau, _, _ = oracle.correlate_windows(np.ascontiguousarray(data.T), W, intervals, idx, FS)
    z, weights, _ = oracle.lts_post_process(tau, xij, oracle.fast_lts(tau, xij, 0.5), 0.5)
    return np.ascontiguousarray(z.T), np.array([kt.rule(weights[:, w], 8, 7)[0] for w in range(NWIN)])


def demonstration_medians(delay_kept, delay_full, delay_clean):
    return tuple(np.median(np.asarray(a), axis=0) for a in (delay_kept, delay_full, delay_clean))


def test_demonstration(oracle):
    rij = synthetic.array_geometry(8, 1.0)
    xij = planner.co_array(rij)[0]
    K = int(planner.element_shifts([0.55], FS)[0])
    assert K == 18
    bad = _band(synthetic.plane_wave(rij, NPTS, FS, 0.1, 5.0, snr_db=10.0, timing_error_s=LATE, bad_element=BAD))
    clean = _band(synthetic.plane_wave(rij, NPTS, FS, 0.1, 5.0, snr_db=10.0))
    zb, mb = _lts(oracle, bad, rij)
    zc, mc = _lts(oracle, clean, rij)
    kept = edt.row64(bad, FS, xij, zb, W, HOP, NWIN, K, dropped=mb)
    full = edt.row64(bad, FS, xij, zb, W, HOP, NWIN, K)
    cln = edt.row64(clean, FS, xij, zc, W, HOP, NWIN, K, dropped=mc)
    mk, mf, mcl = demonstration_medians(kept[0], full[0], cln[0])
    np.set_printoptions(precision=4, suppress=True)
    print('element 7 dropped in %d of %d windows' % (int((mb == 1 << BAD).sum()), NWIN))
    print('kept beam:  medians %s; element 7 range %.3f .. %.3f' % (mk, kept[0][:, BAD].min(), kept[0][:, BAD].max()))
    print('full beam:  medians %s' % (mf,))
    print('clean:      medians %s' % (mcl,))
    print('median cc kept %s' % (np.median(kept[1], axis=0),))
    edt.demonstration_statements(mk, mf, mcl, BAD, LATE, FS)
