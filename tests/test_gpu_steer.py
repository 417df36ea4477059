"""Fractional-sample steering of the beam and the slowness grid (``nbls_set_beam_interpolation``, csrc/beam.hip,
csrc/beam_grid.hip, csrc/steer.h) against tests/steer_truth.py: the plan's tables bit for bit against
the float64 restatement, the results within the derived long-double bounds, the whole-sample plan's bits where every delay
is a whole sample, and bit-equality between the forms of a pass."""
import os
import subprocess
import sys

import numpy as np
import pytest

import beam_truth as bt
import grid_truth as gt
import kept_truth as kt
import seeded_truth as sdt
import steer_truth as stt
from test_steer_truth import demonstration_statements
from narrow_band_least_squares_amd import (engine, planner, synthetic, _hip, ltsva_beam, ltsva_grid, ltsva_kept, ltsva_steered,
                                           ltsva_steered_batch, narrow_band_least_squares_steered,
                                           narrow_band_least_squares_beam, get_freqlist, get_winlenlist)

pytestmark = pytest.mark.gpu

FS = 20.0
T0 = 17884.0729166667
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXIS = np.array([-3.07, -1.535, 0.0, 1.535, 3.07])
GRID5 = np.array([[a, b] for a in AXIS for b in AXIS])            # 5 x 5 points, s = 0 among them
BEAM = ('beam_power', 'fstat')
GRID = ('grid_index', 'grid_fstat', 'grid_power', 'grid_map')
PLAIN = ('vel', 'baz', 'mdccm', 'sigma_tau', 'mask')


def _same(a, b, keys, label=''):
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and x.dtype == y.dtype, (label, k)
        assert x.tobytes() == y.tobytes() or np.array_equal(x, y, equal_nan=True), (label, k)


def _wave(N, npts, radius=0.15, seed=900, snr_db=6.0, noise_only=False):
    """A plane wave at 6 dB over an array of 300 m (delays of a few samples at 20 Hz, mostly fractional), or noise alone."""
    rij = synthetic.array_geometry(N, radius)
    if noise_only:
        data = np.random.default_rng(seed).standard_normal((N, npts))
    else:
        data = synthetic.plane_wave(rij, npts, FS, 0.5, 4.0, baz_deg=60.0, snr_db=snr_db, seed=seed)
    return np.ascontiguousarray(data), rij - rij.mean(axis=1, keepdims=True)


def _process(data, rij, W, taps, alpha=1.0, grid=GRID5, overlap=0.5, fs=FS, **kw):
    kw = dict(dict(want_beam=True, want_z=True), **kw)
    res = engine.process(data, fs, T0, rij, [(None, None)], [(W + 0.5) / fs], overlap, alpha, prefiltered=True, slowness_grid=grid,
                         want_grid_map=grid is not None, beam_taps=taps, **kw)
    assert int(res.W[0]) == W
    return res


def _tables_equal(res, grid, N, taps):
    n, c, tau, halo = stt.grid_tables(res.xij, grid, FS, N, taps)
    np.testing.assert_array_equal(res.handle.fetch_beam_grid_delays(), n)
    got = res.handle.fetch_beam_grid_coefficients()
    assert got.shape == c.shape and got.tobytes() == c.tobytes()             # bit for bit, the signs of the zeros included
    return n, c, tau, halo


def _against_truth(res, filt, grid, taps, label=''):
    """Beam and grid results of band 0 against (b); prints the worst fraction of the bound reached."""
    N = filt.shape[0]
    n, W, inc = int(res.nwin[0]), int(res.W[0]), int(res.inc[0])
    ref = stt.beam_reference(filt, FS, res.xij, res.z[0], W, inc, n, taps)
    on_f, _ = bt.compare(res.beam_power[0, :n], res.fstat[0, :n], ref)
    fin = np.isfinite(ref['beam_power']) & (ref['tol_power'] > 0)
    wp = np.max(np.abs(res.beam_power[0, :n] - ref['beam_power'])[fin] / ref['tol_power'][fin]) if fin.any() else 0.0
    wg = 0.0
    if grid is not None:
        gref = stt.grid_reference(filt, FS, res.xij, grid, W, inc, n, taps)
        for k in range(n):
            gt.check_window(k, gref, int(res.grid_index[0, k]), float(res.grid_fstat[0, k]), float(res.grid_power[0, k]),
                            res.grid_map[0, k])
        ok = np.isfinite(gref['F']) & np.isfinite(gref['tol_fstat'])
        with np.errstate(invalid='ignore'):
            wg = np.max(np.abs(res.grid_map[0, :n] - gref['F'])[ok] / gref['tol_fstat'][ok]) if ok.any() else 0.0
    print('%s N=%d W=%d taps=%d: %d windows, %d compared on F; worst |dP| / bound %.3g, worst grid |dF| / bound %.3g'
          % (label, N, W, taps, n, on_f, wp, wg))
    for k in BEAM + (GRID if grid is not None else ()):
        assert not getattr(res, k)[0, n:].any()                              # cells beyond nwin are zeros
    return ref, on_f


# ---- the plan's tables ----

def test_coefficient_table_is_the_float64_restatement_bit_for_bit():
    """Grid points whose delays are whole samples, -1e-9 (n = -1, mu just below 1), negative half-integers and ordinary
    fractions; a delay just below 2^30 is planned (the global form), one that reaches it is refused as today."""
    N, W = 3, 64
    rij = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    data = np.random.default_rng(5).standard_normal((N, 400))
    grid = np.array([[0.05, 0.1], [-0.05, -0.15], [1e-9 / FS, -1e-9 / FS], [0.025, -0.075], [-0.125, 0.025], [0.0, 0.0],
                     [0.0371, -0.1234], [1.0 / 3.0, -2.0 / 7.0]])
    for taps in stt.TAPS:
        res = _process(data, rij, W, taps, grid=grid)
        n, c, tau, halo = _tables_equal(res, grid, N, taps)
        mu = tau - n
        assert np.all(tau[0] == np.rint(tau[0])) and np.all(tau[1] == np.rint(tau[1])) and np.any(tau[0] != 0)
        assert np.any((n[2] == -1) & (mu[2] > 0.999999)) and np.any((n[2] == 0) & (0 < mu[2]) & (mu[2] < 1e-8))
        assert np.any((tau[3] < 0) & (mu[3] == 0.5)) and np.any((tau[4] < 0) & (mu[4] == 0.5))
        K = taps // 2
        assert np.all(c[5, :, K - 1] == 1.0) and not np.delete(c[5], K - 1, axis=1).any()
        assert _hip.load_library().nbls_beam_grid_lds_bytes(N, W, halo) == N * (W + 2 * halo) * 8
        _against_truth(res, data, grid, taps, label='tables')
    # near 2^30: planned below (every tap outside the trace: zeros, the window's own element 0 alone), refused at it
    big = 2.0 ** 30
    xmax = np.abs(res.xij[:N - 1]).max()
    far = np.array([[0.0, 0.0], [(big - 0.5) / FS / xmax, 0.0]])
    res = _process(data, rij, W, 8, grid=far)
    n, c, tau, halo = _tables_equal(res, far, N, 8)
    assert np.abs(n).max() in (2 ** 30 - 1, 2 ** 30) and halo >= 2 ** 30 - 1
    assert _hip.load_library().nbls_beam_grid_lds_bytes(N, W, min(halo, 2 ** 31 - 1)) == 0
    _against_truth(res, data, far, 8, label='far')
    with pytest.raises(ValueError, match='2\\^30'):
        _process(data, rij, W, 8, grid=np.array([[(big + 1.0) / FS / xmax, 0.0]]))


# ---- whole-sample delays: the whole-sample plan's bits ----

@pytest.mark.parametrize('taps', stt.TAPS)
def test_whole_sample_delays_give_the_whole_sample_plans_bits(taps):
    """fs = 16 Hz, element offsets in whole km and grid points in multiples of 1/16 s/km: every tau is an integer, exactly.
    The traces are one signal with a little noise of their own, so every lag is picked at 0 and the solved z is exactly 0:
    the beam's delays are whole samples as well."""
    fs, N, W = 16.0, 5, 257
    rij = np.array([[0.0, 1.0, -2.0, 3.0, 0.0], [0.0, 2.0, 1.0, -1.0, -3.0]])
    rng = np.random.default_rng(31)
    s = np.convolve(rng.standard_normal(1400), np.hanning(9), mode='same')
    data = np.ascontiguousarray(s[None, :] + 0.05 * rng.standard_normal((N, 1400)))
    ax = np.array([-0.1875, -0.0625, 0.0, 0.125, 0.25])
    grid = np.array([[a, b] for a in ax for b in ax])
    on = _process(data, rij, W, taps, grid=grid, fs=fs)
    off = _process(data, rij, W, 0, grid=grid, fs=fs)
    n = int(on.nwin[0])
    assert n >= 4 and not on.z[0, :n].any()                                  # z == 0 in every window
    tau = np.float64(fs) * (on.xij[:N - 1, None, 0] * grid[None, :, 0] + on.xij[:N - 1, None, 1] * grid[None, :, 1])
    assert np.all(tau == np.rint(tau)) and np.abs(tau).max() >= 8
    np.testing.assert_array_equal(on.handle.fetch_beam_grid_delays(), off.handle.fetch_beam_grid_delays())
    _same(on, off, PLAIN + BEAM + GRID, 'taps %d' % taps)
    assert np.all(np.isfinite(on.fstat[0, :n])) and len(np.unique(on.grid_index[0, :n])) >= 1 and np.all(on.grid_index[0, :n] >= 0)
    with pytest.raises(_hip.NblsError):                                      # the whole-sample plan has no coefficient table
        off.handle.fetch_beam_grid_coefficients()


# ---- against the long-double truth ----

CASES = [(3, 16, 4, True), (4, 255, 6, False), (8, 256, 8, False), (9, 257, 4, True), (32, 512, 8, False), (4, 513, 6, True),
         (8, 1025, 8, False), (3, 512, 6, False), (9, 513, 8, True), (32, 16, 4, False), (8, 257, 6, False), (4, 1025, 4, True)]


@pytest.mark.parametrize('N,W,taps,noise', CASES)
def test_matches_the_truth(N, W, taps, noise):
    """Every N of {3, 4, 8, 9, 32}, every W of {16, 255, 256, 257, 512, 513, 1025} — the beam's switch from one wave to four
    at 512 and the grid's 256-sample step — and every tap count, on noise and on a wave in noise.  The trace ends one sample
    behind its last window: the first and the last windows read taps off both ends."""
    inc = int(planner.window_plan(10 ** 6, FS, (W + 0.5) / FS, 0.5)[1])
    npts = W + 3 * inc + 1
    data, rij = _wave(N, npts, noise_only=noise, seed=700 + N + W)
    grid = GRID5[::2] if N * W > 8000 else GRID5                             # (13 points for the large cases: the truth's time)
    res = _process(data, rij, W, taps, grid=grid)
    n = int(res.nwin[0])
    assert n == 4 and int(res.inc[0]) == inc
    tn, _, _, halo = _tables_equal(res, grid, N, taps)
    K = taps // 2
    assert tn.min() - K + 1 < 0 and (n - 1) * inc + W - 1 + tn.max() + K >= npts      # taps off both ends
    assert _hip.load_library().nbls_beam_grid_lds_bytes(N, W, halo) > 0      # the staged form
    ref, on_f = _against_truth(res, data, grid, taps, label='noise' if noise else 'wave')
    if not noise:
        assert on_f >= 1 and np.all(res.grid_index[0, :n] >= 0)


def test_nan_sample_and_nan_slowness():
    """A NaN sample: NaN in exactly the windows whose taps touch it (a zero coefficient is still multiplied).  A stretch
    where every element records the same samples: all lags 0, under LTS a slowness that is not finite — NaN beam results,
    while the grid, which does not read z, still has its maximum there."""
    N, W, taps = 4, 65, 8
    data, rij = _wave(N, 1201)
    data[:, :400] = data[0, :400]
    data[1, 900] = np.nan
    res = _process(data, rij, W, taps, alpha=0.5)
    n = int(res.nwin[0])
    ref, _ = _against_truth(res, data, GRID5, taps, label='NaN')
    nan_z = ~np.isfinite(res.z[0, :n]).all(axis=1)
    assert nan_z.sum() >= 3 and not nan_z[n // 2:].any()                     # units with NaN z: NaN beam results
    assert np.all(np.isnan(res.beam_power[0, :n][nan_z])) and np.all(np.isnan(res.fstat[0, :n][nan_z]))
    assert np.all(res.grid_index[0, :n][nan_z] >= 0)
    assert np.array_equal(np.isnan(res.beam_power[0, :n]), np.isnan(ref['beam_power']))
    touched = np.isnan(ref['beam_power']) & ~nan_z
    assert 1 <= touched.sum() <= 6 and np.all(np.isnan(res.grid_fstat[0, :n][touched]) | (res.grid_index[0, :n][touched] >= 0))


# ---- the two forms of the grid kernel ----

@pytest.mark.parametrize('taps', [4, 8])
def test_both_grid_forms_give_the_same_bits(taps):
    N, W = 4, 257
    data, rij = _wave(N, 1201)
    xij = planner.co_array(rij)[0]
    far = np.array([[2600.0 / (FS * np.abs(xij[:N - 1, 0]).max()) + 0.013, 0.0]])
    grid_far = np.concatenate((GRID5, far))
    lib = _hip.load_library()
    staged = _process(data, rij, W, taps)
    plain = _process(data, rij, W, taps, grid=grid_far)
    h_near = stt.grid_tables(xij, GRID5, FS, N, taps)[3]
    h_far = _tables_equal(plain, grid_far, N, taps)[3]
    assert lib.nbls_beam_grid_lds_bytes(N, W, h_near) > 0 and h_far >= 2600 and lib.nbls_beam_grid_lds_bytes(N, W, h_far) == 0
    np.testing.assert_array_equal(plain.grid_map[..., :len(GRID5)], staged.grid_map)
    assert plain.grid_map[..., :len(GRID5)].tobytes() == staged.grid_map.tobytes()
    n = int(staged.nwin[0])
    same = plain.grid_index[0, :n] < len(GRID5)
    assert same.sum() >= n // 2
    for k in GRID[:3]:
        np.testing.assert_array_equal(getattr(plain, k)[0, :n][same], getattr(staged, k)[0, :n][same], err_msg=k)
    _same(plain, staged, PLAIN + BEAM)
    _against_truth(plain, data, grid_far, taps, label='global')


# ---- the kept-elements beam ----

def _mistimed(N, npts, bad, second=None):
    rij = synthetic.array_geometry(N, 0.15)
    data = synthetic.plane_wave(rij, npts, FS, 0.5, 4.0, baz_deg=60.0, snr_db=10.0, seed=900, timing_error_s=0.25, bad_element=bad)
    if second is not None:
        data[second] = np.roll(data[second], -7)
    return np.ascontiguousarray(data), rij - rij.mean(axis=1, keepdims=True)


@pytest.mark.parametrize('N,bad,second', [(8, 0, None), (8, 4, None), (8, 7, None), (9, 0, 8), (9, 4, None)])
def test_kept_beam_against_the_truth(N, bad, second):
    """Element 0, a middle element and the last element mistimed so that LTS drops them: the sums over the kept set, the
    delays against its first element (the co-array row of pair (e_0, e_i))."""
    W, taps = 257, 8
    data, rij = _mistimed(N, W * 4 + 1, bad, second)
    res = _process(data, rij, W, taps, alpha=0.5, grid=None, kept=(N - 1, True, False))
    n, inc = int(res.nwin[0]), int(res.inc[0])
    named = sum(1 << e for e in (bad, second) if e is not None)
    assert np.count_nonzero(res.dropped_mask[0, :n] == named) >= n // 2, res.dropped_mask[0, :n]
    rows = []
    for w in range(n):
        kept = kt.kept_of_mask(res.dropped_mask[0, w], N)
        e0 = kept[0]
        xr = np.array([res.xij[e0 * (2 * N - e0 - 1) // 2 + (e - e0 - 1)] for e in kept[1:]])
        rows.append(stt.beam_reference(data[list(kept)], FS, xr, res.z[0], W, inc, 1, taps, first=w))
    ref = {k: np.concatenate([r[k] for r in rows]) for k in rows[0]}
    on_f, _ = bt.compare(res.beam_power[0, :n], res.fstat[0, :n], ref)
    assert on_f >= n // 2
    full = _process(data, rij, W, taps, alpha=0.5, grid=None)
    hit = res.dropped_mask[0, :n] != 0
    _same(res, full, PLAIN)
    assert np.all(res.fstat[0, :n][hit] != full.fstat[0, :n][hit])
    assert res.fstat[0, :n][~hit].tobytes() == full.fstat[0, :n][~hit].tobytes()
    assert np.median(res.fstat[0, :n][hit]) > np.median(full.fstat[0, :n][hit])


def test_kept_plan_that_drops_nothing_gives_the_plain_interpolated_bits():
    N, W = 8, 257
    data, rij = _wave(N, W * 3, snr_db=10.0)
    for alpha in (1.0, 0.5):
        on = _process(data, rij, W, 8, alpha=alpha, grid=None, kept=(N - 1, True, False))
        off = _process(data, rij, W, 8, alpha=alpha, grid=None)
        assert not on.dropped_mask.any()
        _same(on, off, PLAIN + BEAM, 'alpha %g' % alpha)


# ---- the forms of a pass ----

EDGES = [(0.5, 1.5), (1.5, 4.0)]
WINLENS = [257.5 / FS, 65.5 / FS]
FILTER = ('butter', 2, 0.01)
FORM_KW = dict(want_beam=True, slowness_grid=GRID5, want_grid_map=True, beam_taps=8)
FORM_FIELDS = PLAIN + BEAM + GRID


def _recordings(npts=2401, S=3, N=6):
    rij = synthetic.array_geometry(N, 0.15)
    data = [np.ascontiguousarray(synthetic.plane_wave(rij, npts, FS, 0.5, 4.0, baz_deg=20.0 + 67.0 * i, snr_db=10.0, seed=520 + i))
            for i in range(S)]
    return data, rij - rij.mean(axis=1, keepdims=True), [T0 + 0.0173 * i for i in range(S)]


def _two_bands(data, rij, t0=T0, **kw):
    return engine.process(data, FS, t0, rij, EDGES, WINLENS, 0.5, 0.5, *FILTER, **dict(FORM_KW, **kw))


def test_batch_of_three_recordings_equals_three_single_calls():
    recs, rij, t0s = _recordings()
    batch = engine.process_batch([list(d) for d in recs], FS, t0s, rij, EDGES, WINLENS, 0.5, 0.5, *FILTER, **FORM_KW)
    assert len(batch) == 3
    for s in range(3):
        single = _two_bands(recs[s], rij, t0s[s])
        assert [int(w) for w in single.W] == [257, 65]
        _same(batch[s], single, FORM_FIELDS, 'recording %d' % s)
    assert not np.array_equal(batch[0].fstat, batch[1].fstat)
    # ... and they differ from the whole-sample plan's
    whole = _two_bands(recs[0], rij, t0s[0], beam_taps=0)
    _same(whole, batch[0], PLAIN)
    assert not np.array_equal(whole.fstat, batch[0].fstat) and not np.array_equal(whole.grid_map, batch[0].grid_map)


def test_streamed_overlapped_and_two_round_passes_equal_the_plain_pass(monkeypatch):
    recs, rij, _ = _recordings(24001, 1)
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    whole = _two_bands(recs[0], rij)
    h = engine.get_handle()
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '1')
    for overlap in (1, -1):
        try:
            h.set_option('screen_batch_mb', 1)
            h.set_option('solve_min_units', 1)
            h.set_option('overlap', overlap)
            streamed = _two_bands(recs[0], rij)
            nbatches = h.result_batches()
        finally:
            h.set_option('screen_batch_mb', 192)
            h.set_option('solve_min_units', 0)
            h.set_option('overlap', 0)
        assert nbatches >= 3, nbatches
        _same(streamed, whole, FORM_FIELDS, 'streamed, overlap %d' % overlap)
    # two HBM rounds of one band each
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', repr(1.5 * 8.0 * 6 * (24001 + 64) / 2.0 ** 30))
    assert engine.max_bands_per_pass(6, 24001) == 1
    rounds = _two_bands(recs[0], rij)
    _same(rounds, whole, FORM_FIELDS, 'two rounds')


def test_second_estimators_beam():
    """Two estimators of one pass: estimator 1 drops element 2; its beam equals the single call on the reduced array."""
    N, W = 6, 257
    data, rij = _wave(N, W * 3 + 1, snr_db=10.0)
    keep = [0, 1, 3, 4, 5]
    rijs = [rij, np.ascontiguousarray(rij[:, keep])]
    h = engine.get_handle()
    prep0 = engine.prepare(N, data.shape[1], FS, rij, [(None, None)], [(W + 0.5) / FS], 0.5, 1.0, prefiltered=True)
    xij1, pair1, xpinv1 = planner.co_array(rijs[1])
    engine.launch(h, list(data), prep0, beam=True, beam_taps=8,
                  estimators=[dict(lts=None, kept=keep, xij=xij1, pair_idx=pair1, xpinv=xpinv1, eig6=None)])
    h.sync()
    multi = [np.stack(h.fetch_beam(e)) for e in (0, 1)]
    for e, (d, r) in enumerate(((data, rij), (np.ascontiguousarray(data[keep]), rijs[1]))):
        single = _process(d, r, W, 8, grid=None)
        n = int(single.nwin[0])
        assert multi[e][0, 0, :n].tobytes() == single.beam_power[0, :n].tobytes(), e
        assert multi[e][1, 0, :n].tobytes() == single.fstat[0, :n].tobytes(), e
    h.set_estimators(())


# ---- the seeded plan ----

def test_seeded_plan_picks_around_the_interpolated_grid_maximum():
    N, W, K = 6, 257, 3
    data, rij = _wave(N, W * 3 + 1, snr_db=10.0)
    res = _process(data, rij, W, 8, seed_halfwidths=[K], want_lag=True)
    n = int(res.nwin[0])
    tn = _tables_equal(res, GRID5, N, 8)[0]
    _against_truth(res, data, GRID5, 8, label='seeded')
    pairs = [tuple(p) for p in res.pair_idx]
    c = sdt.centres(tn, res.grid_index[0, :n], pairs)                        # the seed: n[g][j] - n[g][i] of the plan's table
    lag, _ = sdt.pick_windows(data, W, [w * int(res.inc[0]) for w in range(n)], pairs, c, K)
    np.testing.assert_array_equal(res.lag[0, :n], lag)


# ---- off again, refusals ----

def test_off_after_on_gives_the_bits_of_a_handle_that_never_asked():
    data, rij = _wave(4, 1201)
    first = _process(data, rij, 257, 0)
    _process(data, rij, 257, 8)
    again = _process(data, rij, 257, 0)
    _same(first, again, PLAIN + BEAM + GRID)
    h = again.handle
    with pytest.raises(_hip.NblsError) as err:
        h.fetch_beam_grid_coefficients()
    assert err.value.code == _hip.NBLS_ERR_STATE
    np.testing.assert_array_equal(h.fetch_beam_grid_delays(), gt.delay_table(again.xij, GRID5, FS, 4)[0])


def test_refusals_of_the_library():
    h = engine.get_handle()
    for bad in (1, 2, 3, 5, 7, 9, 16, -8):
        with pytest.raises(ValueError):
            h.set_beam_interpolation(bad)
    data, rij = _wave(4, 601)
    xij, pair_idx, xpinv = planner.co_array(rij)
    h.set_trace(data, FS)
    h.set_geometry(xij, pair_idx, xpinv)
    h.set_beam_interpolation(8)
    try:
        with pytest.raises(_hip.NblsError) as err:                           # neither the beam nor a grid
            h.plan(None, False, None, None, [65], [32], 40)
        assert err.value.code == _hip.NBLS_ERR_STATE and 'nbls_set_beam_interpolation' in str(err.value)
        h.set_beam(True)
        h.plan(None, False, None, None, [65], [32], 40)                      # sticky: the next plan interpolates too
        h.plan(None, False, None, None, [65], [32], 40)
        with pytest.raises(_hip.NblsError) as err:                           # no grid: no table
            h.fetch_beam_grid_coefficients()
        assert err.value.code == _hip.NBLS_ERR_STATE
    finally:
        h.set_beam(False)
        h.set_beam_interpolation(0)
    h.plan(None, False, None, None, [65], [32], 40)


def test_rccl_communicator_refuses_an_interpolated_plan():
    """A communicator lives as long as its process: a child process over the tests' loopback transport."""
    src = os.path.join(ROOT, 'tests', 'c_caller', 'loopback_rccl.cpp')
    lib = os.path.join(ROOT, 'tests', 'c_caller', 'libloopback_rccl.so')
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.run(['/opt/rocm/bin/hipcc', '-O2', '-shared', '-fPIC', '--offload-arch=gfx950', src, '-o', lib], check=True,
                       timeout=300)
    env = dict(os.environ, NBLS_TEST_TRANSPORT=lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_steer_comm_worker.py')], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and 'STEER_COMM_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the demonstration and the public entry points ----

@pytest.fixture(scope='module')
def demo():
    d = stt.demonstration()
    d['st'] = synthetic.make_stream(d['filt'], d['fs'], starttime=T0)
    return d


def test_demonstration_on_the_small_aperture_array(demo):
    """The three statements of tests/test_steer_truth.py on the GPU's maps of the same eight windows (hop 600, the first at
    sample 300: the trace from sample 300 on, windows of 400 samples every 600)."""
    d = demo
    data = np.ascontiguousarray(d['filt'][:, 300:])
    maps = {}
    for taps in (0, 8):
        res = engine.process(data, d['fs'], T0, d['rij'], [(None, None)], [400.5 / d['fs']], 1.0 - 600.0 / 400.0, 1.0,
                             prefiltered=True, slowness_grid=d['grid'], want_grid_map=True, beam_taps=taps)
        assert int(res.W[0]) == 400 and int(res.inc[0]) == 600 and int(res.nwin[0]) >= 8
        np.testing.assert_array_equal(res.xij, d['xij'])
        maps[taps] = res.grid_map[0, :8].copy()
        assert np.array_equal(res.grid_index[0, :8], [int(np.argmax(f)) for f in maps[taps]])
    rows = len({tuple(r) for r in gt.delay_table(d['xij'], d['grid'], d['fs'], 8)[0]})
    ties0, ties8, err0, err8 = demonstration_statements(d['grid'], d['true'], maps[0], maps[8], rows)
    print('ties per window: whole samples %s, 8 taps %s; median slowness error %.3f -> %.3f s/km; median F %.1f -> %.1f'
          % (ties0, ties8, err0, err8, np.median(maps[0].max(axis=1)), np.median(maps[8].max(axis=1))))


def test_public_entry_points_on_the_demonstration_trace(demo):
    d = demo
    st, rij, grid = demo['st'], demo['rij'], demo['grid'][::7]
    out = ltsva_steered(st, None, None, 20.0, 0.5, rij=rij)
    plain = ltsva_beam(st, None, None, 20.0, 0.5, rij=rij)
    assert len(out) == 10
    for i in range(8):
        assert np.array_equal(out[i], plain[i], equal_nan=True) if not isinstance(out[i], dict) else out[i] == plain[i]
    assert not np.array_equal(out[9], plain[9]) and np.all(np.isfinite(out[9]))
    assert ltsva_steered(st, None, None, 20.0, 0.5, rij=rij, taps=0)[9].tobytes() == plain[9].tobytes()
    # beam F at the OLS slowness of a subsample plan, taps 0 and 8 (recorded; asserted: the median is not lower)
    f0 = ltsva_steered(st, None, None, 20.0, 0.5, rij=rij, taps=0, subsample=True)[9]
    f8 = ltsva_steered(st, None, None, 20.0, 0.5, rij=rij, taps=8, subsample=True)[9]
    print('subsample plan, beam F at the OLS slowness: median %.2f (whole samples) -> %.2f (8 taps)' % (np.median(f0), np.median(f8)))
    assert np.median(f8) >= np.median(f0)
    # the grid returns and the map
    og = ltsva_steered(st, None, None, 20.0, 0.5, rij=rij, slowness_grid=grid, grid_map=True)
    wg = ltsva_grid(st, None, None, 20.0, 0.5, grid, rij=rij, grid_map=True)
    assert len(og) == 16 and og[15].shape == wg[13].shape and og[14].dtype == np.int32
    assert og[9].tobytes() == out[9].tobytes() and not np.array_equal(og[15], wg[13])
    # kept: ltsva_kept's 9-tuple
    ok = ltsva_steered(st, None, None, 20.0, 0.5, alpha=0.75, rij=rij, kept=True)
    wk = ltsva_kept(st, None, None, 20.0, 0.5, alpha=0.75, rij=rij)
    assert len(ok) == 9 and sorted(ok[8]) == sorted(wk[8]) and np.array_equal(ok[8]['kept_count'], wk[8]['kept_count'])
    # the batch: three recordings, bit for bit
    sts = [st, synthetic.make_stream(d['filt'][:, ::-1].copy(), d['fs'], starttime=T0), st]
    batch = ltsva_steered_batch(sts, None, None, 20.0, 0.5, rij=rij, slowness_grid=grid)
    assert len(batch) == 3
    for s, b in zip(sts, batch):
        single = ltsva_steered(s, None, None, 20.0, 0.5, rij=rij, slowness_grid=grid)
        assert len(b) == len(single) == 15
        for x, y in zip(b, single):
            assert (x == y) if isinstance(x, dict) else np.array_equal(x, y, equal_nan=True)
    # the narrow-band call: the beam arrays of two bands filtered on the GPU
    raw = synthetic.make_stream(synthetic.plane_wave(rij, 6001, 20.0, 0.1, 8.0, baz_deg=225, vel_kms=0.34, snr_db=6.0), 20.0,
                                starttime=T0)
    freqlist, NBANDS, _ = get_freqlist(0.5, 4.0, 'log', 2)
    WINLEN_list = get_winlenlist('adaptive', NBANDS, 20, 30, 20)
    fr = np.logspace(-2, 1, 16)
    args = (WINLEN_list, 0.5, 1.0, raw, None, None, NBANDS, np.zeros(16), np.zeros(16), freqlist, 'log', fr, 'butter', 2, 0.01)
    got = narrow_band_least_squares_steered(*args, rij=rij, slowness_grid=grid)
    exp = narrow_band_least_squares_beam(*args, rij=rij)
    assert len(got) == 16 and len(exp) == 11
    for i in (0, 1, 2, 3, 5, 7, 8):
        np.testing.assert_array_equal(got[i], exp[i], err_msg='return %d' % i)
    assert got[9].shape == exp[9].shape and not np.array_equal(got[10], exp[10]) and got[15].dtype == np.int32
