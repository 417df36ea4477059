"""The slowness-grid search of the beam F-statistic (``nbls_set_beam_grid``, csrc/beam_grid.hip: beam_grid_kernel; DESIGN.md
section 15) against the long-double reference of tests/grid_truth.py, which follows the definition literally.  Tolerances:
the derived rounding bounds of beam_truth per (window, grid point), E = 64 N W 2^-53 N S_t propagated to F and P.  The
index is accepted if its F can be the largest within the bounds, and must be the reference's where that one leads by more
than both bounds.  The delay table must equal ``np.rint`` of the float64 expression exactly: the tests assert (on the CPU,
from the inputs alone) that no delay lies within 1e-6 of a rounding tie.  Between the forms of a pass (staged in LDS or
read from global memory, streamed, batched, window slices) the results are equal bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import beam_truth as bt
import grid_truth as gt
from narrow_band_least_squares_amd import (engine, planner, synthetic, _hip, ltsva, ltsva_grid, ltsva_batch,
                                           narrow_band_least_squares, narrow_band_least_squares_grid, get_freqlist,
                                           get_winlenlist)

pytestmark = pytest.mark.gpu

FS = 20.0
T0 = 17884.0729166667
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NW = _hip.BEAM_GRID_WAVES
# trace lengths are odd (the padded row length differs from npts); windows hop by half (a quarter at 1200 samples)
NPTS = {16: 601, 65: 1201, 257: 2401, 1200: 6001}
AXIS = np.array([-3.07, -1.535, 0.0, 1.535, 3.07])                # s/km: the wave's slowness is 2.94
GRID5 = np.array([[a, b] for a in AXIS for b in AXIS])            # 5 x 5 points, s = 0 among them


def _wave(N, npts, mistimed=False, seed=900, snr_db=6.0):
    """A plane wave at 6 dB SNR over a 1 km array, fs = 20 Hz -> (data (N, npts), centred rij)."""
    rij = synthetic.array_geometry(N, 1.0)
    data = synthetic.plane_wave(rij, npts, FS, 0.5, 4.0, baz_deg=60.0, snr_db=snr_db, timing_error_s=0.25 if mistimed else 0.0,
                                bad_element=N - 1 if mistimed else None, seed=seed)
    return data, rij - rij.mean(axis=1, keepdims=True)


def _process(data, rij, W, alpha, grid=GRID5, overlap=0.5, **kw):
    res = engine.process(data, FS, T0, rij, [(None, None)], [(W + 0.5) / FS], overlap, alpha, prefiltered=True,
                         slowness_grid=grid, want_grid_map=True, **kw)
    assert int(res.W[0]) == W
    return res


def _fit_for_exact_delays(xij, grid, N):
    """The condition of the delay comparison, from the inputs alone."""
    d, tau = gt.delay_table(xij, grid, FS, N)
    assert not gt.near_tie(tau), 'a delay of this grid lies within 1e-6 of a rounding tie: change the grid'
    return d


def _against_reference(res, filt, grid, band=0, label='', noisy=True):
    n, W, inc = int(res.nwin[band]), int(res.W[band]), int(res.inc[band])
    ref = gt.grid_reference(filt, FS, res.xij, grid, W, inc, n)
    if noisy:
        assert not ref['power_only'].any(), 'a cell of this case is power_only: change the seed'
    for k in range(n):
        gt.check_window(k, ref, int(res.grid_index[band, k]), float(res.grid_fstat[band, k]), float(res.grid_power[band, k]),
                        res.grid_map[band, k])
    fin = np.isfinite(ref['F']) & np.isfinite(ref['tol_fstat'])
    worst = np.max(np.abs(res.grid_map[band, :n] - ref['F'])[fin] / ref['tol_fstat'][fin]) if fin.any() else 0.0
    print('%s N=%d W=%d G=%d: %d windows, worst |dF| / bound = %.3g, index equal to the reference in %d'
          % (label, filt.shape[0], W, len(grid), n, worst, int(np.count_nonzero(res.grid_index[band, :n] == ref['index']))))
    for a in (res.grid_index, res.grid_fstat, res.grid_power, res.grid_map):            # cells beyond nwin are zeros
        assert not a[band, n:].any()
    return ref


@pytest.mark.parametrize('W', [16, 65, 257, 1200])
@pytest.mark.parametrize('N,alpha', [(3, 1.0), (4, 0.5), (9, 0.5)])
def test_matches_the_truth(N, alpha, W):
    """3 elements under OLS, 4 and 9 under LTS; windows of 16 samples (a quarter of a wave's 64 lanes, shorter than the
    delays), 65 (one past the 64 lanes) and 257 (one past a wave's step of GRID_BLOCK = 256 samples: a whole step and a
    partial one of one sample), 1200 (four whole steps and a part).  The lengths at the step's edges themselves are
    tests/test_gpu_seams.py's.  The first window reads before the trace's start: zeros there."""
    npts = NPTS[W]
    data, rij = _wave(N, npts, mistimed=alpha < 1.0)
    xij = planner.co_array(rij)[0]
    d = _fit_for_exact_delays(xij, GRID5, N)
    res = _process(data, rij, W, alpha, overlap=0.75 if W == 1200 else 0.5)
    np.testing.assert_array_equal(res.xij, xij)
    np.testing.assert_array_equal(res.handle.fetch_beam_grid_delays(), d)
    H = int(np.abs(d).max())
    assert _hip.load_library().nbls_beam_grid_lds_bytes(N, W, H) == N * (W + 2 * H) * 8          # the staged form
    ref = _against_reference(res, data, GRID5, label='truth')
    n, inc = int(res.nwin[0]), int(res.inc[0])
    assert d.min() < 0                                                       # window 0 reads before the trace's start
    assert np.all(res.grid_index[0, :n] >= 0) and np.all(np.isfinite(res.grid_fstat[0, :n])) and np.all(res.grid_power[0, :n] > 0)
    assert np.count_nonzero(res.grid_index[0, :n] == ref['index']) >= n // 2


def test_trace_ends():
    """A trace that ends nine samples behind its last window: the first windows read before the start, the last ones
    behind the end, at every grid point with a delay of that sign — zeros there, in the staged block too."""
    N, W, npts = 4, 65, 65 + 32 * 35 + 9
    data, rij = _wave(N, npts)
    d = _fit_for_exact_delays(planner.co_array(rij)[0], GRID5, N)
    res = _process(data, rij, W, 1.0)
    n, inc = int(res.nwin[0]), int(res.inc[0])
    assert (n, inc) == (36, 32) and d.min() < -32 and (n - 2) * inc + W - 1 + d.max() >= npts    # two windows at either end
    ref = _against_reference(res, data, GRID5, label='trace ends')
    for k in (0, 1, n - 2, n - 1):
        assert np.all(np.isfinite(res.grid_map[0, k])) and res.grid_index[0, k] >= 0
    # the zeros are data: the same window cut out of a longer trace, where the neighbours are samples, gives other sums
    longer = np.concatenate((np.ones((N, 64)), data, np.ones((N, 64))), axis=1)
    inner = gt.grid_reference(longer, FS, res.xij, GRID5, W, inc, 1, first=2)
    assert np.any(np.abs(inner['F'][0] - ref['F'][0]) > ref['tol_fstat'][0] + inner['tol_fstat'][0])


@pytest.mark.parametrize('G', [1, NW - 1, NW + 1, 257])
def test_grid_sizes(G):
    """Fewer grid points than waves, one more than waves, and many trips per wave."""
    rng = np.random.default_rng(40)
    grid = np.round(rng.uniform(-3.0, 3.0, (257, 2)), 3)[:G]
    data, rij = _wave(4, 1201)
    d = _fit_for_exact_delays(planner.co_array(rij)[0], grid, 4)
    res = _process(data, rij, 65, 1.0, grid=grid)
    np.testing.assert_array_equal(res.handle.fetch_beam_grid_delays(), d)
    assert res.grid_map.shape[2] == G
    _against_reference(res, data, grid, label='G')


def test_both_forms_give_the_same_bits():
    """The same data and grid with one far grid point appended: the halo no longer fits the LDS cap, the kernel reads
    global memory with the bounds test — and the shared grid points' map columns are the same bits."""
    N, W = 4, 257
    data, rij = _wave(N, NPTS[W])
    xij = planner.co_array(rij)[0]
    lib = _hip.load_library()
    far = np.array([[2600.0 / (FS * np.abs(xij[:N - 1, 0]).max()) + 0.013, 0.0]])
    grid_far = np.concatenate((GRID5, far))
    d = _fit_for_exact_delays(xij, GRID5, N)
    d_far = _fit_for_exact_delays(xij, grid_far, N)
    assert lib.nbls_beam_grid_lds_bytes(N, W, int(np.abs(d).max())) > 0
    assert int(np.abs(d_far).max()) >= 2600 and lib.nbls_beam_grid_lds_bytes(N, W, int(np.abs(d_far).max())) == 0
    staged = _process(data, rij, W, 1.0)
    plain = _process(data, rij, W, 1.0, grid=grid_far)
    np.testing.assert_array_equal(plain.handle.fetch_beam_grid_delays(), d_far)
    np.testing.assert_array_equal(plain.grid_map[..., :len(GRID5)], staged.grid_map)
    _against_reference(staged, data, GRID5, label='staged')
    _against_reference(plain, data, grid_far, label='global')
    n = int(staged.nwin[0])
    same = plain.grid_index[0, :n] < len(GRID5)
    assert same.sum() >= n // 2
    for k in ('grid_index', 'grid_fstat', 'grid_power'):
        np.testing.assert_array_equal(getattr(plain, k)[0, :n][same], getattr(staged, k)[0, :n][same], err_msg=k)


def test_sign_of_the_delays():
    """A noise-free plane wave whose delays are whole samples (np.roll of a periodic signal): the maximum is on the grid
    point that holds exactly those delays, with F +inf or above 1e6, and agrees with the beam results of the same call at
    the solved slowness; the mirrored point has an F of about 1."""
    N, npts, W = 4, 2001, 200
    rij = np.array([[0.0, 0.30, -0.20, 0.10], [0.0, 0.10, 0.40, -0.35]])
    slow = np.array([2.0, 1.0])                                   # s/km: fs * rij . slow are whole samples
    D = np.rint(FS * (slow @ rij)).astype(int)
    assert list(D) == [0, 14, 0, -3]
    rng = np.random.default_rng(77)
    spec = rng.standard_normal(npts // 2 + 1) + 1j * rng.standard_normal(npts // 2 + 1)
    f = np.fft.rfftfreq(npts, 1.0 / FS)
    spec[(f < 0.5) | (f > 4.0)] = 0.0
    s = np.fft.irfft(spec, n=npts)
    data = np.stack([np.roll(s, d) for d in D])                  # x_i[n] = s[n - D_i]: element i lags element 0 by D_i
    grid = np.array([[0.0, 0.0], slow, -slow, [1.0, 2.0], [-1.0, -2.0]])
    xij = planner.co_array(rij)[0]
    d = _fit_for_exact_delays(xij, grid, N)
    true = [g for g in range(len(grid)) if list(d[g]) == list(D)]
    assert len(true) == 1 and true[0] in (1, 2)                   # reading element i at +D_i lines it up with element 0
    true, mirrored = true[0], 3 - true[0]
    assert list(d[mirrored]) == list(-D)
    res = _process(data, rij, W, 1.0, grid=grid, want_z=True, want_beam=True)
    n, inc = int(res.nwin[0]), int(res.inc[0])
    ref = _against_reference(res, data, grid, label='sign', noisy=False)
    beam = bt.beam_reference(data, FS, res.xij, res.z[0], W, inc, n)
    interior = [w for w in range(n) if w * inc + D.min() >= 0 and w * inc + W - 1 + D.max() < npts]
    assert len(interior) >= n - 3
    for w in interior:
        assert res.grid_index[0, w] == true, (w, res.grid_index[0, w])
        gf = res.grid_fstat[0, w]
        assert gf == np.inf or gf > 1e6, (w, gf)
        dz, _ = bt.delays(res.xij[:N - 1], res.z[0, w], FS)
        assert list(dz) == list(D), (w, dz)                       # the solve found the same delays: the same samples
        tol = beam['tol_fstat'][w] + ref['tol_fstat'][w, true]
        bf = res.fstat[0, w]
        assert (np.isinf(tol) and (bf == np.inf or bf > 1e6)) or abs(gf - bf) <= tol, (w, gf, bf, tol)
        assert abs(res.grid_power[0, w] - res.beam_power[0, w]) <= beam['tol_power'][w] + ref['tol_power'][w, true]
    wrong = np.median(res.grid_map[0, interior, mirrored])
    print('interior windows %d of %d; mirrored-point F median %.3g' % (len(interior), n, wrong))
    assert wrong < 3.0


def test_two_bands_with_different_window_lengths(monkeypatch):
    """Filtered on the GPU, two bands whose windows differ (257 and 65 samples): each band against the reference on the
    filtered, tapered samples the kernel read.  The same call in two HBM rounds of one band gives the same bits."""
    data, rij = _wave(4, 2401)
    _fit_for_exact_delays(planner.co_array(rij)[0], GRID5, 4)
    call = lambda: engine.process(data, FS, T0, rij, [(0.5, 1.5), (1.5, 4.0)], [257.5 / FS, 65.5 / FS], 0.5, 1.0, 'butter', 2,
                                  0.01, slowness_grid=GRID5, want_grid_map=True)
    res = call()
    assert [int(w) for w in res.W] == [257, 65] and res.nwin[0] != res.nwin[1]
    for b in range(2):
        _against_reference(res, res.handle.fetch_filtered(b), GRID5, band=b, label='band %d' % b)
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', repr(1.5 * 8.0 * 4 * (2401 + 64) / 2.0 ** 30))
    assert engine.max_bands_per_pass(4, 2401) == 1
    rounds = call()
    for k in ('vel', 'grid_index', 'grid_fstat', 'grid_power', 'grid_map'):
        np.testing.assert_array_equal(getattr(rounds, k), getattr(res, k), err_msg=k)


def test_streamed_in_several_batches_equals_the_unstreamed_pass(monkeypatch):
    data, rij = _wave(9, 48001, mistimed=True)
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    whole = _process(data, rij, 1200, 0.5, overlap=0.75)
    h = engine.get_handle()
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '1')
    try:
        h.set_option('screen_batch_mb', 1)
        h.set_option('solve_min_units', 1)
        streamed = _process(data, rij, 1200, 0.5, overlap=0.75)
        assert h.result_batches() >= 2
        h.set_option('overlap', 1)                                # the per-batch chains on the second stream
        overlapped = _process(data, rij, 1200, 0.5, overlap=0.75)
    finally:
        h.set_option('overlap', 0)
        h.set_option('screen_batch_mb', 192)
        h.set_option('solve_min_units', 0)
    for got in (streamed, overlapped):
        for k in ('vel', 'grid_index', 'grid_fstat', 'grid_power', 'grid_map'):
            np.testing.assert_array_equal(getattr(got, k), getattr(whole, k), err_msg=k)
    n = int(whole.nwin[0])
    assert np.all(np.isfinite(whole.grid_fstat[0, :n])) and np.all(whole.grid_index[0, :n] >= 0)


def test_batch_of_three_recordings_equals_three_single_calls():
    recs = [_wave(4, 1201, mistimed=True, seed=910 + i) for i in range(3)]
    rij = recs[0][1]
    sts = [synthetic.make_stream(d, FS, starttime=T0 + i) for i, (d, _) in enumerate(recs)]
    batch = ltsva_batch(sts, None, None, 65.5 / FS, 0.5, alpha=0.5, rij=rij, slowness_grid=GRID5)
    assert len(batch) == 3
    for got, st in zip(batch, sts):
        exp = ltsva_grid(st, None, None, 65.5 / FS, 0.5, GRID5, alpha=0.5, rij=rij)
        assert len(got) == len(exp) == 13
        for i in (0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12):
            np.testing.assert_array_equal(got[i], exp[i], err_msg='return %d' % i)
        assert list(got[4].keys()) == list(exp[4].keys())
        assert got[12].dtype == np.int32 and np.all(got[12] >= 0)
    assert not np.array_equal(batch[0][10], batch[1][10])
    plain = ltsva(sts[0], None, None, 65.5 / FS, 0.5, alpha=0.5, rij=rij)
    for i in (0, 1, 3, 5):
        np.testing.assert_array_equal(plain[i], batch[0][i])
    with_map = ltsva_grid(sts[0], None, None, 65.5 / FS, 0.5, GRID5, alpha=0.5, rij=rij, grid_map=True)
    assert len(with_map) == 14 and with_map[13].shape == (len(with_map[0]), len(GRID5))
    np.testing.assert_array_equal(with_map[13][np.arange(len(with_map[0])), with_map[12]], with_map[10])


def test_two_window_slices_add_up_to_the_full_call():
    data, rij = _wave(4, 2401, mistimed=True)
    full = _process(data, rij, 65, 0.5)
    parts = [_process(data, rij, 65, 0.5, window_slice=(k, 2)) for k in range(2)]
    n = int(full.nwin[0])
    for k in ('grid_fstat', 'grid_power', 'grid_index', 'grid_map'):
        a, b = getattr(parts[0], k), getattr(parts[1], k)
        assert not np.any((a != 0) & (b != 0))                     # rows outside a slice stay zero
        np.testing.assert_array_equal(a + b, getattr(full, k), err_msg=k)
    assert np.count_nonzero(parts[0].grid_fstat[0, :n]) == n // 2


def test_nan_sample_dead_channel_empty_window_and_duplicated_points():
    W = 65
    data, rij = _wave(4, 2401)
    twice = np.concatenate((GRID5, GRID5))
    # (1) one NaN sample: NaN at exactly the (window, grid point) cells whose reads touch it, never the winner
    bad = data.copy()
    bad[1, 1000] = np.nan
    res = _process(bad, rij, W, 1.0)
    ref = _against_reference(res, bad, GRID5, label='NaN sample', noisy=False)
    n = int(res.nwin[0])
    nan_ref = np.isnan(ref['F'])
    assert 3 <= nan_ref.sum() and nan_ref.any(axis=1).sum() <= 12 and not nan_ref.all(axis=1).any()
    assert np.array_equal(np.isnan(res.grid_map[0, :n]), nan_ref)
    assert np.all(np.isfinite(res.grid_fstat[0, :n]))
    # (2) a dead channel: finite values equal to the reference
    dead = data.copy()
    dead[2] = 0.0
    res = _process(dead, rij, W, 1.0)
    _against_reference(res, dead, GRID5, label='dead channel')
    assert np.all(np.isfinite(res.grid_map[0, :n]))
    # (3) a stretch of zeros on every channel: a window all of whose reads fall into it has no candidate
    gap = data.copy()
    gap[:, 800:1400] = 0.0
    res = _process(gap, rij, W, 1.0)
    ref = _against_reference(res, gap, GRID5, label='empty windows', noisy=False)
    empty = ref['index'] < 0
    assert empty.sum() >= 3
    assert np.all(res.grid_index[0, :n][empty] == -1)
    assert np.all(np.isnan(res.grid_fstat[0, :n][empty])) and np.all(np.isnan(res.grid_power[0, :n][empty]))
    assert np.all(np.isnan(res.grid_map[0, :n][empty]))
    # (4) every grid point given twice: identical delay rows give identical bits, and the first of the two wins
    res = _process(data, rij, W, 1.0, grid=twice)
    _against_reference(res, data, twice, label='duplicated points')
    np.testing.assert_array_equal(res.grid_map[0, :n, :25], res.grid_map[0, :n, 25:])
    assert np.all(res.grid_index[0, :n] < 25) and np.all(res.grid_index[0, :n] >= 0)


def test_plan_without_a_grid_refuses_the_fetches_and_a_pass_without_solve_keeps_the_grids():
    data, rij = _wave(4, 1201)
    engine.process(data, FS, T0, rij, [(None, None)], [65.5 / FS], 0.5, 1.0, prefiltered=True)
    h = engine.get_handle()
    for fetch in (h.fetch_beam_grid, h.fetch_beam_grid_map, h.fetch_beam_grid_delays):
        with pytest.raises(_hip.NblsError) as err:
            fetch()
        assert err.value.code == _hip.NBLS_ERR_STATE
    res = engine.process(data, FS, T0, rij, [(None, None)], [65.5 / FS], 0.5, 1.0, prefiltered=True, slowness_grid=GRID5)
    h = res.handle
    assert res.grid_map is None
    with pytest.raises(_hip.NblsError) as err:                     # the plan did not ask for the map
        h.fetch_beam_grid_map()
    assert err.value.code == _hip.NBLS_ERR_STATE
    before = h.fetch_beam_grid()
    np.testing.assert_array_equal(before[1], res.grid_fstat)
    assert np.any(before[1] != 0)
    h.execute(stages=3)                                          # filter and correlation only
    after = h.fetch_beam_grid()
    for a, b in zip(after, before):
        np.testing.assert_array_equal(a, b)
    # a fresh plan has zeros until a pass has run the solve stage
    h.set_beam_grid(GRID5)
    try:
        h.plan(None, False, None, None, [65], [32], 40)
    finally:
        h.set_beam_grid(None)
    assert not any(a.any() for a in h.fetch_beam_grid())


def test_delay_of_two_to_the_thirty_is_refused_at_plan_time():
    data, rij = _wave(4, 1201)
    res = engine.process(data, FS, T0, rij, [(None, None)], [65.5 / FS], 0.5, 1.0, prefiltered=True)
    h = res.handle
    xmax = np.abs(res.xij[:3]).max()
    for s, ok in ((0.99 * 2.0 ** 30 / (FS * xmax) / 2.0, True), (1.01 * 2.0 ** 30 / (FS * xmax), False)):
        h.set_beam_grid([[0.0, 0.0], [s, 0.0], [0.0, s]])
        try:
            if ok:
                h.plan(None, False, None, None, [65], [32], 40)
                assert np.abs(h.fetch_beam_grid_delays()).max() < 2 ** 30
            else:
                with pytest.raises(ValueError, match='2\\^30'):
                    h.plan(None, False, None, None, [65], [32], 40)
        finally:
            h.set_beam_grid(None)
    for bad in (np.zeros((0, 2)), [[np.nan, 0.0]], [[0.0, np.inf]]):
        with pytest.raises(ValueError):
            h.set_beam_grid(bad)
    h.plan(None, False, None, None, [65], [32], 40)              # the handle is unchanged: the plain plan


def test_rccl_communicator_refuses_the_grid_at_plan_time():
    """A communicator lives as long as its process: a child process over the tests' loopback transport."""
    src = os.path.join(ROOT, 'tests', 'c_caller', 'loopback_rccl.cpp')
    lib = os.path.join(ROOT, 'tests', 'c_caller', 'libloopback_rccl.so')
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.run(['/opt/rocm/bin/hipcc', '-O2', '-shared', '-fPIC', '--offload-arch=gfx950', src, '-o', lib], check=True,
                       timeout=300)
    env = dict(os.environ, NBLS_TEST_TRANSPORT=lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_grid_comm_worker.py')], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and 'GRID_COMM_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_c_caller_runs():
    from test_grid_host import build_grid_caller
    r = subprocess.run([build_grid_caller()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'GRID_CALLER_OK' in r.stdout, r.stdout + r.stderr


def test_whole_call_on_the_example_parameters():
    """``narrow_band_least_squares_grid`` with example.py's parameters (8 bands 0.1-5 Hz, log, cheby1 order 2, adaptive
    windows 60 .. 30 s, half overlap) on a five-minute trace: the first nine returns are ``narrow_band_least_squares``'s,
    the new arrays match the reference band by band."""
    N, npts, ALPHA = 8, 6001, 0.5
    rij0 = synthetic.array_geometry(N, 1.0)
    data = synthetic.plane_wave(rij0, npts, FS, 0.1, 5.0, timing_error_s=0.25, bad_element=N - 1, seed=930)
    rij = rij0 - rij0.mean(axis=1, keepdims=True)
    _fit_for_exact_delays(planner.co_array(rij)[0], GRID5, N)
    st = synthetic.make_stream(data, FS, starttime=T0)
    freqlist, NBANDS, _ = get_freqlist(0.1, 5.0, 'log', 8)
    WINLEN_list = get_winlenlist('adaptive', NBANDS, 50, 60, 30)
    fr = np.logspace(-2, 1, 32)
    args = (WINLEN_list, 0.5, ALPHA, st, None, None, NBANDS, np.zeros(32), np.zeros(32), freqlist, 'log', fr, 'cheby1', 2, 0.01)
    got = narrow_band_least_squares_grid(*args, rij=rij, slowness_grid=GRID5, grid_map=True)
    exp = narrow_band_least_squares(*args, rij=rij)
    assert len(got) == 15 and len(exp) == 9
    for i in (0, 1, 2, 3, 5, 7, 8):
        np.testing.assert_array_equal(got[i], exp[i], err_msg='return %d' % i)
    assert got[6] == exp[6] and list(got[4].keys()) == list(exp[4].keys())
    gvel, gbaz, gf, gp, gi, gmap = got[9:]
    assert gvel.shape == gbaz.shape == gf.shape == gp.shape == gi.shape == got[0].shape and gi.dtype == np.int32
    assert gmap.shape == got[0].shape + (len(GRID5),)
    assert len(narrow_band_least_squares_grid(*args, rij=rij, slowness_grid=GRID5)) == 14
    # the filtered bands of the same pass, through the engine
    edges = [(freqlist[b], freqlist[b + 1]) for b in range(NBANDS)]
    res = engine.process(data, FS, T0, rij, edges, list(WINLEN_list), 0.5, ALPHA, 'cheby1', 2, 0.01, vector_len=got[0].shape[1],
                         slowness_grid=GRID5, want_grid_map=True, groups=1)
    np.testing.assert_array_equal(res.vel, got[0])
    for a, b in ((res.grid_index, gi), (res.grid_fstat, gf), (res.grid_power, gp), (res.grid_map, gmap)):
        np.testing.assert_array_equal(a, b)
    for b in range(NBANDS):
        _against_reference(res, res.handle.fetch_filtered(b), GRID5, band=b, label='band %d' % (b + 1))
        n = int(res.nwin[b])
        s = GRID5[gi[b, :n]]
        with np.errstate(divide='ignore'):
            np.testing.assert_array_equal(gvel[b, :n], 1.0 / np.hypot(s[:, 0], s[:, 1]))
        np.testing.assert_array_equal(gbaz[b, :n], np.mod(np.arctan2(s[:, 0], s[:, 1]) * 180.0 / np.pi - 360.0, 360.0))
        assert not gvel[b, n:].any() and not gbaz[b, n:].any()
