"""Beam power and Fisher F-statistic at the solved slowness (``nbls_set_beam``, csrc/beam.hip: beam_fstat_kernel; DESIGN.md
section 12) against the long-double reference of tests/beam_truth.py, which follows the definition literally and takes
the slowness as fetched from the GPU.  Tolerance: the derived rounding bound of beam_truth (E = 64 N W 2^-53 N S_t);
windows with a delay within 1e-6 of a rounding tie are left out (at most 1 % of a test's cells).  Between the forms of a
pass (streamed, batched, several estimators, window slices) the results are equal bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import beam_truth as bt
from narrow_band_least_squares_amd import (engine, synthetic, _hip, ltsva, ltsva_beam, ltsva_batch, ltsva_multi,
                                           narrow_band_least_squares, narrow_band_least_squares_beam, get_freqlist,
                                           get_winlenlist)

pytestmark = pytest.mark.gpu

FS = 20.0
T0 = 17884.0729166667
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# trace lengths are odd (the padded row length differs from npts); windows hop by half (a quarter at 1200 samples)
NPTS = {16: 601, 65: 1201, 257: 2401, 1200: 6001}


def _wave(N, npts, mistimed=False, seed=900, snr_db=6.0):
    """A plane wave at 6 dB SNR over a 1 km array, fs = 20 Hz -> (data (N, npts), centred rij)."""
    rij = synthetic.array_geometry(N, 1.0)
    data = synthetic.plane_wave(rij, npts, FS, 0.5, 4.0, baz_deg=60.0, snr_db=snr_db, timing_error_s=0.25 if mistimed else 0.0,
                                bad_element=N - 1 if mistimed else None, seed=seed)
    return data, rij - rij.mean(axis=1, keepdims=True)


def _process(data, rij, W, alpha, overlap=0.5, **kw):
    res = engine.process(data, FS, T0, rij, [(None, None)], [(W + 0.5) / FS], overlap, alpha, prefiltered=True, want_z=True,
                         want_beam=True, **kw)
    assert int(res.W[0]) == W
    return res


def _reads_outside(xij, z, W, inc, nwin, npts, N):
    """How many of the row's windows read before the trace's start or behind its end."""
    n = 0
    for w in range(nwin):
        d, _ = bt.delays(xij[:N - 1], z[w], FS)
        if d is not None and (w * inc + d.min() < 0 or w * inc + W - 1 + d.max() >= npts):
            n += 1
    return n


def _against_reference(res, filt, band=0, label=''):
    n, W, inc = int(res.nwin[band]), int(res.W[band]), int(res.inc[band])
    ref = bt.beam_reference(filt, FS, res.xij, res.z[band], W, inc, n)
    on_f, skipped = bt.compare(res.beam_power[band, :n], res.fstat[band, :n], ref)
    dp = np.nanmax(np.abs(res.beam_power[band, :n] - ref['beam_power']) / np.maximum(ref['tol_power'], 1e-300))
    print('%s N=%d W=%d: %d windows, %d compared on fstat, %d skipped, worst |d power| / bound = %.3g, fstat median %.3g'
          % (label, filt.shape[0], W, n, on_f, skipped, dp, np.nanmedian(ref['fstat'])))
    assert not res.beam_power[band, n:].any() and not res.fstat[band, n:].any()         # cells beyond nwin are zeros
    return ref, on_f


@pytest.mark.parametrize('W', [16, 65, 257, 1200])
@pytest.mark.parametrize('N,alpha', [(3, 1.0), (4, 0.5), (9, 0.5)])
def test_matches_the_reference(N, alpha, W):
    """3 elements under OLS, 4 under LTS with one mistimed element, 9 under LTS (the bucket kernel); windows of 16 samples
    (a quarter of a wave's lanes, shorter than the delays), 65 (one sample past the 64 lanes: lane 0 alone has a second
    sample) and 257 (one past a wave's trip of 64 * BEAM_TU = 256 samples: a second trip of one sample) — all three
    summed by ONE wave per unit, as every window up to BEAM_WAVE_W = 512 samples is — and 1200 (the four waves of the
    workgroup per unit: one whole trip of 1024 samples and a part).  The lengths at the edges themselves are
    tests/test_gpu_seams.py's.  The first or the last windows read outside the trace: zeros there."""
    npts = NPTS[W]
    data, rij = _wave(N, npts, mistimed=alpha < 1.0)
    res = _process(data, rij, W, alpha, overlap=0.75 if W == 1200 else 0.5)
    ref, on_f = _against_reference(res, data, label='reference')
    n = int(res.nwin[0])
    assert on_f >= n // 2
    assert _reads_outside(res.xij, res.z[0], W, int(res.inc[0]), n, npts, N) >= 1
    assert np.all(np.isfinite(res.fstat[0, :n])) and np.all(res.beam_power[0, :n] > 0)


def test_two_bands_with_different_window_lengths(monkeypatch):
    """Filtered on the GPU, two bands whose windows differ (257 and 65 samples): each band against the reference on the
    filtered, tapered samples the kernel read.  The same call in two HBM rounds of one band gives the same bits."""
    data, rij = _wave(4, 2401)
    call = lambda: engine.process(data, FS, T0, rij, [(0.5, 1.5), (1.5, 4.0)], [257.5 / FS, 65.5 / FS], 0.5, 1.0, 'butter', 2,
                                  0.01, want_z=True, want_beam=True)
    res = call()
    assert [int(w) for w in res.W] == [257, 65] and res.nwin[0] != res.nwin[1]
    for b in range(2):
        _against_reference(res, res.handle.fetch_filtered(b), band=b, label='band %d' % b)
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', repr(1.5 * 8.0 * 4 * (2401 + 64) / 2.0 ** 30))
    assert engine.max_bands_per_pass(4, 2401) == 1
    rounds = call()
    for k in ('vel', 'z', 'beam_power', 'fstat'):
        np.testing.assert_array_equal(getattr(rounds, k), getattr(res, k), err_msg=k)


def test_sign_of_the_delays():
    """A noise-free plane wave whose delays are whole samples (np.roll of a periodic signal): lined up with the right sign
    every interior window has S_b = N S_t within the bound, fstat is inf or above 1e6; the wrong sign gives about 1."""
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
    res = _process(data, rij, W, 1.0)
    n, inc = int(res.nwin[0]), int(res.inc[0])
    ref = bt.beam_reference(data, FS, res.xij, res.z[0], W, inc, n)
    wrong = bt.beam_reference(data, FS, res.xij, -res.z[0], W, inc, n)
    interior = [w for w in range(n) if w * inc + (D - D[0]).min() >= 0 and w * inc + W - 1 + (D - D[0]).max() < npts]
    assert len(interior) >= n - 3 and not ref['skip'].any()
    for w in interior:
        d, _ = bt.delays(res.xij[:N - 1], res.z[0, w], FS)
        assert list(d) == list(D - D[0]), (w, d)
        E = 64.0 * N * W * 2.0 ** -53 * N * float(ref['S_t'][w])
        assert abs(float(ref['D'][w])) <= 2 * E
        p, fst = res.beam_power[0, w], res.fstat[0, w]
        assert abs(p - ref['beam_power'][w]) <= ref['tol_power'][w]
        assert fst == np.inf or fst > 1e6, (w, fst)
        S_b = p * N * N * W
        assert (N - 1) * S_b / fst <= 2 * E                       # D of the GPU's sums: S_b = N S_t within the bound
    print('interior windows %d of %d; wrong-sign fstat median %.3g' % (len(interior), n, np.median(wrong['fstat'][interior])))
    assert np.median(wrong['fstat'][interior]) < 3.0


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
        for k in ('vel', 'z', 'beam_power', 'fstat'):
            np.testing.assert_array_equal(getattr(got, k), getattr(whole, k), err_msg=k)
    assert np.all(np.isfinite(whole.fstat[0, :int(whole.nwin[0])]))


def _same_tuple(got, exp):
    assert len(got) == len(exp) == 10
    for i in (0, 1, 2, 3, 5, 6, 7, 8, 9):
        np.testing.assert_array_equal(got[i], exp[i], err_msg='return %d' % i)
    assert list(got[4].keys()) == list(exp[4].keys())


def test_batch_of_three_recordings_equals_three_single_calls():
    recs = [_wave(4, 1201, mistimed=True, seed=910 + i) for i in range(3)]
    rij = recs[0][1]
    sts = [synthetic.make_stream(d, FS, starttime=T0 + i) for i, (d, _) in enumerate(recs)]
    batch = ltsva_batch(sts, None, None, 65.5 / FS, 0.5, alpha=0.5, rij=rij, beam=True)
    assert len(batch) == 3
    for got, st in zip(batch, sts):
        _same_tuple(got, ltsva_beam(st, None, None, 65.5 / FS, 0.5, alpha=0.5, rij=rij))
    plain = ltsva_batch(sts, None, None, 65.5 / FS, 0.5, alpha=0.5, rij=rij)
    assert len(plain[0]) == 8
    np.testing.assert_array_equal(plain[1][0], batch[1][0])


def test_several_estimators_each_with_its_own_elements_and_slowness():
    """Estimator 0 equals ``ltsva_beam``; the estimators without element k equal ``ltsva_beam`` on the reduced stream
    (k = 0 too: the delays are then relative to trace row 1)."""
    data, rij = _wave(5, 1201, mistimed=True)
    st = synthetic.make_stream(data, FS, starttime=T0)
    ests = [(0.5, ()), (1.0, (4,)), (0.75, (0,))]
    multi = ltsva_multi(st, None, None, 65.5 / FS, 0.5, ests, rij=rij, beam=True)
    for (alpha, remove), got in zip(ests, multi):
        kept = [i for i in range(5) if i not in remove]
        st_k = synthetic.make_stream(data[kept], FS, starttime=T0)
        exp = ltsva_beam(st_k, None, None, 65.5 / FS, 0.5, alpha=alpha, rij=np.ascontiguousarray(rij[:, kept]))
        _same_tuple(got, exp)
    assert not np.array_equal(multi[0][9], multi[1][9])
    assert len(ltsva_multi(st, None, None, 65.5 / FS, 0.5, ests, rij=rij)[0]) == 8


def test_two_window_slices_add_up_to_the_full_call():
    data, rij = _wave(4, 2401, mistimed=True)
    full = _process(data, rij, 65, 0.5)
    parts = [_process(data, rij, 65, 0.5, window_slice=(k, 2)) for k in range(2)]
    n = int(full.nwin[0])
    for k in ('beam_power', 'fstat'):
        a, b = getattr(parts[0], k), getattr(parts[1], k)
        assert not np.any((a != 0) & (b != 0))                     # rows outside a slice stay zero
        assert np.count_nonzero(a[0, :n]) == n // 2
        np.testing.assert_array_equal(a + b, getattr(full, k), err_msg=k)


def test_nan_sample_dead_channel_and_empty_window():
    W = 65
    data, rij = _wave(4, 2401)
    # (1) one NaN sample: NaN in exactly the windows the definition names (reads that touch it, or a slowness that is not
    #     finite), finite everywhere else
    bad = data.copy()
    bad[1, 1000] = np.nan
    res = _process(bad, rij, W, 1.0)
    ref, _ = _against_reference(res, bad, label='NaN sample')
    n = int(res.nwin[0])
    nan_ref = np.isnan(ref['beam_power'])
    assert 1 <= nan_ref.sum() <= 12
    keep = ~ref['skip']
    assert np.array_equal(np.isnan(res.beam_power[0, :n])[keep], nan_ref[keep])
    assert np.array_equal(np.isnan(res.fstat[0, :n])[keep], nan_ref[keep])
    # (2) a dead channel: finite values equal to the reference
    dead = data.copy()
    dead[2] = 0.0
    res = _process(dead, rij, W, 1.0)
    _against_reference(res, dead, label='dead channel')
    assert np.all(np.isfinite(res.beam_power[0, :n])) and np.all(np.isfinite(res.fstat[0, :n]))
    # (3) a stretch of zeros on every channel: the windows whose reads all fall into it have beam_power 0 and fstat NaN
    gap = data.copy()
    gap[:, 800:1400] = 0.0
    res = _process(gap, rij, W, 1.0)
    ref, _ = _against_reference(res, gap, label='empty windows')
    empty = (ref['S_t'] == 0) & ~ref['skip']
    assert empty.sum() >= 3
    assert np.all(res.beam_power[0, :n][empty] == 0.0) and np.all(np.isnan(res.fstat[0, :n][empty]))


def test_plan_without_beam_refuses_the_fetch_and_a_pass_without_solve_keeps_the_grids():
    data, rij = _wave(4, 1201)
    engine.process(data, FS, T0, rij, [(None, None)], [65.5 / FS], 0.5, 1.0, prefiltered=True)
    h = engine.get_handle()
    with pytest.raises(_hip.NblsError) as err:
        h.fetch_beam()
    assert err.value.code == _hip.NBLS_ERR_STATE
    res = _process(data, rij, 65, 1.0)
    h = res.handle
    before = h.fetch_beam()
    np.testing.assert_array_equal(before[1], res.fstat)
    h.execute(stages=3)                                          # filter and correlation only
    after = h.fetch_beam()
    np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(after[1], before[1])


def test_rccl_communicator_refuses_beam_at_plan_time():
    """A communicator lives as long as its process: a child process over the tests' loopback transport."""
    src = os.path.join(ROOT, 'tests', 'c_caller', 'loopback_rccl.cpp')
    lib = os.path.join(ROOT, 'tests', 'c_caller', 'libloopback_rccl.so')
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.run(['/opt/rocm/bin/hipcc', '-O2', '-shared', '-fPIC', '--offload-arch=gfx950', src, '-o', lib], check=True,
                       timeout=300)
    env = dict(os.environ, NBLS_TEST_TRANSPORT=lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_beam_comm_worker.py')], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and 'BEAM_COMM_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_c_caller_runs():
    from test_beam_host import build_beam_caller
    r = subprocess.run([build_beam_caller()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'BEAM_CALLER_OK' in r.stdout, r.stdout + r.stderr


def test_whole_call_on_the_example_parameters():
    """``narrow_band_least_squares_beam`` with example.py's parameters (8 bands 0.1-5 Hz, log, cheby1 order 2, adaptive
    windows 60 .. 30 s, half overlap) on a five-minute trace: the first nine returns are ``narrow_band_least_squares``'s,
    the two new arrays match the reference band by band."""
    N, npts, ALPHA = 8, 6001, 0.5
    rij0 = synthetic.array_geometry(N, 1.0)
    data = synthetic.plane_wave(rij0, npts, FS, 0.1, 5.0, timing_error_s=0.25, bad_element=N - 1, seed=930)
    rij = rij0 - rij0.mean(axis=1, keepdims=True)
    st = synthetic.make_stream(data, FS, starttime=T0)
    freqlist, NBANDS, _ = get_freqlist(0.1, 5.0, 'log', 8)
    WINLEN_list = get_winlenlist('adaptive', NBANDS, 50, 60, 30)
    fr = np.logspace(-2, 1, 32)
    args = (WINLEN_list, 0.5, ALPHA, st, None, None, NBANDS, np.zeros(32), np.zeros(32), freqlist, 'log', fr, 'cheby1', 2, 0.01)
    got = narrow_band_least_squares_beam(*args, rij=rij)
    exp = narrow_band_least_squares(*args, rij=rij)
    assert len(got) == 11 and len(exp) == 9
    for i in (0, 1, 2, 3, 5, 7, 8):
        np.testing.assert_array_equal(got[i], exp[i], err_msg='return %d' % i)
    assert got[6] == exp[6] and list(got[4].keys()) == list(exp[4].keys())
    power, fstat = got[9], got[10]
    assert power.shape == fstat.shape == got[0].shape
    # the slowness and the filtered bands of the same pass, through the engine
    edges = [(freqlist[b], freqlist[b + 1]) for b in range(NBANDS)]
    res = engine.process(data, FS, T0, rij, edges, list(WINLEN_list), 0.5, ALPHA, 'cheby1', 2, 0.01, vector_len=got[0].shape[1],
                         want_z=True, want_beam=True, groups=1)
    np.testing.assert_array_equal(res.vel, got[0])
    np.testing.assert_array_equal(res.beam_power, power)
    np.testing.assert_array_equal(res.fstat, fstat)
    for b in range(NBANDS):
        _against_reference(res, res.handle.fetch_filtered(b), band=b, label='band %d' % (b + 1))
