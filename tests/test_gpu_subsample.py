"""Sub-sample refinement of the picked lags (``nbls_set_lag_refinement``, csrc/refine.hip: refine_lag_kernel; DESIGN.md
section 13) on the GPU: the fractions against the long-double statement of tests/refine_truth.py on the GPU's own lags,
within its derived rounding bound; the solve on ``tau = (lag + frac) / fs`` against the oracle on the very same delays;
the pulse tables of tests/solve_truth.py, whose fractions are all zero and whose results must not move by a bit; and the
bit-for-bit equalities between the forms of a pass.  All passes are pre-filtered: the CPU holds the identical samples."""
import os
import subprocess
import sys

import numpy as np
import pytest

import refine_truth as rt
import solve_truth as st
from narrow_band_least_squares_amd import (engine, planner, synthetic, _hip, ltsva, ltsva_subsample, ltsva_batch,
                                           ltsva_multi, narrow_band_least_squares, narrow_band_least_squares_subsample,
                                           get_freqlist, get_winlenlist)

pytestmark = pytest.mark.gpu

FS = 20.0
T0 = 17884.0729166667
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# trace lengths are odd (the padded row length differs from npts); windows hop by half (a quarter at 1200 samples)
NPTS = {16: 601, 65: 1201, 257: 2401, 1200: 6001}


def _wave(N, W, npts=None, seed=None, mistimed=False, noise=0.05):
    """A band-limited plane wave (40 sinusoids, 0.4 .. 2 Hz) at fractional delays with 5 % incoherent noise; the array is
    scaled so that no delay exceeds a quarter of the window (17 samples at most); ``mistimed``: the last element 0.27 s
    late -> (data (N, npts), rij)."""
    data, rij, _ = rt.sinusoid_wave(N, NPTS[W] if npts is None else npts, FS, 700 + N + W if seed is None else seed,
                                    max_delay=min(17.0, W / 4.0), noise=noise, timing_error_s=0.27 if mistimed else 0.0)
    return data, rij


def _process(data, rij, W, alpha, overlap=None, subsample=True, **kw):
    overlap = (0.75 if W == 1200 else 0.5) if overlap is None else overlap
    res = engine.process(data, FS, T0, rij, [(None, None)], [(W + 0.5) / FS], overlap, alpha, prefiltered=True, want_lag=True,
                         want_z=True, want_subsample=subsample, **kw)
    assert int(res.W[0]) == W
    return res


def _reference(res, data, band=0):
    n, W, inc = int(res.nwin[band]), int(res.W[band]), int(res.inc[band])
    return rt.refine_windows(data, W, [w * inc for w in range(n)], [tuple(p) for p in res.pair_idx], res.lag[band, :n]), n


def _check_fractions(res, data, label, band=0):
    """Every pair of every window of the band (``data``: its samples) within the bound; none is skipped: first, on the
    reference alone, |D| >= 2^20 E."""
    ref, n = _reference(res, data, band)
    W = int(res.W[band])
    assert n >= 3 and np.all(np.abs(res.lag[band, :n]) < W - 1), '%s: a lag at the end of the range (choose another seed)' % label
    assert np.all(np.abs(ref['D']) >= 2.0 ** 20 * ref['E']), '%s: a pair without a clear maximum (choose another seed)' % label
    got = res.lag_frac[band, :n]
    err = np.abs(got - ref['frac'])
    print('%s: %d windows x %d pairs, worst |d frac| / bound = %.3g, |frac| median %.3g, max %.3g, min |D| / E = %.3g'
          % (label, n, got.shape[1], np.max(err / ref['bound']), np.median(np.abs(ref['frac'])), np.max(np.abs(ref['frac'])),
             np.min(np.abs(ref['D']) / ref['E'])))
    assert np.all(err <= ref['bound']), label
    assert np.all(np.abs(got) <= 0.5) and np.count_nonzero(got) >= got.size // 2
    assert not res.lag_frac[band, n:].any()                                       # cells beyond nwin are zeros
    return ref, n


@pytest.mark.parametrize('W', [16, 65, 257, 1200])
@pytest.mark.parametrize('N,alpha', [(3, 1.0), (4, 0.5), (9, 0.5)])
def test_fractions_match_the_reference(N, alpha, W):
    """Windows of 16 samples (below a wave), 65 (one past it), 257 (one past a 256-thread workgroup) and 1200 (cfg-3's);
    3 elements under OLS, 4 under the register LTS kernel, 9 under the bucket LTS kernel.  9 x 1200 samples (86 400 B) is
    past the kernel's LDS limit and takes its global-memory form, every other shape the LDS form; the two shapes right at
    the switch are ``test_fractions_on_either_side_of_the_lds_switch``."""
    data, rij = _wave(N, W)
    res = _process(data, rij, W, alpha)
    assert (_hip.refine_lds_bytes(N, W) == 0) == ((N, W) == (9, 1200))
    _check_fractions(res, data, 'N=%d W=%d' % (N, W))


LDS_LIMIT = 80 * 1024          # refine.hip: REFINE_LDS_MAX


def test_form_selector_switches_at_the_lds_limit():
    """``nbls_refine_lds_bytes``: nelem * W * 8 bytes up to 80 KiB, 0 (the global-memory form) beyond."""
    assert _hip.refine_lds_bytes(8, 1280) == LDS_LIMIT and _hip.refine_lds_bytes(8, 1281) == 0
    assert _hip.refine_lds_bytes(8, 1200) == 76800 and _hip.refine_lds_bytes(9, 1200) == 0
    assert _hip.refine_lds_bytes(3, 16) == 384 and _hip.refine_lds_bytes(32, 320) == LDS_LIMIT
    assert _hip.refine_lds_bytes(32, 321) == 0
    with pytest.raises(ValueError):
        _hip.refine_lds_bytes(0, 16)


@pytest.mark.parametrize('W', [1280, 1281])
def test_fractions_on_either_side_of_the_lds_switch(W):
    """8 elements x 1280 samples are exactly the 80 KiB the LDS form takes, 1281 samples the first shape of the
    global-memory form: both against the reference."""
    assert (_hip.refine_lds_bytes(8, W) > 0) == (W == 1280)
    data, rij, _ = rt.sinusoid_wave(8, 6401, FS, 741, max_delay=17.0, noise=0.05)
    res = _process(data, rij, W, 1.0, overlap=0.75)
    _check_fractions(res, data, 'N=8 W=%d' % W)


def test_the_two_forms_give_the_same_bits():
    """A 9 x 1200 pass runs the global-memory form, the 8 x 1200 call on the first eight of its elements the LDS form:
    the fractions of the 28 shared pairs are equal bit for bit — as a sub-array estimator of the 9-element pass, and as
    the rows of the full array's table."""
    data, rij = _wave(9, 1200)
    assert _hip.refine_lds_bytes(9, 1200) == 0 and _hip.refine_lds_bytes(8, 1200) > 0
    nine = _process(data, rij, 1200, 1.0)
    eight = _process(np.ascontiguousarray(data[:8]), np.ascontiguousarray(rij[:, :8]), 1200, 1.0)
    m = engine.kept_pair_map(9, (8,))
    np.testing.assert_array_equal(eight.lag, nine.lag[..., m])
    np.testing.assert_array_equal(eight.lag_frac, nine.lag_frac[..., m])
    assert np.count_nonzero(eight.lag_frac) > eight.lag_frac[0, :int(eight.nwin[0])].size // 2
    ests = engine.normalize_estimators([(1.0, ()), (1.0, (8,))], 9)
    rijs = [rij, np.ascontiguousarray(rij[:, :8])]
    multi = engine.process_multi(list(data), FS, [T0] * 2, rijs, [(None, None)], [1200.5 / FS], 0.75, ests, prefiltered=True,
                                 want_lag=True, want_subsample=True)
    np.testing.assert_array_equal(multi[1].lag_frac, eight.lag_frac)
    for k in ('vel', 'baz', 'sigma_tau'):
        np.testing.assert_array_equal(getattr(multi[1], k), getattr(eight, k), err_msg=k)


def test_fractions_behind_the_valu_correlator():
    data, rij = _wave(4, 65)
    h = engine.get_handle()
    h.set_profiling(True)
    try:
        res = _process(data, rij, 65, 1.0, xcorr_impl=1)
        assert h.timings()['xcorr_impl'] == 1
    finally:
        h.set_profiling(False)
    _check_fractions(res, data, 'VALU correlator')
    auto = _process(data, rij, 65, 1.0)
    np.testing.assert_array_equal(auto.lag, res.lag)
    np.testing.assert_array_equal(auto.lag_frac, res.lag_frac)                   # the fractions depend on (W, l) alone
    mfma = _process(data, rij, 65, 1.0, xcorr_impl=2)
    np.testing.assert_array_equal(mfma.lag_frac, res.lag_frac)


@pytest.mark.parametrize('N', [4, 8, 9])
@pytest.mark.parametrize('alpha', [0.5, 1.0])
def test_solve_on_the_gpus_own_refined_lags(oracle, N, alpha):
    """tau = (lag + frac) / fs formed in NumPy from the two fetched tables is what the solve kernels read: the oracle's
    ``ols_solve`` / ``fast_lts`` + ``lts_post_process`` on it give the weights and ``stdict`` exactly and z, vel, baz,
    sigma_tau within the tolerances of tests/test_gpu_solve.py."""
    W = 65
    data, rij = _wave(N, W, mistimed=True)
    res = _process(data, rij, W, alpha, want_uncert=True)
    n = int(res.nwin[0])
    xij, pairs, _ = planner.co_array(rij)
    tau = np.ascontiguousarray(((res.lag[0, :n].astype(np.float64) + res.lag_frac[0, :n]) / FS).T)
    assert np.any(tau * FS != np.rint(tau * FS))
    if alpha == 1.0:
        z_o, _, _, sig_o = oracle.ols_solve(xij, tau)
        w_o = np.ones((len(xij), n), dtype=np.uint8)
    else:
        z_o, w_o, sig_o = oracle.lts_post_process(tau, xij, oracle.fast_lts(tau, xij, alpha), alpha)
        assert np.any(w_o == 0), 'no window of the LTS case drops a pair'
        for w in range(n):
            np.testing.assert_array_equal(res.weights[0, w], w_o[:, w], err_msg='weights of window %d' % w)
    vel_o, baz_o = oracle.vel_baz(z_o)
    for what, got, exp in (('z', res.z[0, :n], z_o.T), ('sigma_tau', res.sigma_tau[0, :n], sig_o),
                           ('vel', res.vel[0, :n], vel_o), ('baz', res.baz[0, :n], baz_o)):
        np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg='NaN pattern of ' + what)
    np.testing.assert_allclose(res.z[0, :n], z_o.T, rtol=1e-9, atol=1e-14, equal_nan=True)
    np.testing.assert_allclose(res.vel[0, :n], vel_o, rtol=1e-9, equal_nan=True)
    np.testing.assert_allclose(res.baz[0, :n], baz_o, rtol=1e-9, equal_nan=True)
    np.testing.assert_allclose(res.sigma_tau[0, :n], sig_o, rtol=1e-7, atol=1e-12, equal_nan=True)
    # the public call: the same rows, and the dictionary of the oracle's weights under ltsva's own key text
    got = ltsva_subsample(synthetic.make_stream(data, FS, starttime=T0), None, None, (W + 0.5) / FS, 0.5, alpha=alpha, rij=rij)
    np.testing.assert_array_equal(got[0], res.vel[0, :n])
    np.testing.assert_array_equal(got[5], res.sigma_tau[0, :n])
    np.testing.assert_array_equal(got[6], res.vel_uncert[0, :n])
    if alpha == 1.0:
        assert got[4] == {}
    else:
        exp = oracle.stdict_from_weights(w_o, pairs, got[2], N)
        assert set(got[4].keys()) == set(exp.keys()) and got[4]['size'] == N
        for k, v in exp.items():
            np.testing.assert_array_equal(got[4][k], v, err_msg=k)
    # the same windows with whole-sample lags: MdCCM and the lags are those, the fit is not
    plain = _process(data, rij, W, alpha, subsample=False)
    assert plain.lag_frac is None
    np.testing.assert_array_equal(plain.lag, res.lag)
    np.testing.assert_array_equal(plain.mdccm, res.mdccm)
    assert not np.array_equal(plain.sigma_tau, res.sigma_tau)


@pytest.mark.parametrize('N,alpha', [(3, 1.0), (8, 0.5), (8, 0.75), (9, 0.5), (12, 1.0)])
def test_pulse_tables_have_zero_fractions_and_unchanged_results(N, alpha):
    """The tables of tests/test_gpu_solve.py (one unit pulse per channel; the +-(W - 1) rows of ``extreme`` included):
    every fraction is 0 and every result equals the pass without refinement bit for bit."""
    tabs = st.tables(N)
    names = [t for t, _ in tabs]
    assert 'extreme' in names
    x = st.pulse_trace(tabs)
    rij = st.grid_geometry(N)
    n = len(tabs)
    kw = dict(prefiltered=True, want_lag=True, want_cmax=True, want_z=True, want_uncert=True, vector_len=n + 3)
    run = lambda sub: engine.process(x, st.FS, T0, rij, [(None, None)], [st.W / st.FS], 0.0, alpha, want_subsample=sub, **kw)
    off, on = run(False), run(True)
    lag, _ = st.designed_lags(tabs)
    np.testing.assert_array_equal(on.lag[0, :n], lag)
    assert np.abs(lag[names.index('extreme')]).max() == st.W - 1
    assert on.lag_frac.shape == on.lag.shape and not on.lag_frac.any()
    assert not np.signbit(on.lag_frac).any()
    for k in ('vel', 'baz', 'mdccm', 'sigma_tau', 'vel_uncert', 'baz_uncert', 'z', 'lag', 'cmax', 'mask'):
        np.testing.assert_array_equal(getattr(on, k), getattr(off, k), err_msg=k)
    assert np.isfinite(on.z[0, :n]).any() and (alpha == 1.0 or np.isnan(on.z[0, :n]).any())   # (MAD(tau) = 0 rows: NaN under LTS)


def test_nan_sample_and_dead_channel_follow_the_contract():
    W = 65
    data, rij = _wave(4, W)
    bad = data.copy()
    bad[1, 700] = np.nan
    bad[2, 300:500] = 0.0                                          # windows in which channel 2 is dead
    res = _process(bad, rij, W, 1.0)
    ref, n = _reference(res, bad)
    touched = ~np.isfinite(ref['D']) | (ref['D'] >= 0)
    assert touched.sum() >= 6
    assert not res.lag_frac[0, :n][touched].any()
    ok = ~touched & (np.abs(ref['D']) >= 2.0 ** 20 * ref['E'])
    assert ok.sum() >= ok.size // 2
    assert np.all(np.abs(res.lag_frac[0, :n] - ref['frac'])[ok] <= ref['bound'][ok])
    plain = _process(bad, rij, W, 1.0, subsample=False)
    np.testing.assert_array_equal(np.isnan(plain.sigma_tau), np.isnan(res.sigma_tau))   # NaN windows keep today's behaviour
    np.testing.assert_array_equal(plain.lag, res.lag)


def test_streamed_in_several_batches_equals_the_unstreamed_pass(monkeypatch):
    data, rij = _wave(9, 1200, npts=48001, mistimed=True)
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    whole = _process(data, rij, 1200, 0.5)
    h = engine.get_handle()
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '1')
    try:
        h.set_option('screen_batch_mb', 1)
        h.set_option('solve_min_units', 1)
        streamed = _process(data, rij, 1200, 0.5)
        assert h.result_batches() >= 2
        h.set_option('overlap', 1)                                # the per-batch chains on the second stream
        overlapped = _process(data, rij, 1200, 0.5)
    finally:
        h.set_option('overlap', 0)
        h.set_option('screen_batch_mb', 192)
        h.set_option('solve_min_units', 0)
    for got in (streamed, overlapped):
        for k in ('vel', 'baz', 'sigma_tau', 'z', 'lag', 'lag_frac', 'mask'):
            np.testing.assert_array_equal(getattr(got, k), getattr(whole, k), err_msg=k)
    assert np.count_nonzero(whole.lag_frac) > whole.lag_frac[0, :int(whole.nwin[0])].size // 2


def _same_tuple(got, exp, n=8):
    assert len(got) == len(exp) == n
    for i in [i for i in range(n) if i != 4]:
        np.testing.assert_array_equal(got[i], exp[i], err_msg='return %d' % i)
    assert list(got[4].keys()) == list(exp[4].keys())
    for k in exp[4]:
        np.testing.assert_array_equal(got[4][k], exp[4][k], err_msg=k)


def test_batch_of_three_recordings_equals_three_single_calls():
    recs = [_wave(4, 65, seed=810 + i, mistimed=True) for i in range(3)]
    rij = recs[0][1]
    sts = [synthetic.make_stream(d, FS, starttime=T0 + i) for i, (d, _) in enumerate(recs)]
    batch = ltsva_batch(sts, None, None, 65.5 / FS, 0.5, alpha=0.5, rij=rij, subsample=True)
    assert len(batch) == 3
    for got, s in zip(batch, sts):
        _same_tuple(got, ltsva_subsample(s, None, None, 65.5 / FS, 0.5, alpha=0.5, rij=rij))
    plain = ltsva_batch(sts, None, None, 65.5 / FS, 0.5, alpha=0.5, rij=rij)
    np.testing.assert_array_equal(plain[1][3], batch[1][3])                     # MdCCM is unchanged
    assert not np.array_equal(plain[1][5], batch[1][5])                         # sigma_tau is not
    _same_tuple(plain[1], ltsva(sts[1], None, None, 65.5 / FS, 0.5, alpha=0.5, rij=rij))


def test_sub_array_estimator_equals_the_call_on_the_sub_array():
    data, rij = _wave(5, 65, mistimed=True)
    s = synthetic.make_stream(data, FS, starttime=T0)
    ests = [(0.5, ()), (1.0, (4,)), (0.75, (0,))]
    multi = ltsva_multi(s, None, None, 65.5 / FS, 0.5, ests, rij=rij, subsample=True)
    for (alpha, remove), got in zip(ests, multi):
        kept = [i for i in range(5) if i not in remove]
        s_k = synthetic.make_stream(data[kept], FS, starttime=T0)
        exp = ltsva_subsample(s_k, None, None, 65.5 / FS, 0.5, alpha=alpha, rij=np.ascontiguousarray(rij[:, kept]))
        assert len(got) == 8
        for i in (0, 1, 2, 5, 6, 7):
            np.testing.assert_array_equal(got[i], exp[i], err_msg='return %d, remove %s' % (i, remove))
        np.testing.assert_allclose(got[3], exp[3], rtol=0, atol=1e-12)          # (MdCCM of a subset: tests/test_gpu_multi.py)
        assert list(got[4].keys()) == list(exp[4].keys())
    # the compact fraction rows of a sub-array are the full array's rows of its pairs
    ests_n = engine.normalize_estimators(ests, 5)
    rijs = [np.ascontiguousarray(rij[:, engine.kept_elements(5, rm)]) for _, rm in ests_n]
    res = engine.process_multi(list(data), FS, [T0] * 3, rijs, [(None, None)], [65.5 / FS], 0.5, ests_n, prefiltered=True,
                               want_lag=True, want_subsample=True)
    assert np.count_nonzero(res[0].lag_frac) > 0
    for r, (_, rm) in zip(res[1:], ests_n[1:]):
        m = engine.kept_pair_map(5, rm)
        np.testing.assert_array_equal(r.lag_frac, res[0].lag_frac[..., m])
        np.testing.assert_array_equal(r.lag, res[0].lag[..., m])


def test_two_window_slices_add_up_to_the_full_call():
    data, rij = _wave(4, 65, npts=2401, mistimed=True)
    full = _process(data, rij, 65, 0.5)
    parts = [_process(data, rij, 65, 0.5, window_slice=(k, 2)) for k in range(2)]
    n = int(full.nwin[0])
    for k in ('lag_frac', 'sigma_tau', 'vel'):
        a, b = getattr(parts[0], k), getattr(parts[1], k)
        assert not np.any((a != 0) & (b != 0))                     # rows outside a slice stay zero
        np.testing.assert_array_equal(a + b, getattr(full, k), err_msg=k)
    assert np.count_nonzero(parts[0].sigma_tau[0, :n]) == n // 2


def test_beam_follows_the_refined_slowness():
    """beam and refinement in one pass (a batch of one IS the single call): the first eight returns are
    ``ltsva_subsample``'s, the beam's delays are those of the refined z (tests/beam_truth.py)."""
    import beam_truth as bt
    data, rij = _wave(4, 65, mistimed=True)
    s = synthetic.make_stream(data, FS, starttime=T0)
    both = ltsva_batch([s], None, None, 65.5 / FS, 0.5, alpha=0.5, rij=rij, beam=True, subsample=True)[0]
    assert len(both) == 10
    _same_tuple(both[:8], ltsva_subsample(s, None, None, 65.5 / FS, 0.5, alpha=0.5, rij=rij))
    res = engine.process(data, FS, T0, rij, [(None, None)], [65.5 / FS], 0.5, 0.5, prefiltered=True, want_z=True, want_beam=True,
                         want_subsample=True)
    n = int(res.nwin[0])
    np.testing.assert_array_equal(res.beam_power[0, :n], both[8])
    np.testing.assert_array_equal(res.fstat[0, :n], both[9])
    ref = bt.beam_reference(data, FS, res.xij, res.z[0], 65, int(res.inc[0]), n)
    on_f, skipped = bt.compare(res.beam_power[0, :n], res.fstat[0, :n], ref)
    assert on_f >= n // 2


def test_plan_without_refinement_refuses_the_fetch_and_a_solve_only_pass_keeps_the_fractions():
    data, rij = _wave(4, 65)
    engine.process(data, FS, T0, rij, [(None, None)], [65.5 / FS], 0.5, 1.0, prefiltered=True)
    h = engine.get_handle()
    with pytest.raises(_hip.NblsError) as err:
        h.fetch_lag_fraction()
    assert err.value.code == _hip.NBLS_ERR_STATE
    out = np.empty((1, h.vector_len, 6))
    dp = out.ctypes.data_as(_hip.C.POINTER(_hip.C.c_double))
    assert h.lib.nbls_est_fetch_lag_fraction(h._h, 0, dp) == _hip.NBLS_ERR_STATE
    res = _process(data, rij, 65, 1.0)
    h = res.handle
    before = h.fetch_lag_fraction()
    np.testing.assert_array_equal(before, res.lag_frac)
    assert np.count_nonzero(before) > 0
    h.execute(stages=4)                                          # the solve alone: on the lags and fractions that are there
    after = h.fetch_lag_fraction()
    np.testing.assert_array_equal(after, before)
    again = h.fetch(want_z=True)
    np.testing.assert_array_equal(again['sigma_tau'], res.sigma_tau)
    np.testing.assert_array_equal(again['z'], res.z)


def test_rccl_communicator_accepts_the_plan_and_gathers_the_refined_block():
    """A communicator lives as long as its process: a child process over the tests' loopback transport."""
    src = os.path.join(ROOT, 'tests', 'c_caller', 'loopback_rccl.cpp')
    lib = os.path.join(ROOT, 'tests', 'c_caller', 'libloopback_rccl.so')
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.run(['/opt/rocm/bin/hipcc', '-O2', '-shared', '-fPIC', '--offload-arch=gfx950', src, '-o', lib], check=True,
                       timeout=300)
    env = dict(os.environ, NBLS_TEST_TRANSPORT=lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_subsample_comm_worker.py')], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and 'SUBSAMPLE_COMM_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_whole_call_on_the_example_parameters():
    """``narrow_band_least_squares_subsample`` with example.py's parameters (8 bands 0.1-5 Hz, log, cheby1 order 2,
    adaptive windows 60 .. 30 s, half overlap) on a five-minute trace: ``t`` and the window counts are those of
    ``narrow_band_least_squares``, every sigma_tau is finite where the whole-sample call's is."""
    N, npts, ALPHA = 8, 6001, 1.0
    rij0 = synthetic.array_geometry(N, 1.0)
    data = synthetic.plane_wave(rij0, npts, FS, 0.1, 5.0, seed=930)
    rij = rij0 - rij0.mean(axis=1, keepdims=True)
    s = synthetic.make_stream(data, FS, starttime=T0)
    freqlist, NBANDS, _ = get_freqlist(0.1, 5.0, 'log', 8)
    WINLEN_list = get_winlenlist('adaptive', NBANDS, 50, 60, 30)
    fr = np.logspace(-2, 1, 32)
    args = (WINLEN_list, 0.5, ALPHA, s, None, None, NBANDS, np.zeros(32), np.zeros(32), freqlist, 'log', fr, 'cheby1', 2, 0.01)
    got = narrow_band_least_squares_subsample(*args, rij=rij)
    exp = narrow_band_least_squares(*args, rij=rij)
    assert len(got) == len(exp) == 9
    np.testing.assert_array_equal(got[3], exp[3], err_msg='t')
    np.testing.assert_array_equal(got[6], exp[6], err_msg='num_compute_list')
    np.testing.assert_array_equal(got[2], exp[2], err_msg='mdccm')
    assert got[5].shape == exp[5].shape and np.all(np.isfinite(got[5][np.isfinite(exp[5])]))
    assert not np.array_equal(got[5], exp[5])
    computed = exp[5] > 0
    print('median sigma_tau: whole-sample lags %.4g s, refined %.4g s' % (np.median(exp[5][computed]), np.median(got[5][computed])))
