"""Closure (consistency) of the picked lags (``nbls_set_closure``, csrc/closure.hip: closure_kernel)
against the truth of tests/closure_truth.py, always evaluated on the GPU's OWN fetched lags and fractions (the correlators
are pinned elsewhere).  Whole-sample form: exact integers, the float64 expression within 4 * 2^-52 relative, zero exactly
0.0.  Refined form: the long-double truth within its derived bound.  Between the forms of a pass (streamed, overlapped,
batched, window slices, several estimators) the results are equal bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import closure_truth as ct
import solve_truth as st
from narrow_band_least_squares_amd import (engine, planner, synthetic, _hip, ltsva, ltsva_subsample, ltsva_consistency,
                                           ltsva_multi, narrow_band_least_squares, narrow_band_least_squares_consistency,
                                           get_freqlist, get_winlenlist)

pytestmark = pytest.mark.gpu

FS = 20.0
T0 = 17884.0729166667
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAD = 3                                                          # cells beyond nwin, which must come back as zeros
REL = 4 * 2.0 ** -52
NAMES = ('consistency', 'closure_max', 'element_consistency')


def _noise(N, W=64, nwin=6, seed=0):
    """White noise: lag tables with no closure at all -> (data (N, nwin W + 1), centred rij)."""
    rij = synthetic.array_geometry(N, 1.0)
    data = np.random.default_rng(1700 + 100 * seed + N).standard_normal((N, nwin * W + 1))
    return data, rij - rij.mean(axis=1, keepdims=True)


def _wave(N, npts, seed=1800, mistimed=False):
    rij = synthetic.array_geometry(N, 1.0)
    data = synthetic.plane_wave(rij, npts, FS, 0.5, 4.0, baz_deg=60.0, snr_db=6.0, timing_error_s=0.25 if mistimed else 0.0,
                                bad_element=N - 1 if mistimed else None, seed=seed + N)
    return data, rij - rij.mean(axis=1, keepdims=True)


def _process(data, rij, W, alpha=1.0, overlap=0.0, refined=False, **kw):
    res = engine.process(data, FS, T0, rij, [(None, None)], [(W + 0.5) / FS], overlap, alpha, prefiltered=True, want_lag=True,
                         want_subsample=refined, want_consistency=True, **kw)
    assert int(res.W[0]) == W
    return res


def _check_whole_sample(res, band=0, label=''):
    """Every computed cell of the band against the exact integers of its own fetched lags; cells beyond nwin are zeros."""
    N, n = res.nchans, int(res.nwin[band])
    worst = 0.0
    for w in range(n):
        cons, cmax, el, Q = ct.outputs_int(res.lag[band, w], N, FS)
        assert Q < 2 ** 48                                         # (a Q off by one is 2^-48 relative: outside the tolerance)
        for name, got, exp in (('consistency', res.consistency[band, w], cons), ('closure_max', res.closure_max[band, w], cmax)):
            assert abs(got - exp) <= REL * exp, (label, name, w, got, exp)
            worst = max(worst, abs(got - exp) / exp if exp else 0.0)
        got = res.element_consistency[band, w]
        assert np.all(np.abs(got - el) <= REL * el), (label, w, got, el)
        assert np.all(got[el == 0.0] == 0.0)
    for name in NAMES:
        assert not getattr(res, name)[band, n:].any(), name
    return worst


def _check_refined(res, band=0, label=''):
    N, n, W = res.nchans, int(res.nwin[band]), int(res.W[band])
    worst = 0.0
    for w in range(n):
        ref = ct.outputs_refined(res.lag[band, w], res.lag_frac[band, w], N, FS, W)
        for name, got, exp, tol in (('consistency', res.consistency[band, w], ref['cons'], ref['tol_cons']),
                                    ('closure_max', res.closure_max[band, w], ref['cmax'], ref['tol_cmax'])):
            assert abs(got - exp) <= tol, (label, name, w, got, exp, tol)
            worst = max(worst, abs(got - exp) / tol)
        d = np.abs(res.element_consistency[band, w] - ref['el'])
        assert np.all(d <= ref['tol_el']), (label, w, d, ref['tol_el'])
        worst = max(worst, float(np.max(d / ref['tol_el'])))
    for name in NAMES:
        assert not getattr(res, name)[band, n:].any(), name
    return worst


def _same(got, exp, keys=NAMES + ('vel', 'lag')):
    for k in keys:
        np.testing.assert_array_equal(getattr(got, k), getattr(exp, k), err_msg=k)


@pytest.mark.parametrize('N', [3, 4, 8, 9, 12, 32])
def test_whole_sample_form_is_the_exact_integers(N):
    """White noise, W = 64, hop 64, 6 windows, OLS.  N where the loops change against the 64 lanes of a wave: 1, 4, 56, 84,
    220 and 4960 triplets; 3 .. 36 pairs (one trip, part of the lanes), 66 (a second trip of two lanes) and 496 pairs."""
    data, rij = _noise(N)
    res = _process(data, rij, 64, vector_len=6 + PAD)
    assert int(res.nwin[0]) == 6 and res.element_consistency.shape == (1, 6 + PAD, N)
    worst = _check_whole_sample(res, label='N=%d' % N)
    print('N=%d: %d triplets, consistency %s s, worst relative difference %.3g' % (N, ct.counts(N)[0], res.consistency[0, :6], worst))
    assert np.all(res.consistency[0, :6] > 0)                     # no closure at all: the sums are not trivially zero
    if N == 3:                                                    # one triplet: the three outputs are one number
        np.testing.assert_array_equal(res.consistency[0, :6], res.closure_max[0, :6])
        np.testing.assert_array_equal(res.element_consistency[0, :6, 1], res.closure_max[0, :6])


@pytest.mark.parametrize('N', [4, 8])
def test_designed_tables(N):
    """``solve_truth.tables`` through ``solve_truth.pulse_trace``: the exact-fit rows close exactly, the ``extreme`` row reaches
    lags of +-(W - 1), and on the ``off_closure`` row the largest closure is the miss of its one open pair."""
    tabs = st.tables(N)
    x, n = st.pulse_trace(tabs), len(tabs)
    res = engine.process(x, st.FS, T0, st.grid_geometry(N), [(None, None)], [st.W / st.FS], 0.0, 1.0, prefiltered=True,
                         want_lag=True, want_consistency=True, vector_len=n + PAD)
    assert int(res.nwin[0]) == n
    lag, _ = st.designed_lags(tabs)
    np.testing.assert_array_equal(res.lag[0, :n], lag, err_msg='CORRELATOR finding: the fetched lags are not the designed table')
    _check_whole_sample(res, label='tables N=%d' % N)
    seen = set()
    for w, (name, _) in enumerate(tabs):
        kind = name.split()[0]
        if kind in ('exact', 'one_bad', 'two_bad', 'one_bad_by_1', 'all_same', 'all_but_one_same', 'extreme', 'random') or \
                kind.endswith('_past_breakdown'):
            # single pulses: lag_ij = p_j - p_i, a table that closes whatever the element offsets
            assert res.consistency[0, w] == 0.0 and res.closure_max[0, w] == 0.0 and not res.element_consistency[0, w].any(), name
        if kind == 'extreme':
            assert np.abs(res.lag[0, w]).max() == st.W - 1
        if kind == 'off_closure':
            open_pairs = st.off_closure_pairs(res.lag[0, w], N)
            assert open_pairs is not None and len(open_pairs) == 1, name
            i, j = st.pair_table(N)[open_pairs[0]]
            m = next(m for m in range(N) if m not in (i, j))
            a, b, c = sorted((i, j, m))
            idx = ct.pair_index(N)
            miss = abs(int(res.lag[0, w, idx[(a, b)]]) + int(res.lag[0, w, idx[(b, c)]]) - int(res.lag[0, w, idx[(a, c)]]))
            assert miss == st.OFF_G
            assert res.closure_max[0, w] == np.float64(miss) / np.float64(st.FS), name
            assert res.consistency[0, w] > 0
        seen.add(kind)
    assert {'exact', 'extreme', 'off_closure'} <= seen


@pytest.mark.parametrize('W', [64, 257])
@pytest.mark.parametrize('N', [4, 9, 32])
def test_refined_form_within_the_derived_bound(N, W):
    """A plane wave at 6 dB with lag refinement: every output within ``tol`` of the long-double truth on the GPU's own lags
    and fractions."""
    data, rij = _wave(N, 6 * W + 1)
    res = _process(data, rij, W, refined=True, vector_len=6 + PAD)
    assert int(res.nwin[0]) == 6 and res.lag_frac is not None
    assert np.count_nonzero(res.lag_frac[0, :6]) > res.lag_frac[0, :6].size // 2
    worst = _check_refined(res, label='N=%d W=%d' % (N, W))
    print('N=%d W=%d: consistency %s s, worst |difference| / tol = %.3g' % (N, W, res.consistency[0, :6], worst))
    assert np.all(res.consistency[0, :6] > 0)


@pytest.mark.parametrize('N', [4, 8])
def test_refined_form_with_zero_fractions_is_the_whole_sample_form(N):
    """Unit pulses: R(l - 1) = R(l + 1) = 0 around every pick, every fraction is 0 and t = (double)lag exactly."""
    tabs = [t for t in st.tables(N) if not t[0].startswith('off_closure')] + \
        [('shuffled %d' % k, [[(int(p), 1.0)] for p in np.random.default_rng(40 + k).integers(0, st.W, size=N)]) for k in range(3)]
    x, n = st.pulse_trace(tabs), len(tabs)
    kw = dict(prefiltered=True, want_lag=True, want_consistency=True, vector_len=n + PAD)
    plain = engine.process(x, st.FS, T0, st.grid_geometry(N), [(None, None)], [st.W / st.FS], 0.0, 1.0, **kw)
    fine = engine.process(x, st.FS, T0, st.grid_geometry(N), [(None, None)], [st.W / st.FS], 0.0, 1.0, want_subsample=True, **kw)
    assert not fine.lag_frac.any()
    np.testing.assert_array_equal(fine.lag, plain.lag)
    for name in NAMES:
        a, b = getattr(fine, name), getattr(plain, name)
        assert np.all(np.abs(a - b) <= REL * np.abs(b)), name
        assert np.all(a[b == 0.0] == 0.0)


# ---- bit-equality across the forms of a pass -----------------------------------------------------------------------

@pytest.mark.parametrize('refined', [False, True])
def test_streamed_in_several_batches_and_overlapped_equal_the_single_pass(monkeypatch, refined):
    data, rij = _wave(9, 48001, mistimed=True)
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    whole = _process(data, rij, 1200, 0.5, overlap=0.75, refined=refined)
    h = engine.get_handle()
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '1')
    try:
        h.set_option('screen_batch_mb', 1)
        h.set_option('solve_min_units', 1)
        streamed = _process(data, rij, 1200, 0.5, overlap=0.75, refined=refined)
        assert h.result_batches() >= 3
        h.set_option('overlap', 1)                                # the per-batch chains on the second stream
        overlapped = _process(data, rij, 1200, 0.5, overlap=0.75, refined=refined)
        assert h.result_batches() >= 3
    finally:
        h.set_option('overlap', 0)
        h.set_option('screen_batch_mb', 192)
        h.set_option('solve_min_units', 0)
    for got in (streamed, overlapped):
        _same(got, whole)
    (_check_refined if refined else _check_whole_sample)(whole)
    assert whole.consistency[0, :int(whole.nwin[0])].any()


@pytest.mark.parametrize('refined', [False, True])
def test_batch_of_three_recordings_equals_three_single_passes(refined):
    recs = [_wave(5, 1201, seed=1900 + 10 * i) for i in range(3)]
    rij = recs[0][1]
    out = engine.process_batch([list(d) for d, _ in recs], FS, [T0 + i for i in range(3)], rij, [(None, None)], [65.5 / FS], 0.5,
                               1.0, prefiltered=True, want_subsample=refined, want_consistency=True)
    assert len(out) == 3
    for i, (got, (d, _)) in enumerate(zip(out, recs)):
        one = _process(d, rij, 65, overlap=0.5, refined=refined)
        _same(got, one, NAMES + ('vel',))
        (_check_refined if refined else _check_whole_sample)(one, label='recording %d' % i)
    assert not np.array_equal(out[0].consistency, out[1].consistency)


@pytest.mark.parametrize('refined', [False, True])
def test_two_window_slices_add_up_to_the_full_pass(refined):
    data, rij = _noise(4, 64, 37)
    full = _process(data, rij, 65, overlap=0.5, refined=refined)
    parts = [_process(data, rij, 65, overlap=0.5, refined=refined, window_slice=(k, 2)) for k in range(2)]
    n = int(full.nwin[0])
    for k in NAMES:
        a, b = getattr(parts[0], k), getattr(parts[1], k)
        assert not np.any((a != 0) & (b != 0))                     # cells outside a slice are zeros
        assert not a[0, n // 2:].any() and not b[0, :n // 2].any()
        np.testing.assert_array_equal(a + b, getattr(full, k), err_msg=k)
    assert np.count_nonzero(full.consistency[0, :n]) == n


@pytest.mark.parametrize('refined', [False, True])
def test_every_estimator_equals_a_separate_pass_on_its_sub_array(refined):
    """OLS and LTS at ALPHA = 0.5 on all 8 elements and without element 3: estimator e of the one pass against a pass of
    its own on the sub-array's rows, bit for bit; the sub-array's truth on ITS gathered lags."""
    N = 8
    data, rij = _wave(N, 1201, mistimed=True)
    ests = engine.normalize_estimators([1.0, 0.5, (1.0, (3,)), (0.5, (3,))], N)
    kept = [engine.kept_elements(N, rm) for _, rm in ests]
    rijs = [np.ascontiguousarray(rij[:, k]) for k in kept]
    multi = engine.process_multi(list(data), FS, [T0] * len(ests), rijs, [(None, None)], [65.5 / FS], 0.5, ests, prefiltered=True,
                                 want_lag=True, want_subsample=refined, want_consistency=True)
    for res, (alpha, remove), k, r in zip(multi, ests, kept, rijs):
        one = _process(np.ascontiguousarray(data[k]), r, 65, alpha, overlap=0.5, refined=refined)
        assert res.element_consistency.shape[2] == len(k)
        _same(res, one)
        (_check_refined if refined else _check_whole_sample)(res, label='alpha=%g remove=%s' % (alpha, remove))
    np.testing.assert_array_equal(multi[0].consistency, multi[1].consistency)       # the closure does not depend on the solve
    assert not np.array_equal(multi[0].consistency, multi[2].consistency)


# ---- combinations ----------------------------------------------------------------------------------------------------

def test_follows_the_bounded_and_the_seeded_picks():
    data, rij = _wave(6, 2401)
    plain = _process(data, rij, 130, overlap=0.5)
    bounded = _process(data, rij, 130, overlap=0.5, min_velocity=0.25)
    grid = planner.slowness_grid(4.0, 9)
    seeded = _process(data, rij, 130, overlap=0.5, slowness_grid=grid, seed_halfwidths=2)
    for res, label in ((plain, 'plain'), (bounded, 'bounded'), (seeded, 'seeded')):
        _check_whole_sample(res, label=label)
    fine = _process(data, rij, 130, overlap=0.5, refined=True, min_velocity=0.25)
    _check_refined(fine, label='bounded and refined')


# ---- stage and state semantics ---------------------------------------------------------------------------------------

def test_stage_and_state_semantics():
    data, rij = _noise(4, 64, 10)
    xij, pair_idx, xpinv = planner.co_array(rij)
    h = _hip.Handle()
    h.set_trace(data, FS)
    h.set_geometry(xij, pair_idx, xpinv)
    h.plan(None, False, None, None, [65], [32], 40)
    h.execute()
    never = h.fetch(want_lag=True)
    with pytest.raises(_hip.NblsError) as err:                    # the plan did not ask
        h.fetch_closure()
    assert err.value.code == _hip.NBLS_ERR_STATE
    with pytest.raises(_hip.NblsError) as err:
        h._chk(h.lib.nbls_est_fetch_closure(h._h, 0, None, None, None))
    assert err.value.code == _hip.NBLS_ERR_STATE
    h.set_closure(True)
    try:
        h.plan(None, False, None, None, [65], [32], 40)
    finally:
        h.set_closure(False)
    h.execute(stages=3)                                          # filter and correlation only: the grids are still zeros
    for a in h.fetch_closure():
        assert not a.any()
    h.execute()
    before = h.fetch_closure()
    n = int(h.fetch()['nwin'][0])
    assert np.all(before[0][0, :n] > 0) and not before[0][0, n:].any()
    h.execute(stages=3)                                          # ... and a later pass without the solve stage keeps them
    for a, b in zip(h.fetch_closure(), before):
        np.testing.assert_array_equal(a, b)
    # a plan made after nbls_set_closure(h, 0) is the plain pass again
    h.plan(None, False, None, None, [65], [32], 40)
    h.execute()
    again = h.fetch(want_lag=True)
    for k in ('vel', 'baz', 'mdccm', 'sigma_tau', 'lag'):
        np.testing.assert_array_equal(again[k], never[k], err_msg=k)
    with pytest.raises(_hip.NblsError) as err:
        h.fetch_closure()
    assert err.value.code == _hip.NBLS_ERR_STATE
    h.close()


def test_rccl_communicator_refuses_closure_at_plan_time():
    """A communicator lives as long as its process: a child process over the tests' loopback transport."""
    src = os.path.join(ROOT, 'tests', 'c_caller', 'loopback_rccl.cpp')
    lib = os.path.join(ROOT, 'tests', 'c_caller', 'libloopback_rccl.so')
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.run(['/opt/rocm/bin/hipcc', '-O2', '-shared', '-fPIC', '--offload-arch=gfx950', src, '-o', lib], check=True,
                       timeout=300)
    env = dict(os.environ, NBLS_TEST_TRANSPORT=lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_closure_comm_worker.py')], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and 'CLOSURE_COMM_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_c_caller_runs():
    from test_closure_host import build_closure_caller
    r = subprocess.run([build_closure_caller()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'CLOSURE_CALLER_OK' in r.stdout, r.stdout + r.stderr


# ---- the public calls -----------------------------------------------------------------------------------------------

def test_ltsva_consistency_and_ltsva_multi():
    N = 6
    data, rij = _wave(N, 1201, mistimed=True)
    stream = synthetic.make_stream(data, FS, starttime=T0)
    for alpha in (1.0, 0.5):
        got = ltsva_consistency(stream, None, None, 65.5 / FS, 0.5, alpha=alpha, rij=rij)
        exp = ltsva(stream, None, None, 65.5 / FS, 0.5, alpha=alpha, rij=rij)
        assert len(got) == 11 and len(exp) == 8
        for i in (0, 1, 2, 3, 5, 6, 7):
            np.testing.assert_array_equal(got[i], exp[i], err_msg='return %d' % i)
        assert list(got[4].keys()) == list(exp[4].keys())
        n = len(exp[0])
        assert got[8].shape == got[9].shape == (n,) and got[10].shape == (n, N)
        res = _process(data, rij, 65, alpha, overlap=0.5)
        np.testing.assert_array_equal(got[8], res.consistency[0, :n])
        np.testing.assert_array_equal(got[10], res.element_consistency[0, :n])
    fine = ltsva_consistency(stream, None, None, 65.5 / FS, 0.5, rij=rij, subsample=True)
    exp = ltsva_subsample(stream, None, None, 65.5 / FS, 0.5, rij=rij)
    for i in (0, 1, 2, 3, 5, 6, 7):
        np.testing.assert_array_equal(fine[i], exp[i], err_msg='return %d' % i)
    assert not np.array_equal(fine[8], got[8])
    ests = [(0.5, ()), (1.0, (5,)), (0.75, (0,))]
    multi = ltsva_multi(stream, None, None, 65.5 / FS, 0.5, ests, rij=rij, consistency=True)
    for (alpha, remove), m in zip(ests, multi):
        kept = [i for i in range(N) if i not in remove]
        st_k = synthetic.make_stream(data[kept], FS, starttime=T0)
        one = ltsva_consistency(st_k, None, None, 65.5 / FS, 0.5, alpha=alpha, rij=np.ascontiguousarray(rij[:, kept]))
        assert len(m) == len(one) == 11
        for i in (0, 1, 2, 3, 5, 6, 7, 8, 9, 10):
            np.testing.assert_array_equal(m[i], one[i], err_msg='return %d' % i)
    assert len(ltsva_multi(stream, None, None, 65.5 / FS, 0.5, ests, rij=rij)[0]) == 8
    single = ltsva_multi(stream, None, None, 65.5 / FS, 0.5, [1.0], rij=rij, consistency=True)     # one estimator IS the single call
    np.testing.assert_array_equal(single[0][8], ltsva_consistency(stream, None, None, 65.5 / FS, 0.5, rij=rij)[8])


def test_whole_call_on_the_example_parameters():
    """``narrow_band_least_squares_consistency`` with example.py's parameters (8 bands 0.1-5 Hz, log, cheby1 order 2, adaptive
    windows 60 .. 30 s, half overlap) on a five-minute trace: the first nine returns are ``narrow_band_least_squares``'s, the
    three new arrays are the truth on the lags of the same pass, band by band."""
    N, npts, ALPHA = 8, 6001, 0.5
    rij0 = synthetic.array_geometry(N, 1.0)
    data = synthetic.plane_wave(rij0, npts, FS, 0.1, 5.0, timing_error_s=0.25, bad_element=N - 1, seed=1930)
    rij = rij0 - rij0.mean(axis=1, keepdims=True)
    stream = synthetic.make_stream(data, FS, starttime=T0)
    freqlist, NBANDS, _ = get_freqlist(0.1, 5.0, 'log', 8)
    WINLEN_list = get_winlenlist('adaptive', NBANDS, 50, 60, 30)
    fr = np.logspace(-2, 1, 32)
    args = (WINLEN_list, 0.5, ALPHA, stream, None, None, NBANDS, np.zeros(32), np.zeros(32), freqlist, 'log', fr, 'cheby1', 2, 0.01)
    got = narrow_band_least_squares_consistency(*args, rij=rij)
    exp = narrow_band_least_squares(*args, rij=rij)
    assert len(got) == 12 and len(exp) == 9
    for i in (0, 1, 2, 3, 5, 7, 8):
        np.testing.assert_array_equal(got[i], exp[i], err_msg='return %d' % i)
    assert got[6] == exp[6] and list(got[4].keys()) == list(exp[4].keys())
    cons, cmax, el = got[9:]
    assert cons.shape == cmax.shape == got[0].shape and el.shape == got[0].shape + (N,)
    edges = [(freqlist[b], freqlist[b + 1]) for b in range(NBANDS)]
    res = engine.process(data, FS, T0, rij, edges, list(WINLEN_list), 0.5, ALPHA, 'cheby1', 2, 0.01, vector_len=got[0].shape[1],
                         want_lag=True, want_consistency=True, groups=1)
    np.testing.assert_array_equal(res.vel, got[0])
    for name, a in zip(NAMES, (cons, cmax, el)):
        np.testing.assert_array_equal(getattr(res, name), a, err_msg=name)
    for b in range(NBANDS):
        _check_whole_sample(res, band=b, label='band %d' % (b + 1))
