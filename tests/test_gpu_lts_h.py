"""Every FAST-LTS kernel at every subset size h it can be given (tests/lts_h_cases.py): the register-resident kernel of
4 ... 8 elements (``select_reg<PT, H>``: the pruned instance at h(0.5), ``<P, 0>`` at every other h, its sorting network
asked for every output from P / 2 to P - 2), the bucket kernel of 9 ... 32 (``bk_select`` for every rank of 36 pairs, and
h(0.5), h(0.5) + 1, h(0.75), the first h with ALPHA > 0.875, P - 2 and P - 1 at 66, 120, 253, 276 and 496 pairs) and the
lane-per-start kernel of option ``lts_impl = 1`` at all of them.

Per (N, h) two pre-filtered passes at ``alpha_of(P, h)``: the pulse tables of tests/solve_truth.py, whose mistimed rows
cross the exact-fit edge at h = C(N - b, 2), and the noisy windows, on which searching with a neighbouring h changes the
result (tests/test_lts_h_cases.py shows both on the CPU).  The fetched lags are the designed table / the oracle's
correlation; everything behind them is judged on the GPU's own lags with ``_check_against_oracle`` of
tests/test_gpu_solve.py, tolerances unchanged, weights exact.  Every window of both traces is compared; none is left out.

Comparisons between two GPU runs (kernel families, ``process_multi``, the streamed pass) are bit for bit."""
import functools

import numpy as np
import pytest

import lts_h_cases as lc
import solve_truth as st
from test_gpu_solve import GRIDS, PAD, T0, _check_against_oracle, _process
from narrow_band_least_squares_amd import engine, planner

pytestmark = pytest.mark.gpu

IDS = [lc.case_id(c) for c in lc.CASES]
FAMILY_FIELDS = ('z', 'weights', 'sigma_tau', 'vel', 'baz')
KW = dict(prefiltered=True, want_lag=True, want_cmax=True, want_z=True, want_uncert=True)


def _noisy(N, alpha, x=None, **kw):
    """One pre-filtered pass over the noisy trace (or ``x``, windows of the same length) -> (result, nwin)."""
    x = lc.noisy_trace(N) if x is None else x
    n = (x.shape[1] - 1) // st.W
    res = engine.process(x, st.FS, T0, st.grid_geometry(N), [(None, None)], [st.W / st.FS], 0.0, alpha, vector_len=n + PAD,
                         **dict(KW, **kw))
    assert int(res.nwin[0]) == n
    return res, n


def _passes(N, h):
    """Both passes of a case with whatever options the handle has -> dict(pulse=(res, n), noisy=(res, n)); the lags are
    checked in both."""
    P = lc.npairs(N)
    alpha = lc.alpha_of(P, h)
    assert planner.lts_h(P, alpha) == h
    pulse, n, _, _ = _process(N, alpha, lc.pulse_tables(N))                  # (asserts the designed lags)
    noisy, m = _noisy(N, alpha)
    np.testing.assert_array_equal(noisy.lag[0, :m], lc.noisy_lags(N), err_msg='CORRELATOR finding, not a solve finding: N=%d, '
                                  'the lags of the noisy windows are not the oracle\'s' % N)
    return dict(pulse=(pulse, n), noisy=(noisy, m))


@functools.lru_cache(maxsize=None)
def _default(N, h):
    """The passes of the default kernel of the size, run once per case and left unchanged."""
    return _passes(N, h)


def _worst(got, exp):
    with np.errstate(invalid='ignore', divide='ignore'):
        d = np.abs(got - exp) / np.abs(exp)
    d = d[np.isfinite(d)]
    return float(d.max()) if d.size else 0.0


@pytest.mark.parametrize('N,h', lc.CASES, ids=IDS)
def test_every_h_against_the_oracle(oracle, N, h):
    P = lc.npairs(N)
    alpha = lc.alpha_of(P, h)
    xij = planner.co_array(st.grid_geometry(N))[0]
    tabs = lc.pulse_tables(N)
    runs = _default(N, h)
    dropped = 0
    for kind, names in (('pulse', [t for t, _ in tabs]), ('noisy', ['noisy %d' % w for w in range(lc.noisy_windows(N))])):
        res, n = runs[kind]
        assert n == len(names)
        r = st.oracle_lts(oracle, res.lag[0, :n], xij, alpha)                # the GPU's own lags
        tag = 'LTS N=%d h=%d alpha=%.6f, %s' % (N, h, alpha, kind)
        print('%s: worst relative deviation from the oracle: z %.3g, sigma_tau %.3g (%d windows)' % (
            tag, _worst(res.z[0, :n], r['z'].T), _worst(res.sigma_tau[0, :n], r['sigma_tau']), n))
        for w in range(n):
            np.testing.assert_array_equal(res.weights[0, w], r['weights'][:, w],
                                          err_msg='SOLVE finding (%s): weights of window %d (%s)' % (tag, w, names[w]))
        _check_against_oracle(oracle, res, n, xij, r['z'], r['sigma_tau'], names, tag)
        dropped += int(np.sum(res.weights[0, :n] == 0))
        if kind != 'pulse':
            continue
        # the mistimed rows: exact fits exactly up to h = C(N - b, 2); there the kept pairs are the clean elements' and
        # sigma_tau (rounding residue of an exact fit, or NaN) is the oracle's to the bit
        paths, _ = st.classify(oracle, r['tau'], xij, alpha, r['zraw'])
        edge = 0
        for w, name in enumerate(names):
            b = lc.bad_elements(name)
            if b is None or 'mad_zero' in paths[w]:
                continue
            edge += 1
            assert ('exact_fit' in paths[w]) == lc.exact_fit_expected(N, b, h), (tag, name)
            if 'exact_fit' in paths[w]:
                np.testing.assert_array_equal(res.weights[0, w], lc.clean_pairs(N, b), err_msg='SOLVE finding (%s): %s' % (tag, name))
        assert edge >= 1
        exact = [w for w in range(n) if 'exact_fit' in paths[w]]
        assert exact
        np.testing.assert_array_equal(res.sigma_tau[0, exact], r['sigma_tau'][exact],
                                      err_msg='SOLVE finding (%s): sigma_tau of the exact-fit rows %s' % (tag, [names[w] for w in exact]))
    assert dropped > 0


def _with_option(option, N, h):
    hd = engine.get_handle()
    hd.set_option(option, 1)
    try:
        return _passes(N, h)
    finally:
        hd.set_option(option, 0)


def _same_bits(a, b, n, label):
    for k in FAMILY_FIELDS:
        x, y = np.ascontiguousarray(getattr(a, k)), np.ascontiguousarray(getattr(b, k))
        assert x.shape == y.shape and x.dtype == y.dtype, (label, k)
        np.testing.assert_array_equal(x, y, err_msg='%s: %s' % (label, k))
        assert x.tobytes() == y.tobytes(), '%s: %s has equal values in different bits' % (label, k)
    assert np.isfinite(a.z[0, :n]).any()


@pytest.mark.parametrize('N,h', lc.CASES, ids=IDS)
def test_kernel_families_agree(N, h):
    """The default kernel of the size against ``solve_lts_kernel`` with ``select_h`` (option ``lts_impl = 1``), and at h(0.5) of
    4 ... 8 elements against ``<P, 0>`` (option ``lts_generic_h = 1``), bit for bit on both traces."""
    base = _default(N, h)
    options = ['lts_impl'] + (['lts_generic_h'] if N <= 8 and h == st.half_h(lc.npairs(N)) else [])
    for option in options:
        other = _with_option(option, N, h)
        for kind in ('pulse', 'noisy'):
            _same_bits(base[kind][0], other[kind][0], base[kind][1], 'N=%d h=%d %s=1, %s' % (N, h, option, kind))
    pulse, n = base['pulse']
    assert np.isnan(pulse.z[0, :n]).any()                               # MAD(tau) = 0 windows were compared as well


@pytest.mark.parametrize('N', [8, 9])
def test_several_h_in_one_pass(N):
    """``engine.process_multi`` with h(0.5) + 1, a middle h and P - 1 on both traces: every estimator equals its own single
    call bit for bit (the comparison of tests/test_gpu_solve.py::test_several_estimators_in_one_pass)."""
    P = lc.npairs(N)
    hs = (st.half_h(P) + 1, (st.half_h(P) + P - 1) // 2, P - 1)
    assert all(h in lc.H_LIST[N] for h in hs) and len(set(hs)) == 3
    ests = engine.normalize_estimators([lc.alpha_of(P, h) for h in hs], N)
    rij = st.grid_geometry(N)
    differ = 0
    for kind, x in (('pulse', st.pulse_trace(lc.pulse_tables(N))), ('noisy', lc.noisy_trace(N))):
        n = (x.shape[1] - 1) // st.W
        multi = engine.process_multi(list(x), st.FS, [T0] * len(ests), [rij] * len(ests), [(None, None)], [st.W / st.FS], 0.0, ests,
                                     prefiltered=True, want_lag=True, want_cmax=True, want_uncert=True, vector_len=n + PAD)
        for res, h in zip(multi, hs):
            one, m = _default(N, h)[kind]
            tag = 'N=%d h=%d %s' % (N, h, kind)
            assert int(res.nwin[0]) == m == n
            np.testing.assert_array_equal(res.lag, one.lag, err_msg='CORRELATOR finding: lags, ' + tag)
            for name in ('vel', 'baz', 'sigma_tau', 't', 'mask', 'vel_uncert', 'baz_uncert', 'mdccm', 'weights'):
                a, b = np.ascontiguousarray(getattr(res, name)), np.ascontiguousarray(getattr(one, name))
                np.testing.assert_array_equal(a, b, err_msg='%s, %s' % (name, tag))
                assert a.tobytes() == b.tobytes(), '%s, %s: equal values in different bits' % (name, tag)
        differ += sum(not np.array_equal(multi[0].mask, r.mask) for r in multi[1:])
    assert differ >= 2                                                  # the estimators of one pass do not share a result


def test_streamed_pass_at_the_largest_h(monkeypatch):
    """9 elements at h = P - 1, the noisy windows 64 times over: with 1 MiB of quantised windows per batch the pass comes in
    several result batches (option settings of tests/test_gpu_band_batch.py::_streamed); equal to the pass in one piece."""
    N = 9
    P = lc.npairs(N)
    alpha = lc.alpha_of(P, P - 1)
    x = lc.noisy_trace(N)
    reps = 64
    long = np.ascontiguousarray(np.concatenate([x[:, :-1]] * reps + [x[:, -1:]], axis=1))
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    whole, n = _noisy(N, alpha, long)
    assert n == reps * lc.noisy_windows(N)
    hd = engine.get_handle()
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '1')
    try:
        hd.set_option('screen_batch_mb', 1)
        hd.set_option('solve_min_units', 1)
        streamed, _ = _noisy(N, alpha, long)
        nbatches = hd.result_batches()
    finally:
        hd.set_option('screen_batch_mb', 192)
        hd.set_option('solve_min_units', 0)
        monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    print('streamed: %d result batches for %d units' % (nbatches, n))
    assert nbatches >= 2
    for k in GRIDS + ('z', 'lag', 'cmax', 'mask', 'weights'):
        a, b = np.ascontiguousarray(getattr(streamed, k)), np.ascontiguousarray(getattr(whole, k))
        np.testing.assert_array_equal(a, b, err_msg='streamed: ' + k)
        assert a.tobytes() == b.tobytes(), 'streamed: %s has equal values in different bits' % k
    # ... and the long pass repeats the one of the sweep, window for window
    one, m = _default(N, P - 1)['noisy']
    for k in ('z', 'weights', 'sigma_tau', 'vel', 'baz'):
        np.testing.assert_array_equal(getattr(whole, k)[0, :n].reshape((reps, m) + getattr(one, k).shape[2:]),
                                      np.broadcast_to(getattr(one, k)[0, :m], (reps, m) + getattr(one, k).shape[2:]),
                                      err_msg='the repeated windows: ' + k)
    assert np.any(whole.weights[0, :n] == 0)
