"""tests/solve_truth.py checked on the CPU: the pulse traces correlate to the designed lag tables through the oracle's
own correlator, the tables reach the paths of the oracle's LTS they were built for — for every (N, ALPHA) that
tests/test_gpu_solve.py runs, asserted, never skipped — and the exact-rational OLS truth agrees with the oracle within
the derived rounding bounds."""
import collections
import re
from fractions import Fraction

import numpy as np
import pytest

import solve_truth as st
from narrow_band_least_squares_amd import planner

ALL_N = sorted({n for n, _ in st.LTS_CASES} | set(st.OLS_N))


def _xij(N):
    return planner.co_array(st.grid_geometry(N))


@pytest.mark.parametrize('N', ALL_N)
def test_pulse_traces_correlate_to_the_designed_lags(oracle, N):
    """Geometry on the 0.25 km grid; hop = W = 64 at 20 Hz; the oracle's correlator on the pulse trace gives exactly the
    designed lags, cmax 1 or the three values of the two-pulse rows."""
    rij = st.grid_geometry(N)
    assert np.array_equal(rij / st.DX_KM, np.rint(rij / st.DX_KM))
    tabs = st.tables(N, slowness=st.SLOWNESS, nrandom=4, short=False)
    assert [n for n, _ in tabs if n.startswith('random')] == ['random %d' % k for k in range(4)]
    x = st.pulse_trace(tabs)
    nwin = len(tabs)
    assert x.shape == (N, nwin * st.W + 1)
    assert planner.window_plan(x.shape[1], st.FS, st.W / st.FS, 0.0) == (st.W, st.W, nwin)
    lag, cmax = st.designed_lags(tabs)
    tau, _, cmax_o = oracle.correlate_windows(x.T, st.W, np.arange(nwin) * st.W, st.pair_table(N), st.FS)
    np.testing.assert_array_equal(np.rint(tau.T * st.FS).astype(np.int64), lag)
    np.testing.assert_array_equal(tau.T, lag / st.FS)
    np.testing.assert_allclose(cmax_o.T, cmax, rtol=4e-16, atol=0)
    names = [n for n, _ in tabs]
    single = [w for w, n in enumerate(names) if not n.startswith('off_closure')]
    assert np.all(cmax_o.T[single] == 1.0)
    for w in set(range(nwin)) - set(single):
        vals = sorted(set(np.round(cmax_o[:, w], 4)))
        assert vals == ([0.7809, 0.9756, 1.0] if N > 3 else [0.7809, 0.9756]), (names[w], vals)
    # integer-delay plane waves: fs x_ij . z is the designed lag, exactly in integers
    q = st.grid_units(N)
    for s in st.SLOWNESS:
        w = names.index('exact z(%d,%d)' % s)
        d = q[:, 0] * s[0] + q[:, 1] * s[1]
        np.testing.assert_array_equal(lag[w], [d[i] - d[j] for i, j in st.pair_table(N)])
    np.testing.assert_array_equal(lag[names.index('all_same')], 0)
    assert np.abs(lag[names.index('extreme')]).max() == st.W - 1


def test_mistimed_rows_are_named_by_the_breakdown_point():
    """C(N - b, 2) >= h(0.5) for one mistimed element from 5 elements on and for two from 8 on (15 = 15: the edge)."""
    assert [st.half_h(n * (n - 1) // 2) for n in (4, 5, 6, 7, 8, 9)] == [4, 6, 9, 12, 15, 19]
    assert [planner.lts_h(p, 0.5) for p in (6, 10, 15, 21, 28, 36, 496)] == [st.half_h(p) for p in (6, 10, 15, 21, 28, 36, 496)]
    assert [n for n in range(4, 33) if st.within_breakdown(n, 1)] == list(range(5, 33))
    assert [n for n in range(4, 33) if st.within_breakdown(n, 2)] == list(range(8, 33))
    for n, _ in st.LTS_CASES:
        names = [t for t, _ in st.tables(n)]
        assert any(t.startswith('one_bad z') for t in names) == (n >= 5) or n >= 32
        assert any(t.startswith('two_bad z') for t in names) == (n >= 8)
        assert any(t.startswith('two_bad_past_breakdown') for t in names) == (n < 8)


@pytest.mark.parametrize('N,alpha', st.LTS_CASES)
def test_tables_reach_the_paths_they_were_built_for(oracle, N, alpha):
    """The reach conditions of every LTS case of tests/test_gpu_solve.py, on the oracle alone."""
    tabs = st.tables(N)
    names = [n for n, _ in tabs]
    xij, _, _ = _xij(N)
    planner.lts_plan(xij, alpha)                               # the planner's co-array MAD is non-zero on both axes
    lag, _ = st.designed_lags(tabs)
    r = st.oracle_lts(oracle, lag, xij, alpha)
    paths, w = st.classify(oracle, r['tau'], xij, alpha, r['zraw'])
    np.testing.assert_array_equal(w, r['weights'])             # the restatement IS the oracle's post-processing
    count = collections.Counter(t for p in paths for t in p)
    print('N=%d alpha=%g h=%d of %d pairs, %d windows: %s' % (N, alpha, planner.lts_h(len(xij), alpha), len(xij), len(tabs),
                                                             dict(sorted(count.items()))))
    by = dict(zip(names, paths))
    for name, p in by.items():
        kind, _, tag = name.partition(' ')
        plane = tag.startswith('z(') and tag != 'z(0,0)'
        if alpha == 0.5 and plane and kind in ('exact', 'one_bad', 'two_bad'):
            assert 'exact_fit' in p, name
        if alpha == 0.5 and kind.endswith('_past_breakdown'):
            assert 'exact_fit' not in p, name
        if name in ('all_same', 'exact z(0,0)') or (name == 'all_but_one_same' and N >= 5):
            assert p == {'mad_zero'}, name
            assert np.isnan(r['z'][:, names.index(name)]).all() and np.all(r['weights'][:, names.index(name)] == 1)
        if kind == 'off_closure_on_plane':
            assert {'exact_fit', 'dropped'} <= p and int(np.sum(r['weights'][:, names.index(name)] == 0)) == 1, name
    for kind in ('exact z', 'two_bad', 'all_same', 'all_but_one_same', 'extreme', 'off_closure ('):
        assert any(n.startswith(kind) for n in names), kind
    assert N >= 32 or all(any(n.startswith(kind) for n in names) for kind in ('one_bad', 'one_bad_by_1', 'random', 'off_closure_on_plane'))
    assert np.abs(lag[names.index('extreme')]).max() == st.W - 1
    assert count['tie_across_h'] >= 1
    assert count['dropped'] >= 1
    assert count['mad_zero'] >= 1
    # one pair off closure in each two-pulse row, none anywhere else
    for wdx, name in enumerate(names):
        off = st.off_closure_pairs(lag[wdx], N)
        if name.startswith('off_closure'):
            a, c = [int(v) for v in re.findall(r'\d+', name.split(' ')[1])]
            assert off == [st.pair_table(N).index((min(a, c), max(a, c)))], name
        else:
            assert off == [], name
    # neither of these is reached by a pulse table
    assert count['rew_scale_zero'] == 0 and count['few_kept'] == 0


def test_tied_windows_hang_on_the_index_order(oracle):
    """In the windows marked ``tie_across_h`` the h-subset really depends on the rule for equal |r|: taking the tied pairs
    in descending instead of ascending index order selects another subset."""
    N, alpha = 8, 0.5
    tabs = st.tables(N)
    xij, _, _ = _xij(N)
    lag, _ = st.designed_lags(tabs)
    r = st.oracle_lts(oracle, lag, xij, alpha)
    paths, _ = st.classify(oracle, r['tau'], xij, alpha, r['zraw'])
    tied = [w for w, p in enumerate(paths) if 'tie_across_h' in p]
    assert tied
    h = planner.lts_h(len(xij), alpha)
    differ = 0
    for w in tied:
        z0, z1 = r['zraw'][:, w]
        ar = np.abs((r['tau'][:, w] - xij[:, 0] * z0) - xij[:, 1] * z1)
        first = np.argsort(ar, kind='stable')[:h]
        last = ((len(ar) - 1) - np.argsort(ar[::-1], kind='stable'))[:h]
        differ += set(first) != set(last)
    assert differ >= 1


@pytest.mark.parametrize('N', st.OLS_N)
def test_exact_ols_truth_against_the_oracle(oracle, N):
    xij, _, xpinv = _xij(N)
    P = len(xij)
    tabs = st.tables(N, slowness=st.SLOWNESS, nrandom=4, short=False)
    lag, _ = st.designed_lags(tabs)
    z_o, vel_o, _, sig_o = oracle.ols_solve(xij, np.ascontiguousarray(lag.T / st.FS))
    nan = 0
    for w, (name, _) in enumerate(tabs):
        t = st.ols_truth(xij, xpinv, lag[w])
        np.testing.assert_array_equal(t['tau'], lag[w] / st.FS)
        for c in range(2):
            assert abs(Fraction(float(z_o[c, w])) - t['z'][c]) <= t['z_bound'][c], (name, c)
        acc, e_acc, e_sig = st.ols_acc(xij, t['tau'], z_o[:, w])
        if np.isnan(sig_o[w]):
            nan += 1
            assert acc <= e_acc, (name, float(acc), float(e_acc))          # negative by rounding only
        else:
            assert abs(Fraction(float(sig_o[w])) ** 2 * (P - 2) - acc) <= e_sig, (name, float(acc), float(e_sig))
        if name in ('all_same', 'exact z(0,0)'):
            assert sig_o[w] == 0.0 and np.isinf(vel_o[w]) and not z_o[:, w].any()
    print('N=%d: %d of %d windows with sigma_tau NaN under OLS' % (N, nan, len(tabs)))
