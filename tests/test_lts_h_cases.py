"""tests/lts_h_cases.py checked on the CPU, by the oracle alone: the conditions under which the cases of
tests/test_gpu_lts_h.py can tell a kernel that selects rank h from one that selects rank h - 1 or h + 1.

* ``alpha_of`` maps back to h through the planner and the oracle; the planner's scale factors at that ALPHA are the
  oracle's (both branches of ``_cnp2``).
* The ``one_bad`` / ``two_bad`` pulse rows are exact fits exactly up to h = C(N - b, 2).
* The noisy windows do not close and hold gross outliers; none has a confidence ellipse that the oracle's 20 000-point
  sampling cannot resolve to the GPU checker's tolerance.
* Discrimination: the oracle mutant that SEARCHES with h - 1 or h + 1 (``oracle.fast_lts``) and post-processes with h
  changes the final weights or the bits of z in at least two of the 40 noisy windows, for every h of 4 ... 9 elements
  and both neighbours.  From 12 elements on (8 or 3 windows) the minimum is one window; a case below it is printed as
  ``NOT DISCRIMINATED`` (the pulse rows and the other h of that size still cover the kernel there).  The counts are
  printed per (N, h)."""
import collections

import numpy as np
import pytest

import lts_h_cases as lc
import solve_truth as st
from narrow_band_least_squares_amd import planner


def _xij(N):
    return planner.co_array(st.grid_geometry(N))[0]


@pytest.mark.parametrize('N', lc.ALL_N)
def test_alpha_of_maps_back_to_h(oracle, N):
    P = lc.npairs(N)
    hs = lc.h_range(N)
    assert hs[0] == planner.lts_h(P, 0.5) == st.half_h(P) and hs[-1] == P - 1
    for h in hs:
        a = lc.alpha_of(P, h)
        assert 0.5 <= a < 1.0, (N, h, a)
        assert planner.lts_h(P, a) == h and oracle.lts_h(P, a) == h, (N, h, a)


def test_h_lists():
    assert [len(lc.H_LIST[N]) for N in lc.SMALL_N] == [2, 4, 6, 9, 13, 17]
    assert sum(len(lc.H_LIST[N]) for N in lc.SMALL_N) == 51
    for N in lc.ALL_N:
        P = lc.npairs(N)
        hl = lc.H_LIST[N]
        assert list(hl) == sorted(set(hl)) and set(hl) <= set(lc.h_range(N))
        assert st.half_h(P) in hl and P - 1 in hl
        # both branches of ``_cnp2``.  With 6 pairs h = 5 belongs to ALPHA in [0.75, 1): its midpoint IS 0.875, the last
        # value of the first branch (the two branches meet there), so 4 elements cannot reach the second one through
        # ``alpha_of``; every other size does
        assert any(lc.alpha_of(P, h) <= 0.875 for h in hl)
        assert any(lc.alpha_of(P, h) > 0.875 for h in hl) or (N == 4 and lc.alpha_of(P, P - 1) == 0.875)
        if N in lc.SMALL_N:
            assert list(hl) == lc.h_range(N)
        else:
            above = min(h for h in lc.h_range(N) if lc.alpha_of(P, h) > 0.875)
            assert lc.alpha_of(P, above - 1) <= 0.875
            assert list(hl) == sorted({st.half_h(P), st.half_h(P) + 1, planner.lts_h(P, 0.75), above, P - 2, P - 1}) and len(hl) == 6
    assert lc.H_LIST[8] == tuple(range(15, 28)) and lc.H_LIST[9] == tuple(range(19, 36))
    assert lc.H_LIST[32][0] == 249 and lc.H_LIST[32][-1] == 495
    assert len(lc.CASES) == 51 + 5 * 6 and len({lc.case_id(c) for c in lc.CASES}) == len(lc.CASES)


@pytest.mark.parametrize('N,h', lc.CASES, ids=[lc.case_id(c) for c in lc.CASES])
def test_plan_factors_match_the_oracle(oracle, N, h):
    """As tests/test_host.py::test_lts_plan_matches_oracle_constants, at the ALPHA of every case."""
    P = lc.npairs(N)
    a = lc.alpha_of(P, h)
    ho, raw_o, rew_o = oracle.lts_scale_tables(P, a)
    raw, rew = planner._lts_factors(P, a)
    assert ho == h and raw == raw_o
    np.testing.assert_array_equal(rew, rew_o)
    lp = planner.lts_plan(_xij(N), a)
    assert lp['h'] == h and lp['raw_factor'] == raw_o
    np.testing.assert_array_equal(lp['rew_table'], rew_o)


def test_exact_fit_edges():
    """8 elements: one mistimed element is an exact fit up to h = 21, two up to h = 15 = h(0.5), the breakdown edge."""
    assert [h for h in lc.H_LIST[8] if lc.exact_fit_expected(8, 1, h)] == list(range(15, 22))
    assert [h for h in lc.H_LIST[8] if lc.exact_fit_expected(8, 2, h)] == [15]
    for N in lc.ALL_N:
        for b in (1, 2):
            assert lc.exact_fit_expected(N, b, st.half_h(lc.npairs(N))) == st.within_breakdown(N, b)
            assert not lc.exact_fit_expected(N, b, lc.npairs(N) - 1)          # P - 1 > C(N - 1, 2) from 3 elements on
    assert lc.bad_elements('one_bad z(1,2)') == 1 and lc.bad_elements('two_bad_past_breakdown z(0,0)') == 2
    assert lc.bad_elements('one_bad_by_1 z(1,2)') is None and lc.bad_elements('exact z(1,2)') is None


@pytest.mark.parametrize('N,h', lc.CASES, ids=[lc.case_id(c) for c in lc.CASES])
def test_mistimed_rows_cross_the_exact_fit_edge(oracle, N, h):
    """``solve_truth.classify`` on the pulse tables at every h: a ``one_bad`` / ``two_bad`` row is on the oracle's exact-fit
    path exactly where C(N - b, 2) >= h, and keeps exactly the pairs of the clean elements there."""
    tabs = lc.pulse_tables(N)
    xij = _xij(N)
    a = lc.alpha_of(lc.npairs(N), h)
    lag, _ = st.designed_lags(tabs)
    r = st.oracle_lts(oracle, lag, xij, a)
    paths, w = st.classify(oracle, r['tau'], xij, a, r['zraw'])
    np.testing.assert_array_equal(w, r['weights'])
    seen = collections.Counter()
    for wdx, (name, _) in enumerate(tabs):
        b = lc.bad_elements(name)
        if b is None or 'mad_zero' in paths[wdx]:
            continue
        exp = lc.exact_fit_expected(N, b, h)
        assert ('exact_fit' in paths[wdx]) == exp, (N, h, name, sorted(paths[wdx]))
        seen[(b, exp)] += 1
        if exp:
            np.testing.assert_array_equal(r['weights'][:, wdx], lc.clean_pairs(N, b), err_msg='%d %d %s' % (N, h, name))
    assert any(b == 2 for b, _ in seen), (N, h)
    assert N >= 16 or any(b == 1 for b, _ in seen), (N, h)
    print('N=%d h=%d: mistimed rows (elements, exact fit): %s' % (N, h, dict(sorted(seen.items()))))


@pytest.mark.parametrize('N', lc.ALL_N)
def test_noisy_windows_do_not_close_and_hold_gross_outliers(N):
    x = lc.noisy_trace(N)
    n = lc.noisy_windows(N)
    assert n == (40 if N <= 9 else 8 if N <= 16 else 3)
    assert x.shape == (N, n * st.W + 1) and planner.window_plan(x.shape[1], st.FS, st.W / st.FS, 0.0) == (st.W, st.W, n)
    lag = lc.noisy_lags(N)
    assert lag.shape == (n, lc.npairs(N)) and np.abs(lag).max() < st.W
    for w in range(n):
        assert st.off_closure_pairs(lag[w], N) != [], 'window %d closes' % w
    dev = np.abs(lag - lc.plane_lags(N)[None, :])
    gross, on = float(np.mean(dev > 8)), float(np.mean(dev <= 1.5))
    print('N=%d: %d windows, %.0f %% of the lags within 1.5 samples of the wave, %.0f %% more than 8 samples off' % (
        N, n, 100 * on, 100 * gross))
    assert gross >= 0.2 and on >= 0.2                      # gross outliers, and a plane to find among them
    assert np.all(np.sum(dev > 8, axis=1) >= 1) or N < 7   # ... in every window (6 pairs can all be near the wave)


@pytest.mark.parametrize('N,h', lc.CASES, ids=[lc.case_id(c) for c in lc.CASES])
def test_sampled_confidence_intervals_are_converged(oracle, N, h):
    """``_check_against_oracle`` of tests/test_gpu_solve.py holds the kernel's confidence intervals to the oracle's ellipse
    sampled at 20 000 points within 1e-4.  The sampled minimum radius lies above the true one by up to
    ``a^2 d^2 / (2 r_min)`` (semi-axis a, half a sample step d = pi / 20 000): 1.2e-8 (a / r_min)^2 of r_min, more than
    1e-4 once the ellipse passes the origin within a hundredth of its semi-axis.  There the SAMPLING is what deviates (at
    320 000 points it moves onto the closed form); such a window would fail the GPU test whatever the kernel does.  So
    the traces hold none: on every window of both traces and at every h, the oracle's sampled and closed-form values
    agree within half the checker's tolerance."""
    xij = _xij(N)
    a = lc.alpha_of(lc.npairs(N), h)
    lag, _ = st.designed_lags(lc.pulse_tables(N))
    worst = 0.0
    for kind, r in (('pulse', st.oracle_lts(oracle, lag, xij, a)), ('noisy', lc.oracle_noisy(oracle, N, h))):
        gv, gb = lc.sampler_gap(oracle, xij, r['z'], r['sigma_tau'])
        for g in (gv, gb):
            if np.any(np.isfinite(g)):
                worst = max(worst, float(np.nanmax(g)))
                assert np.nanmax(g) <= 0.5, (N, h, kind, np.nanargmax(g), float(np.nanmax(g)))
    print('N=%d h=%d: sampled against closed-form confidence intervals, worst %.3g of the tolerance' % (N, h, worst))


@pytest.mark.parametrize('N,h', lc.CASES, ids=[lc.case_id(c) for c in lc.CASES])
def test_neighbouring_h_changes_the_result(oracle, N, h):
    """The oracle mutant of the module docstring.  A condition on the inputs: if it fails, the trace's seed or SNR is
    changed, never the minimum."""
    need = 2 if N <= 9 else 1
    for g in (h - 1, h + 1):
        if g not in lc.h_range(N):
            continue
        count = int(lc.mutant_differs(oracle, N, h, g).sum())
        print('N=%d h=%d searched with %d: %d of %d windows differ' % (N, h, g, count, lc.noisy_windows(N)))
        if N <= 9:
            assert count >= need, (N, h, g, count)
        elif count < need:
            print('NOT DISCRIMINATED: N=%d h=%d against %d' % (N, h, g))
            assert (N, h, g) in lc.NOT_DISCRIMINATED, 'a case below the minimum that lts_h_cases.NOT_DISCRIMINATED does not name'
        else:
            assert (N, h, g) not in lc.NOT_DISCRIMINATED, 'named as not discriminated, but it is'
