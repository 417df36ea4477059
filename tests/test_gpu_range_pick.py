"""The two range-restricted correlators against each other (csrc/lag_pick.h: the bounded and the seeded lag search are one
pick routine under two policies).  With the one-point grid [[0, 0]] every delay is 0, so the seeded range of every pair is
[-K, K] clamped to W-1: the bounded range with every limit equal to K.  On the same pre-filtered noise the two passes then
give equal lags and cmax equal as bit patterns — the general forms against each other, and the staged seeded form (both
of its branches) against the bounded general form on shared rows.  On windows that are not finite the two differ as their
contracts say, each checked against its own NumPy statement."""
import numpy as np
import pytest

import bounded_truth as bt
import test_gpu_bounded as tb
import test_gpu_seeded as ts
from narrow_band_least_squares_amd import _hip

pytestmark = pytest.mark.gpu

GRID0 = np.array([[0.0, 0.0]])


def _both(data_b, data_s, W, inc, L):
    """The bounded pass of ``data_b`` with every limit L and the seeded pass of ``data_s`` with half-width L around the
    zero delays of GRID0 -> (lag, cmax) of each."""
    P = len(bt.pair_table(data_b.shape[0]))
    lag_b, cmax_b = tb._pass(data_b, W, inc, np.full(P, L, dtype=np.int64))
    got = ts._pass(data_s, ts._geometry(data_s.shape[0]), W, inc, GRID0, L)
    assert not got['delays'].any()
    return lag_b, cmax_b, got['lag'], got['cmax']


def _assert_same_bits(lag_b, cmax_b, lag_s, cmax_s):
    np.testing.assert_array_equal(lag_b, lag_s)
    np.testing.assert_array_equal(np.ascontiguousarray(cmax_b).view(np.int64), np.ascontiguousarray(cmax_s).view(np.int64))


@pytest.mark.parametrize('W,L', [(48, 0), (48, 5), (48, 46), (130, 40)])
def test_the_general_forms_give_the_same_bits(W, L):
    """17 elements: both general forms.  W = 48 at one lag, 11 lags and all but the outermost (at L = W-1 the bounded plan
    takes the ordinary route); W = 130 at 81 lags: two trips of 64 lanes, the second partial."""
    data, inc, _ = tb._noise(17, W, nwin=4)
    assert _hip.lag_limit_form(17, W, L) == 2 and _hip.lag_seed_form(17, W) == 2
    lag_b, cmax_b, lag_s, cmax_s = _both(data, data, W, inc, L)
    assert np.all(np.abs(lag_b) <= L) and np.all(np.isfinite(cmax_b))
    _assert_same_bits(lag_b, cmax_b, lag_s, cmax_s)


@pytest.mark.parametrize('L', [40, 9])
def test_the_staged_seeded_form_gives_the_bits_of_the_bounded_general_form(L):
    """8 x 130 seeded (staged form: a wave per pair at K = 40, packed chunks at K = 9) against 17 x 130 bounded (general
    form) whose first 8 rows are the same data: the 28 shared pairs."""
    W = 130
    data17, inc, _ = tb._noise(17, W, nwin=4)
    data8 = np.ascontiguousarray(data17[:8])
    p17 = bt.pair_table(17)
    shared = [k for k, (i, j) in enumerate(p17) if j < 8]
    assert [p17[k] for k in shared] == bt.pair_table(8)
    assert _hip.lag_limit_form(17, W, L) == 2 and _hip.lag_seed_form(8, W) == 1
    lag_b, cmax_b, lag_s, cmax_s = _both(data17, data8, W, inc, L)
    _assert_same_bits(lag_b[:, shared], cmax_b[:, shared], lag_s, cmax_s)


def test_windows_that_are_not_finite_keep_the_two_contracts_apart():
    """17 x 48, L = K = 5, windows that do not overlap.  A NaN sample in element 1's window 1: bounded gives
    min(plain lag, L) = L, seeded gives hi = L, both cmax NaN.  A +Inf sample three from the end of element 3's window 2:
    bounded gives min(plain lag, L) — lag 2 for the pairs (3, j) —, seeded still hi.  Each result against its own truth
    module; the clean pairs keep equal bits."""
    W, L = 48, 5
    data = np.random.default_rng(4100 + 37 * 17 + W + 7).standard_normal((17, 4 * W + 1))
    starts = [w * W for w in range(4)]
    data[1, W + W // 3] = np.nan
    data[3, 2 * W + W - 3] = np.inf
    pairs = bt.pair_table(17)
    lim = np.full(len(pairs), L, dtype=np.int64)
    assert _hip.lag_limit_form(17, W, L) == 2 and _hip.lag_seed_form(17, W) == 2
    with np.errstate(invalid='ignore'):
        exp_lag, exp_cmax = bt.pick_windows(data, W, starts, pairs, lim)
    lag_b, cmax_b = tb._pass(data, W, W, lim)
    got = ts._pass(data, ts._geometry(17), W, W, GRID0, L)
    assert not got['delays'].any()
    bad = np.array([[(w == 1 and 1 in p) or (w == 2 and 3 in p) for p in pairs] for w in range(4)])
    np.testing.assert_array_equal(np.isnan(exp_cmax), bad)
    # bounded: NumPy's first NaN of the slice
    np.testing.assert_array_equal(lag_b, exp_lag)
    np.testing.assert_array_equal(np.isnan(cmax_b), bad)
    np.testing.assert_allclose(cmax_b[~bad], exp_cmax[~bad], rtol=0, atol=1e-12)
    # seeded: the first lag of the range
    ts._check(got, data, W, starts, L)
    np.testing.assert_array_equal(np.isnan(got['cmax']), bad)
    np.testing.assert_array_equal(got['lag'][bad], L)
    # where they differ, and where they do not
    np.testing.assert_array_equal(lag_b[1][bad[1]], L)
    inf_a = np.array([p[0] == 3 for p in pairs])
    np.testing.assert_array_equal(lag_b[2, inf_a], 2)
    np.testing.assert_array_equal(lag_b[2, bad[2] & ~inf_a], L)
    np.testing.assert_array_equal(lag_b != got['lag'], bad & (np.arange(4) == 2)[:, None] & inf_a[None, :])
    _assert_same_bits(lag_b[~bad], cmax_b[~bad], got['lag'][~bad], got['cmax'][~bad])
