"""Without a GPU: the cases of tests/test_gpu_seams.py (tests/seam_cases.py) reach what they were built for — the seam
lists are what the kernels' constants give, the LDS helpers switch where the tests say, the crafted refinement traces
have their designed arg-max, the grids are clear of rounding ties, the window counts are as assumed — and the
references alone meet the conditions under which a comparison there cannot hide a failure:

* beam: no delay within 2e-6 of a rounding tie at the oracle's slowness of the same data (the GPU's slowness agrees
  with it to 1e-9, the comparison leaves out cells within 1e-6: none is skipped, where at most 1 % may be), and F is
  compared on at least half the windows of a case;
* grid: no ``power_only`` cell;
* refinement: at least three windows, no lag at the end of the range, |D| >= 2^20 E, at least half the fractions non-zero."""
import os
import re

import numpy as np
import pytest

import beam_truth as bt
import grid_truth as gt
import refine_truth as rt
import seam_cases as sc
import test_gpu_grid as tg
from narrow_band_least_squares_amd import planner, engine, _hip

FS = sc.FS
TIE_MARGIN = 2e-6


def test_stated_constants_are_the_sources():
    for name, pattern, value in sc.STATED:
        with open(os.path.join(sc.CSRC, name)) as f:
            found = re.findall(pattern, f.read())
        assert found and all(int(v) == value for v in found), '%s: %s gives %r, tests/seam_cases.py states %d' % (
            name, pattern, found, value)


def test_seam_lists_are_what_the_constants_give():
    assert sc.BEAM_SEAMS == [255, 256, 511, 512, 513, 1023, 1024, 1025]
    assert sc.GRID_SEAMS == [255, 256, 511, 512, 513]
    assert sc.REFINE_SEAMS == [63, 64, 127, 128, 129]
    trips = lambda W, step: -(-W // step)
    # beam: one wave up to BEAM_WAVE_W in trips of 256 samples, the workgroup beyond in trips of 1024
    one = [W for W in sc.BEAM_SEAMS if W <= sc.BEAM_WAVE_W]
    assert [trips(W, sc.BEAM_WAVE_STEP) for W in one] == [1, 1, 2, 2] and [W % sc.BEAM_WAVE_STEP for W in one] == [255, 0, 255, 0]
    coop = [W for W in sc.BEAM_SEAMS if W > sc.BEAM_WAVE_W]
    assert [trips(W, sc.BEAM_COOP_STEP) for W in coop] == [1, 1, 1, 2] and coop[0] == sc.BEAM_WAVE_W + 1
    # grid: whole steps and the partial one
    assert [(W // sc.GRID_BLOCK, W % sc.GRID_BLOCK > 0) for W in sc.GRID_SEAMS] == [(0, True), (1, False), (1, True), (2, False),
                                                                                  (2, True)]
    assert [(W // sc.REFINE_STEP, W % sc.REFINE_STEP) for W in sc.REFINE_SEAMS] == [(0, 63), (1, 0), (1, 63), (2, 0), (2, 1)]
    assert sc.MIXED_W == (513, 65) and sc.SIZE_W == (65, 513) and sc.CRAFTED_W == (16, 65)
    assert [c[0] for c in sc.BEAM_SIZE_CASES] == [16, 16, 17, 17, 32, 32] and (32, 0.5, 513) not in sc.OTHER_SIZE_CASES
    assert len(sc.OTHER_SIZE_CASES) == 5


def test_lds_helpers_switch_where_the_tests_say():
    assert [sc.refine_switch(N) for N in sc.REFINE_SWITCH_N] == [3413, 320]
    for N in sc.REFINE_SWITCH_N:
        W = sc.refine_switch(N)
        assert _hip.refine_lds_bytes(N, W) == N * W * 8 and _hip.refine_lds_bytes(N, W + 1) == 0
    lib = _hip.load_library()
    assert [sc.largest_staged_halo(N, W) for N, W, _ in sc.GRID_CAP_SHAPES] == [2367, 279]
    for N, W, _ in sc.GRID_CAP_SHAPES:
        H = sc.largest_staged_halo(N, W)
        assert lib.nbls_beam_grid_lds_bytes(N, W, H) == N * (W + 2 * H) * 8 and lib.nbls_beam_grid_lds_bytes(N, W, H + 1) == 0


def test_window_counts_are_as_assumed():
    for W in sc.BEAM_SEAMS + sc.REFINE_SEAMS + list(sc.SIZE_W) + [sc.refine_switch(N) + k for N in sc.REFINE_SWITCH_N for k in (0, 1)]:
        npts = sc.trace_len(W)
        got_W, inc, nwin = planner.window_plan(npts, FS, sc.winlen(W), 0.5)
        assert (got_W, nwin) == (W, 11) and npts % 2 == 1 and 5 * W < npts < 7 * W
        assert 2 <= npts - ((nwin - 1) * inc + W) <= 3                       # a delay of four samples reads behind the end
    for N, W, n in sc.GRID_CAP_SHAPES:
        assert planner.window_plan(sc.trace_len(W, n), FS, sc.winlen(W), 0.5)[::2] == (W, n)
    # the mixed workgroup: units are band-major (nbls_plan: unit_off), a workgroup takes BEAM_WAVES consecutive ones
    for order in (sc.MIXED_W, sc.MIXED_W[::-1]):
        W, inc, nwin, _ = engine.plan_windows(sc.MIXED_NPTS, FS, [sc.winlen(w) for w in order], 0.5)
        assert tuple(W) == order and nwin[0] % sc.BEAM_WAVES != 0
        assert (W[0] > sc.BEAM_WAVE_W) != (W[1] > sc.BEAM_WAVE_W)
    for W in sc.CRAFTED_W:
        for kinds in (sc.CRAFTED_KINDS, sc.NAN_KINDS):
            x = sc.crafted_trace(W, kinds)
            assert planner.window_plan(x.shape[1], FS, sc.winlen(W), 0.0) == (W, W, len(kinds))


def _grid_cases():
    """(label, data, xij, grid, W) of every pass of the grid tests."""
    out = []
    for W in sc.GRID_SEAMS:
        data, rij = sc.plane_wave(4, W)
        xij = planner.co_array(rij)[0]
        out.append(('steps W=%d staged' % W, data, xij, tg.GRID5, W))
        out.append(('steps W=%d global' % W, data, xij, sc.far_grid(xij, 4, W), W))
    for N, W, n in sc.GRID_CAP_SHAPES:
        data, rij = sc.plane_wave(N, W, nwin=n)
        xij = planner.co_array(rij)[0]
        H, grids = sc.cap_grids(xij, N, W)
        out.extend(('cap N=%d W=%d H%+d' % (N, W, k), data, xij, g, W) for k, g in enumerate(grids))
    for N, alpha, W in sc.OTHER_SIZE_CASES:
        data, rij = sc.plane_wave(N, W, mistimed=alpha < 1.0)
        out.append(('sizes N=%d W=%d' % (N, W), data, planner.co_array(rij)[0], tg.GRID5, W))
    return out


def test_grids_are_clear_of_ties_and_take_the_form_they_were_built_for():
    lib = _hip.load_library()
    for label, data, xij, grid, W in _grid_cases():
        N = data.shape[0]
        d, tau = gt.delay_table(xij, grid, FS, N)
        assert not gt.near_tie(tau), label
        H = int(np.abs(d).max())
        staged = lib.nbls_beam_grid_lds_bytes(N, W, H) > 0
        if label.startswith('steps'):
            assert staged == label.endswith('staged'), label
        if label.startswith('cap'):
            cap = sc.largest_staged_halo(N, W)
            assert H == cap + int(label[-1]) and staged == label.endswith('+0'), label
            assert int(np.abs(d[:len(tg.GRID5)]).max()) < cap and d.min() < 0 < d.max()
            # the far point's samples are data in the first windows: the far end of the staged block is not all zeros
            assert W + H < data.shape[1]


@pytest.mark.parametrize('k', range(19))
def test_grid_references_have_no_power_only_cell(k):
    label, data, xij, grid, W = _grid_cases()[k]
    _, inc, n = planner.window_plan(data.shape[1], FS, sc.winlen(W), 0.5)
    ref = gt.grid_reference(data, FS, xij, grid, W, inc, n)
    assert not ref['power_only'].any() and np.all(ref['index'] >= 0), label
    # (the maximum lies among GRID5's points: index, F and P there are compared between the two forms)
    assert np.count_nonzero(ref['index'] < len(tg.GRID5)) >= n // 2 + 1, label


def test_the_grid_cases_are_counted():
    assert len(_grid_cases()) == 19


def _oracle_z(oracle, data, xij, W, alpha, overlap=0.5):
    """The oracle's slowness of every window -> (z (nwin, 2), inc, nwin)."""
    N, npts = data.shape
    Wp, inc, starts = oracle.window_plan(npts, FS, sc.winlen(W), overlap)
    assert Wp == W
    tau, _, _ = oracle.correlate_windows(np.ascontiguousarray(data.T), W, starts, oracle.pair_table(N), FS)
    if alpha == 1.0:
        z = oracle.ols_solve(xij, tau)[0]
    else:
        z = oracle.lts_post_process(tau, xij, oracle.fast_lts(tau, xij, alpha), alpha)[0]
    return np.ascontiguousarray(z.T), inc, len(starts)


def _beam_conditions(data, xij, z, W, inc, n, label):
    N = data.shape[0]
    assert np.all(np.isfinite(z)), label
    tau = FS * (xij[None, :N - 1, 0] * z[:, None, 0] + xij[None, :N - 1, 1] * z[:, None, 1])
    dist = np.abs(np.abs(tau - np.floor(tau)) - 0.5).min()
    assert dist >= TIE_MARGIN, '%s: a delay %.3g from a rounding tie (change the seed)' % (label, dist)
    ref = bt.beam_reference(data, FS, xij, z, W, inc, n)
    assert not ref['skip'].any()
    on_f = int(np.count_nonzero(~ref['power_only'] & np.isfinite(ref['fstat'])))
    assert on_f >= n // 2, '%s: F compared on %d of %d windows' % (label, on_f, n)
    return ref


@pytest.mark.parametrize('W', sc.BEAM_SEAMS)
def test_beam_window_cases_meet_the_conditions(oracle, W):
    data, rij = sc.plane_wave(4, W, mistimed=True, swap=True)
    xij = planner.co_array(rij)[0]
    z, inc, n = _oracle_z(oracle, data, xij, W, 0.5)
    _beam_conditions(data, xij, z, W, inc, n, 'W=%d' % W)
    before, behind = sc.reads_outside(xij, z, W, inc, n, data.shape[1], 4)
    assert before >= 1 and behind >= 1


@pytest.mark.parametrize('N,alpha,W', sc.BEAM_SIZE_CASES)
def test_beam_size_cases_meet_the_conditions(oracle, N, alpha, W):
    data, rij = sc.plane_wave(N, W, mistimed=alpha < 1.0)
    xij = planner.co_array(rij)[0]
    z, inc, n = _oracle_z(oracle, data, xij, W, alpha)
    _beam_conditions(data, xij, z, W, inc, n, 'N=%d W=%d' % (N, W))


def test_beam_sub_array_case_meets_the_conditions(oracle):
    data, rij = sc.plane_wave(32, sc.SIZE_W[0], mistimed=True)
    kept = engine.kept_elements(32, sc.SUB_REMOVE)
    assert len(kept) == 30 and 31 in kept
    xij = planner.co_array(np.ascontiguousarray(rij[:, kept]))[0]
    z, inc, n = _oracle_z(oracle, data[kept], xij, sc.SIZE_W[0], 0.5)
    _beam_conditions(data[kept], xij, z, sc.SIZE_W[0], inc, n, '30 of 32')


def test_beam_mixed_case_meets_the_conditions(oracle):
    """The two bands of the mixed-workgroup pass, filtered by the oracle as the pass filters them."""
    data, rij = sc.plane_wave(4, None, npts=sc.MIXED_NPTS)
    xij = planner.co_array(rij)[0]
    for (fmin, fmax), W in zip(sc.MIXED_BANDS, sc.MIXED_W):
        stf, _, _ = oracle.filter_data(oracle.make_stream(data, FS), 'butter', fmin, fmax, 2, 0.01)
        filt = np.stack([tr.data for tr in stf])
        z, inc, n = _oracle_z(oracle, filt, xij, W, 1.0)
        _beam_conditions(filt, xij, z, W, inc, n, 'band of W=%d' % W)


def _refine_conditions(data, W, label):
    N = data.shape[0]
    _, inc, n = planner.window_plan(data.shape[1], FS, sc.winlen(W), 0.5)
    starts, pairs = [w * inc for w in range(n)], rt.pair_table(N)
    lag = rt.pick_lags(data, W, starts, pairs)
    ref = rt.refine_windows(data, W, starts, pairs, lag)
    assert n >= 3 and np.all(np.abs(lag) < W - 1), label
    assert np.all(np.abs(ref['D']) >= 2.0 ** 20 * ref['E']), label
    assert np.all(np.isfinite(ref['bound'])) and np.count_nonzero(ref['frac']) >= ref['frac'].size // 2, label


@pytest.mark.parametrize('N,W', [(4, W) for W in sc.REFINE_SEAMS] + [(N, sc.refine_switch(N) + k) for N in sc.REFINE_SWITCH_N
                                                                     for k in (0, 1)])
def test_refinement_window_cases_meet_the_conditions(N, W):
    _refine_conditions(sc.sinusoids(N, W, mistimed=N == 4)[0], W, 'N=%d W=%d' % (N, W))


@pytest.mark.parametrize('N,alpha,W', sc.OTHER_SIZE_CASES)
def test_refinement_size_cases_meet_the_conditions(N, alpha, W):
    _refine_conditions(sc.sinusoids(N, W, mistimed=alpha < 1.0)[0], W, 'N=%d W=%d' % (N, W))


@pytest.mark.parametrize('W', sc.CRAFTED_W)
def test_crafted_traces_have_their_designed_arg_max_and_a_non_zero_fraction(oracle, W):
    LD = np.longdouble
    kinds = sc.CRAFTED_KINDS
    x = sc.crafted_trace(W, kinds)
    starts = [w * W for w in range(len(kinds))]
    tau, _, _ = oracle.correlate_windows(np.ascontiguousarray(x.T), W, starts, sc.CRAFTED_PAIRS, FS)
    lag = np.rint(tau.T * FS).astype(np.int64)
    np.testing.assert_array_equal(lag, sc.crafted_lags(kinds, W))
    ref = rt.refine_windows(x, W, starts, sc.CRAFTED_PAIRS, lag)
    for w, kind in enumerate(kinds):
        sign = 1 if kind == '+' else -1
        assert lag[w, 0] == sign * (W - 2) and lag[w, 5] == sign * (W - 1)
        assert ref['frac'][w, 0] == float(-sign * LD(1) / 12)                 # the last refined lag, not zero
        assert ref['frac'][w, 5] == 0.0 and np.isnan(ref['D'][w, 5])          # the end of the range: the rule, not a value
        # R(l+1), R(l), R(l-1) of the pick have one, two and three terms (the far one first)
        a, b = x[0, starts[w]:starts[w] + W], x[1, starts[w]:starts[w] + W]
        r = [float(v) for v in rt.corr3(a, b, int(lag[w, 0]))]
        assert r == ([0.5, 1.125, 0.25] if kind == '+' else [0.25, 1.125, 0.5])
    plus = kinds.index('+')
    assert lag[plus, 3] == -(W - 2) and ref['frac'][plus, 3] == float(-LD(1) / 14)     # pair (1, 2) of a plus window
    assert np.all(np.isfinite(ref['bound']))
    # the NaN trace: windows 1 and 2 are clean, their picks and fractions those of the plain trace
    xn = sc.crafted_nan_trace(W)
    assert np.isnan(xn[0, W - 1]) and np.isnan(xn[0, 3 * W]) and np.count_nonzero(np.isnan(xn)) == 2
    tau, _, _ = oracle.correlate_windows(np.ascontiguousarray(xn.T), W, [W, 2 * W], sc.CRAFTED_PAIRS, FS)
    lagn = np.rint(tau.T * FS).astype(np.int64)
    np.testing.assert_array_equal(lagn, sc.crafted_lags(sc.NAN_KINDS[1:3], W))
    refn = rt.refine_windows(xn, W, [W, 2 * W], sc.CRAFTED_PAIRS, lagn)
    assert refn['frac'][0, 0] == float(-LD(1) / 12) and refn['frac'][1, 0] == float(LD(1) / 12)
