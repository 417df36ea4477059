"""tests/grid_refine_truth.py against itself and the demonstration of DESIGN.md section 28 (CPU): the replay is exact, a
float64 greedy search passes ``check_cell`` as the GPU must, the prefix property and the monotonicity hold, the inputs of the
GPU cases keep the path check, and a coarse grid with refinement does what the section says it does."""
from fractions import Fraction

import numpy as np
import pytest

import grid_refine_truth as grt
import steer_truth as stt


def _coarse(filt, fs, xij, grid, W, starts, taps):
    """The float64 grid maximum of every window -> (index (nwin,), F (nwin,)); -1 / NaN where no point has a ratio."""
    n, c, _, _ = stt.grid_tables(xij, grid, fs, len(filt), taps)
    F = stt.grid_fstat64(filt, W, starts, n, c)
    idx = np.array([-1 if np.all(np.isnan(r)) else int(np.nanargmax(r)) for r in F])
    return idx, np.array([np.nan if i < 0 else F[k, i] for k, i in enumerate(idx)])


def _search(filt, fs, xij, grid, W, starts, taps, step, levels, fast=False):
    """Coarse maximum + greedy refinement of every window -> (index, F0, list of ``greedy64`` dicts or None)."""
    idx, F0 = _coarse(filt, fs, xij, grid, W, starts, taps)
    N = len(filt)
    out = []
    for k, s0 in enumerate(starts):
        if idx[k] < 0:
            out.append(None)
            continue
        if fast:                                 # one vectorised evaluation per slowness (F only; P is not looked at)
            def evaluate(s, s0=s0):
                n, c, _, _ = stt.grid_tables(xij, s[None, :], fs, N, taps)
                return float(stt.grid_fstat64(filt, W, [s0], n, c)[0, 0]), 0.0
        else:
            def evaluate(s, s0=s0):
                return grt.fstat64(filt, fs, xij, s0, W, taps, s)
        P0 = 0.0 if fast else grt.fstat64(filt, fs, xij, s0, W, taps, grid[idx[k]])[1]
        out.append(grt.greedy64(evaluate, grid[idx[k]], F0[k], P0, step, levels))
    return idx, F0, out


def test_replay_is_exact():
    """Dyadic grid point and step: every addition is exact, so the replay equals the rational sum; any step: the centre stays
    within step (1 - 2^-R) of the grid point, a path of fours does not move it, and -0.0 survives a centre that stays."""
    rng = np.random.default_rng(3)
    g, step = np.array([-1.5, 0.75]), np.array([0.5, 0.25])
    for R in (1, 2, 5, 12):
        path = rng.integers(0, 9, size=R)
        c = grt.replay(g, step, path)
        assert c.shape == (R + 1, 2) and np.array_equal(c[0], g)
        want = [Fraction(float(g[0])), Fraction(float(g[1]))]
        for l, j in enumerate(path, start=1):
            a, b = grt.offsets(int(j))
            want[0] += a * Fraction(float(step[0])) / 2 ** l
            want[1] += b * Fraction(float(step[1])) / 2 ** l
            assert Fraction(float(c[l, 0])) == want[0] and Fraction(float(c[l, 1])) == want[1]
    g, step = np.array([0.1, -0.3]), np.array([0.7, 1.1])
    for R in (1, 7, 12):
        for path in (np.zeros(R, dtype=int), np.full(R, 8), rng.integers(0, 9, size=R)):
            c = grt.replay(g, step, path)
            assert np.all(np.abs(c[-1] - g) <= grt.reach(g, step, R))
        assert np.all(grt.reach(g, step, R) < step)
        assert grt.same_bits(grt.replay(g, step, np.full(R, 4))[-1], g)
    assert np.signbit(grt.replay(np.array([-0.0, 0.0]), step, [4, 4])[-1][0])
    assert not np.signbit(grt.replay(np.array([-0.0, 0.0]), step, [3])[-1][0])       # a = 0: -0.0 + 0.0 * e = +0.0
    assert np.all(np.isnan(grt.replay(g, step, [-1, -1, -1])))
    assert [grt.offsets(j) for j in range(9)] == [(a, b) for a in (-1, 0, 1) for b in (-1, 0, 1)]


def test_the_order_of_the_candidates():
    nan, inf = np.nan, np.inf
    assert grt.choose([1, 1, 1, 1, nan, 1, 1, 1, 1], 1.0) == 4                      # the centre before any other
    assert grt.choose([1, 3, 1, 3, nan, 3, 1, 1, 1], 2.0) == 1                      # then j ascending
    assert grt.choose([nan] * 9, 0.5) == 4 and grt.choose([nan, 7.0] + [nan] * 7, 0.5) == 1
    assert grt.choose([1, 2, inf, 3, nan, inf, 1, 1, 1], 5.0) == 2 and grt.choose([inf] * 9, inf) == 4


@pytest.mark.parametrize('N,W,taps,levels,noise', [(3, 16, 4, 5, True), (4, 65, 6, 3, False), (8, 130, 8, 2, False)])
def test_a_float64_greedy_search_agrees_with_the_truth(N, W, taps, levels, noise):
    """What the GPU is held to, held against the float64 restatement: ``check_row`` passes, the prefix property and the
    monotonicity hold."""
    data, rij, inc = grt.case_inputs(N, W, noise)
    from narrow_band_least_squares_amd import planner
    xij = planner.co_array(rij)[0]
    step = grt.lattice_step(grt.GRID5)
    starts = [w * inc for w in range(4)]
    idx, F0, found = _search(data, grt.FS, xij, grt.GRID5, W, starts, taps, step, levels)
    assert np.all(idx >= 0)
    refined = (np.array([f['slowness'] for f in found]), np.array([f['fstat'] for f in found]), np.array([f['power'] for f in found]),
               np.array([f['path'] for f in found]), np.array([f['stencil'] for f in found]))
    skipped, total, worst = grt.check_row(data, grt.FS, xij, W, inc, 4, taps, grt.GRID5, step, levels, idx, F0, refined)
    print('N=%d W=%d taps=%d levels=%d: %d of %d levels skipped, worst |dF| / bound %.3g' % (N, W, taps, levels, skipped, total, worst))
    assert total == 4 * levels and skipped <= 0.05 * total and worst <= 1.0
    for k, f in enumerate(found):
        assert f['fstat'] >= F0[k] and np.all(np.abs(f['slowness'] - grt.GRID5[idx[k]]) <= grt.reach(grt.GRID5[idx[k]], step, levels))
        assert grt.same_bits(f['centres'], grt.replay(grt.GRID5[idx[k]], step, f['path']))
        if np.all(f['path'][:-1] == 4):
            assert f['stencil'][4] == F0[k]
    for l in range(1, levels):                   # the prefix property: an l-level search is the first l levels
        _, _, short = _search(data, grt.FS, xij, grt.GRID5, W, starts, taps, step, l)
        for f, s in zip(found, short):
            assert np.array_equal(s['path'], f['path'][:l]) and grt.same_bits(s['slowness'], f['centres'][l])


@pytest.mark.parametrize('case', grt.CASES, ids=lambda c: 'N%d-W%d-L%d-R%d-%s-%s' % (c[0], c[1], c[2], c[3], 'noise' if c[4] else 'wave', c[5]))
def test_the_inputs_of_the_gpu_cases_keep_the_path_check(case):
    """No more than 5 % of a case's levels may be skipped for the path check (a ``power_only`` bound): the float64 search on
    the case's own inputs stays within that, and passes the check the GPU has to pass."""
    N, W, taps, levels, noise, gname = case
    from narrow_band_least_squares_amd import planner
    grid = grt.GRIDS[gname]
    data, rij, inc = grt.case_inputs(N, W, noise)
    xij = planner.co_array(rij)[0]
    step = grt.lattice_step(grid)
    starts = [w * inc for w in range(4)]
    idx, F0, found = _search(data, grt.FS, xij, grid, W, starts, taps, step, levels)
    assert np.all(idx >= 0) and 9 <= len(grid) <= 25
    refined = tuple(np.array([f[k] for f in found]) for k in ('slowness', 'fstat', 'power', 'path', 'stencil'))
    skipped, total, worst = grt.check_row(data, grt.FS, xij, W, inc, 4, taps, grid, step, levels, idx, F0, refined)
    print('%r: %d of %d levels skipped, worst |dF| / bound %.3g' % (case, skipped, total, worst))
    assert skipped <= 0.05 * total and worst <= 1.0
    K = taps // 2                                # taps off both ends of the trace
    n = stt.grid_tables(xij, grid, grt.FS, N, taps)[0]
    assert n.min() - K + 1 < 0 and 3 * inc + W - 1 + n.max() + K >= data.shape[1]


# ---- the demonstration -------------------------------------------------------------------------------------------------
def small_array_statements(true, fine, coarse, refined):
    """What DESIGN.md section 28 says of the section 22.4 trace (100 m array, 20 Hz, 1-3 Hz, 8 windows), asserted on the
    slowness vectors (8, 2) of the 41 x 41 grid's maximum, the 11 x 11 grid's and its refinement, each with its F (8,)."""
    err = {k: np.hypot(*(v[0] - true).T) for k, v in (('fine', fine), ('coarse', coarse), ('refined', refined))}
    assert np.all(refined[1] >= coarse[1])                                   # refined F >= coarse F in every window
    assert np.median(err['refined']) <= np.median(err['fine'])               # ... no worse a slowness than the fine grid's
    return err


def demonstration_small(taps=8):
    d = stt.demonstration(taps)
    filt, fs, xij, W, starts, true = d['filt'], d['fs'], d['xij'], d['W'], d['starts'], d['true']
    ax = np.arange(-5, 6) * 0.8
    coarse_grid = np.ascontiguousarray(np.stack(np.meshgrid(ax, ax, indexing='ij'), axis=-1).reshape(-1, 2))
    fi, fF = _coarse(filt, fs, xij, d['grid'], W, starts, taps)
    ci, cF, found = _search(filt, fs, xij, coarse_grid, W, starts, taps, np.array([0.8, 0.8]), 4, fast=True)
    fine = (d['grid'][fi], fF)
    coarse = (coarse_grid[ci], cF)
    refined = (np.array([f['slowness'] for f in found]), np.array([f['fstat'] for f in found]))
    return d, coarse_grid, fine, coarse, refined


def test_demonstration_small_array():
    d, coarse_grid, fine, coarse, refined = demonstration_small()
    err = small_array_statements(d['true'], fine, coarse, refined)
    for name, evals, k, v in (('41 x 41, step 0.2', '1681', 'fine', fine), ('11 x 11, step 0.8', '121', 'coarse', coarse),
                              ('11 x 11 + 4 levels', '121 + 32', 'refined', refined)):
        print('100 m array, 8 taps, %-20s %9s evaluations: slowness error median %.3f worst %.3f s/km, median F %.1f'
              % (name, evals, np.median(err[k]), np.max(err[k]), np.median(v[1])))


def test_demonstration_large_array():
    """The section 15 trace: 8 elements in a 1 km disc at 40 Hz, a plane wave (225 deg, 0.34 km/s) at -6 dB in 1.0-1.1 Hz,
    40 windows of 1200 samples.  ``slowness_grid(4.0, 21)`` (317 points) and 4 levels: refined F >= coarse F in every window,
    and no fewer windows within 5 degrees and 10 % of the truth than the coarse maximum alone.  The comparison with the
    1257-point grid (27 windows, median F 6.20: 1257 evaluations against 317 + 32) is recorded in DESIGN.md section 28."""
    from scipy import signal
    from narrow_band_least_squares_amd import planner, synthetic
    from narrow_band_least_squares_amd.lts_array import refined_slowness
    fs, W, N, nwin, taps = 40.0, 1200, 8, 40, 8
    inc = W // 2
    rij = synthetic.array_geometry(N, 1.0)
    data = synthetic.plane_wave(rij, W + (nwin - 1) * inc + 1, fs, 0.1, 10.0, snr_db=-6.0)
    filt = np.ascontiguousarray(signal.sosfiltfilt(signal.butter(2, [1.0, 1.1], btype='bandpass', fs=fs, output='sos'), data, axis=1))
    xij = planner.co_array(rij)[0]
    starts = [w * inc for w in range(nwin)]
    s = 1.0 / 0.34
    true = np.array([s * np.sin(np.deg2rad(225.0)), s * np.cos(np.deg2rad(225.0))])

    def hits(slow):
        vel, baz = refined_slowness(slow, np.zeros(len(slow), dtype=int))
        dbaz = np.abs((baz - 225.0 + 180.0) % 360.0 - 180.0)
        return int(np.count_nonzero((dbaz <= 5.0) & (np.abs(vel - 0.34) <= 0.034)))
    grid = planner.slowness_grid(4.0, 21)
    step = planner.grid_cells(grid)[1]
    assert grid.shape == (317, 2) and np.allclose(step, 0.4)
    ci, cF, found = _search(filt, fs, xij, grid, W, starts, taps, step, 4, fast=True)
    rs, rF = np.array([f['slowness'] for f in found]), np.array([f['fstat'] for f in found])
    got = dict(coarse=hits(grid[ci]), refined=hits(rs))
    print('1 km array, -6 dB, 8 taps, 317 points + 4 levels (317 + 32 evaluations): windows within 5 deg / 10 %% of the truth (of %d): %r; '
          'slowness error median %.3f -> %.3f s/km, median F %.2f -> %.2f'
          % (nwin, got, np.median(np.hypot(*(grid[ci] - true).T)), np.median(np.hypot(*(rs - true).T)), np.median(cF), np.median(rF)))
    assert np.all(rF >= cF)
    assert got['refined'] >= got['coarse']
    # recorded, not asserted: a coarse step wider than the main lobe (81 points, step 0.8 s/km, 5 levels) misses it
    wide = planner.slowness_grid(4.0, 11)
    wi, wF, wfound = _search(filt, fs, xij, wide, W, starts, taps, planner.grid_cells(wide)[1], 5, fast=True)
    print('1 km array, %d points, step %.1f s/km, + 5 levels: %d windows (coarse maximum alone: %d)'
          % (len(wide), planner.grid_cells(wide)[1][0], hits(np.array([f['slowness'] for f in wfound])), hits(wide[wi])))
