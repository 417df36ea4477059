"""The refinement of the grid maximum between grid points (``nbls_set_beam_grid_refinement``, csrc/beam_grid_refine.hip;
DESIGN.md section 28) against tests/grid_refine_truth.py: the GPU's own trail judged level by level within the derived
long-double bounds, the consequences of the definition bit for bit, both forms of the kernel, bit-equality between the
forms of a pass, the special values, the refusals and the public entry points."""
import os
import subprocess
import sys

import numpy as np
import pytest

import grid_refine_truth as grt
import steer_truth as stt
from test_grid_refine_truth import small_array_statements
from narrow_band_least_squares_amd import (engine, planner, synthetic, _hip, ltsva_grid, ltsva_steered, ltsva_grid_refined,
                                           ltsva_grid_refined_batch, narrow_band_least_squares_grid_refined,
                                           narrow_band_least_squares_grid, get_freqlist, get_winlenlist)

pytestmark = pytest.mark.gpu

FS = grt.FS
T0 = 17884.0729166667
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID5 = grt.GRID5
STEP5 = np.array([1.535, 1.535])
PLAIN = ('vel', 'baz', 'mdccm', 'sigma_tau', 'mask')
GRID = ('grid_index', 'grid_fstat', 'grid_power')
REFINED = ('grid_refined_slowness', 'grid_refined_fstat', 'grid_refined_power', 'grid_refined_path', 'grid_refined_stencil')


def _same(a, b, keys, label=''):
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and x.dtype == y.dtype, (label, k)
        assert x.tobytes() == y.tobytes() or np.array_equal(x, y, equal_nan=True), (label, k)


def _process(data, rij, W, taps, levels, step=None, grid=GRID5, alpha=1.0, overlap=0.5, fs=FS, **kw):
    res = engine.process(data, fs, T0, rij, [(None, None)], [(W + 0.5) / fs], overlap, alpha, prefiltered=True, slowness_grid=grid,
                         beam_taps=taps, grid_refine=None if not levels else (levels, step), **kw)
    assert int(res.W[0]) == W
    return res


def _refined(res, row=0):
    return tuple(getattr(res, k)[row] for k in REFINED)


def _halo(xij, N, grid, taps, step, fs=FS):
    """H_r of the plan, as include/nbls.h derives it."""
    xr = np.abs(np.asarray(xij)[:N - 1])
    return int(stt.grid_tables(xij, grid, fs, N, taps)[3] + np.ceil(fs * np.max(xr[:, 0] * step[0] + xr[:, 1] * step[1])) + 1)


def _check_consequences(res, grid, step, levels, row=0):
    """What follows from the definition, bit for bit, in every computed cell of a row; zeros beyond."""
    n = int(res.nwin[row])
    slow, fstat, power, path, stencil = _refined(res, row)
    idx, gf, gp = (getattr(res, k)[row] for k in GRID)
    for w in range(n):
        if idx[w] < 0:
            assert np.all(np.isnan(slow[w])) and np.isnan(fstat[w]) and np.isnan(power[w]) and np.all(np.isnan(stencil[w]))
            assert np.all(path[w] == -1)
            continue
        assert fstat[w] >= gf[w], (w, fstat[w], gf[w])
        assert grt.same_bits(slow[w], grt.replay(grid[idx[w]], step, path[w])[-1]), w
        assert np.all(np.abs(slow[w] - grid[idx[w]]) <= grt.reach(grid[idx[w]], step, levels)), w
        if np.all(path[w] == 4):
            assert grt.same_bits(fstat[w], gf[w]) and grt.same_bits(power[w], gp[w]) and grt.same_bits(slow[w], grid[idx[w]]), w
        if levels == 1 or np.all(path[w][:-1] == 4):
            assert grt.same_bits(stencil[w][4], gf[w]), w                            # the centre is the grid kernel's own value
        j = int(path[w][-1])
        assert grt.same_bits(fstat[w], stencil[w][j]), w                             # the chosen candidate's own bits
    for a in (slow, fstat, power, path, stencil):
        assert not a[n:].any()                                                       # cells beyond nwin are zeros


# ---- against the long-double truth ----

@pytest.mark.parametrize('case', grt.CASES, ids=lambda c: 'N%d-W%d-L%d-R%d-%s-%s' % (c[0], c[1], c[2], c[3], 'noise' if c[4] else 'wave', c[5]))
def test_matches_the_truth(case):
    """Every N of {3, 4, 8, 9, 32}, W of {16, 255, 256, 257, 513}, tap count and level count of {1, 2, 5, 12}, on noise and on
    a wave in noise, grids of 9 and 25 points.  The trace ends one sample behind its last window: the first and the last
    windows read taps off both ends.  The staged form."""
    N, W, taps, levels, noise, gname = case
    grid = grt.GRIDS[gname]
    step = grt.lattice_step(grid)
    data, rij, inc = grt.case_inputs(N, W, noise)
    res = _process(data, rij, W, taps, levels, step, grid=grid)
    n = int(res.nwin[0])
    assert n == 4 and int(res.inc[0]) == inc and res.grid_refined_path.shape == (1, res.vel.shape[1], levels)
    H = _halo(res.xij, N, grid, taps, step)
    assert _hip.load_library().nbls_beam_grid_refine_lds_bytes(N, W, H) == N * (W + 2 * H) * 8
    skipped, total, worst = grt.check_row(data, FS, res.xij, W, inc, n, taps, grid, step, levels, res.grid_index[0], res.grid_fstat[0],
                                          _refined(res), label=repr(case))
    print('%r: %d of %d levels skipped for the path check, worst |dF| / bound %.3g' % (case, skipped, total, worst))
    assert total == n * levels and skipped <= 0.05 * total
    _check_consequences(res, grid, step, levels)


def test_one_level_keeps_the_grid_kernels_own_centre():
    data, rij, _ = grt.case_inputs(8, 257, False)
    res = _process(data, rij, 257, 8, 1)                                             # step None: the grid's lattice step
    n = int(res.nwin[0])
    assert res.grid_refined_stencil[0, :n, 4].tobytes() == res.grid_fstat[0, :n].tobytes()
    _check_consequences(res, GRID5, grt.lattice_step(GRID5), 1)
    assert np.allclose(grt.lattice_step(GRID5), STEP5)
    assert res.handle.refine_levels == 1


def _aligned(fs=16.0, N=5, W=129, npts=700, s=(0.125, -0.0625), noise=1e-4):
    """A broad-band signal that crosses an array of whole-km offsets at a slowness of whole sixteenths s/km: at fs = 16 Hz
    every delay at a grid point of that lattice is a whole sample, so the wave lines up exactly at its own grid point."""
    rij = np.array([[0.0, 1.0, -2.0, 3.0, 0.0], [0.0, 2.0, 1.0, -1.0, -3.0]])[:, :N]
    rng = np.random.default_rng(31)
    sig = np.convolve(rng.standard_normal(npts + 200), np.hanning(9), mode='same')
    xij = planner.co_array(rij)[0]
    d = np.concatenate(([0], np.rint(fs * (xij[:N - 1, 0] * s[0] + xij[:N - 1, 1] * s[1])).astype(int)))
    data = np.stack([sig[100 - d[i]:100 - d[i] + npts] for i in range(N)])           # x_i[t + d_i] = sig[100 + t]
    return np.ascontiguousarray(data + noise * rng.standard_normal(data.shape)), rij, fs


def test_where_no_neighbour_improves_the_grid_maximum_stays():
    """The true slowness on a grid point and a step smaller than the lobe: every path entry is 4 and the three refined
    values are the grid's own bits."""
    data, rij, fs = _aligned()
    ax = np.array([-0.1875, -0.0625, 0.0, 0.125, 0.25])
    grid = np.array([[a, b] for a in ax for b in ax])
    step = np.array([0.03125, 0.03125])
    res = _process(data, rij, 129, 8, 3, step, grid=grid, fs=fs)
    n = int(res.nwin[0])
    want = int(np.flatnonzero((grid[:, 0] == 0.125) & (grid[:, 1] == -0.0625))[0])
    assert n >= 4 and np.all(res.grid_index[0, :n] == want) and np.all(np.isfinite(res.grid_fstat[0, :n]))
    assert np.all(res.grid_refined_path[0, :n] == 4)
    assert res.grid_refined_fstat[0, :n].tobytes() == res.grid_fstat[0, :n].tobytes()
    assert res.grid_refined_power[0, :n].tobytes() == res.grid_power[0, :n].tobytes()
    assert np.all(res.grid_refined_slowness[0, :n] == grid[want])
    assert np.all(res.grid_refined_stencil[0, :n, 4:5] > np.delete(res.grid_refined_stencil[0, :n], 4, axis=1))
    _check_consequences(res, grid, step, 3)


def test_prefix_property():
    """The first l entries of the path of a 3-level plan are the path of an l-level plan, the centres equal bit for bit."""
    data, rij, _ = grt.case_inputs(8, 257, False)
    runs = {R: _process(data, rij, 257, 6, R, STEP5) for R in (1, 2, 3)}
    n = int(runs[3].nwin[0])
    assert np.any(runs[3].grid_refined_path[0, :n] != 4)
    for R in (1, 2):
        _same(runs[R], runs[3], PLAIN + GRID)
        assert np.array_equal(runs[R].grid_refined_path[0, :n], runs[3].grid_refined_path[0, :n, :R])
        for w in range(n):
            centres = grt.replay(GRID5[runs[3].grid_index[0, w]], STEP5, runs[3].grid_refined_path[0, w])
            assert grt.same_bits(runs[R].grid_refined_slowness[0, w], centres[R]), (R, w)
        assert np.all(runs[R].grid_refined_fstat[0, :n] <= runs[3].grid_refined_fstat[0, :n])


# ---- the two forms of the kernel ----

def test_both_forms_give_the_same_bits():
    """N = 4, W = 257: a block of 4 (257 + 2 H) doubles fits 156 KiB up to H = 2367.  One far grid point, never the maximum,
    puts the plan's halo H_r at 2367 (the staged form, at its cap) and at 2368 (the global form); the step, and so every
    candidate, is the same as on the near grid alone (the staged form with a small halo)."""
    N, W, taps, levels = 4, 257, 8, 3
    data, rij, _ = grt.case_inputs(N, W, False)
    xij = planner.co_array(rij)[0]
    lib = _hip.load_library()
    i = int(np.argmax(np.abs(xij[:N - 1, 0])))
    grids = {}
    for target in (2367, 2368):
        for tau in np.arange(target - 60, target + 2) + 0.37:
            g = np.concatenate((GRID5, [[tau / (FS * xij[i, 0]), 0.0]]))
            if _halo(xij, N, g, taps, STEP5) == target:
                grids[target] = g
                break
    assert sorted(grids) == [2367, 2368]
    assert lib.nbls_beam_grid_refine_lds_bytes(N, W, 2367) == N * (W + 2 * 2367) * 8 == 159712
    assert lib.nbls_beam_grid_refine_lds_bytes(N, W, 2368) == 0
    near = _process(data, rij, W, taps, levels, STEP5)
    staged = _process(data, rij, W, taps, levels, STEP5, grid=grids[2367])
    plain = _process(data, rij, W, taps, levels, STEP5, grid=grids[2368])
    n = int(near.nwin[0])
    assert np.all(near.grid_index[0, :n] >= 0) and np.any(near.grid_refined_path[0, :n] != 4)
    for other, label in ((staged, 'staged at the cap'), (plain, 'global')):
        assert np.array_equal(other.grid_index[0, :n], near.grid_index[0, :n]), label          # the far point is never the maximum
        _same(other, near, PLAIN + GRID + REFINED, label)
    _check_consequences(plain, grids[2368], STEP5, levels)
    grt.check_row(data, FS, plain.xij, W, int(plain.inc[0]), n, taps, grids[2368], STEP5, levels, plain.grid_index[0],
                  plain.grid_fstat[0], _refined(plain), label='global')


# ---- the forms of a pass ----

EDGES = [(0.5, 1.5), (1.5, 4.0)]
WINLENS = [257.5 / FS, 65.5 / FS]
FILTER = ('butter', 2, 0.01)
FORM_KW = dict(slowness_grid=GRID5, beam_taps=8, grid_refine=(3, STEP5))
FORM_FIELDS = PLAIN + GRID + REFINED


def _recordings(npts=2401, S=3, N=6):
    rij = synthetic.array_geometry(N, 0.15)
    data = [np.ascontiguousarray(synthetic.plane_wave(rij, npts, FS, 0.5, 4.0, baz_deg=20.0 + 67.0 * i, snr_db=10.0, seed=520 + i))
            for i in range(S)]
    return data, rij - rij.mean(axis=1, keepdims=True), [T0 + 0.0173 * i for i in range(S)]


def _two_bands(data, rij, t0=T0, **kw):
    return engine.process(data, FS, t0, rij, EDGES, WINLENS, 0.5, 0.5, *FILTER, **dict(FORM_KW, **kw))


def test_batch_of_three_recordings_equals_three_single_calls():
    recs, rij, t0s = _recordings()
    batch = engine.process_batch([list(d) for d in recs], FS, t0s, rij, EDGES, WINLENS, 0.5, 0.5, *FILTER, **FORM_KW)
    assert len(batch) == 3
    for s in range(3):
        single = _two_bands(recs[s], rij, t0s[s])
        assert [int(w) for w in single.W] == [257, 65]
        _same(batch[s], single, FORM_FIELDS, 'recording %d' % s)
        for row in (0, 1):
            _check_consequences(single, GRID5, STEP5, 3, row)
    assert not np.array_equal(batch[0].grid_refined_fstat, batch[1].grid_refined_fstat)
    assert np.any(batch[0].grid_refined_path[batch[0].grid_index >= 0] != 4)
    # ... and without the request the pass returns what it returned, and carries no refined field
    off = _two_bands(recs[0], rij, t0s[0], grid_refine=None)
    _same(off, batch[0], PLAIN + GRID)
    assert not any(hasattr(off, k) for k in REFINED)


def test_streamed_overlapped_and_two_round_passes_equal_the_plain_pass(monkeypatch):
    recs, rij, _ = _recordings(24001, 1)
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    whole = _two_bands(recs[0], rij)
    h = engine.get_handle()
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '1')
    for overlap in (1, -1):
        try:
            h.set_option('screen_batch_mb', 1)
            h.set_option('solve_min_units', 1)
            h.set_option('overlap', overlap)
            streamed = _two_bands(recs[0], rij)
            nbatches = h.result_batches()
        finally:
            h.set_option('screen_batch_mb', 192)
            h.set_option('solve_min_units', 0)
            h.set_option('overlap', 0)
        assert nbatches >= 3, nbatches
        _same(streamed, whole, FORM_FIELDS, 'streamed, overlap %d' % overlap)
    # two HBM rounds of one band each
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', repr(1.5 * 8.0 * 6 * (24001 + 64) / 2.0 ** 30))
    assert engine.max_bands_per_pass(6, 24001) == 1
    rounds = _two_bands(recs[0], rij)
    _same(rounds, whole, FORM_FIELDS, 'two rounds')


def test_two_window_slices_add_up_to_the_full_call():
    data, rij, _ = grt.case_inputs(6, 65, False, seed=44)
    data = np.ascontiguousarray(np.tile(data, 3))
    full = _process(data, rij, 65, 8, 3, STEP5)
    parts = [_process(data, rij, 65, 8, 3, STEP5, window_slice=(k, 2)) for k in range(2)]
    n = int(full.nwin[0])
    assert n >= 8
    c0, c1 = (p.grid_refined_fstat[0, :n] != 0 for p in parts)                       # the cells a slice computed
    assert c0.any() and c1.any() and np.all(c0 ^ c1) and np.flatnonzero(c0).max() < np.flatnonzero(c1).min()
    for k in REFINED + GRID:
        a, b, f = getattr(parts[0], k)[0, :n], getattr(parts[1], k)[0, :n], getattr(full, k)[0, :n]
        assert not a[~c0].any() and not b[~c1].any(), k                              # outside a window slice: zeros
        both = np.where(c0.reshape((-1,) + (1,) * (a.ndim - 1)), a, b)
        assert both.tobytes() == f.tobytes() or np.array_equal(both, f, equal_nan=True), k


def test_a_pass_of_one_unit():
    """One workgroup per unit: a pass of a single unit."""
    N, W = 4, 65
    data, rij, inc = grt.case_inputs(N, W, False, seed=45)
    short = np.ascontiguousarray(data[:, :W + 1])
    one = _process(short, rij, W, 8, 2, STEP5)
    assert int(one.nwin[0]) == 1 and one.grid_index[0, 0] >= 0
    _check_consequences(one, GRID5, STEP5, 2)
    grt.check_row(short, FS, one.xij, W, inc, 1, 8, GRID5, STEP5, 2, one.grid_index[0], one.grid_fstat[0], _refined(one), label='one unit')


def test_one_unit_more_than_a_unit_batch_holds(monkeypatch):
    """8 elements x W = 600 with ``screen_batch_mb`` 1: a unit batch holds 107 units (``unit_count_cases.screen_batches``).
    A streamed pass of 108 units runs as two batches, so the kernel is launched a second time with a first unit other
    than 0: bit-equal to the pass in one piece."""
    import unit_count_cases as uc
    N, W, inc = 8, 600, 100
    WP = (W + 15) // 16 * 16
    capacity = max(64, (1 << 20) // (N * 2 * WP))
    nu = capacity + 1
    batches = uc.screen_batches(nu, N, WP, 1)
    assert capacity == 107 and uc.screen_batches(capacity, N, WP, 1) == [capacity] and batches == [56, 52]
    rij = synthetic.array_geometry(N, 0.15)
    data = np.ascontiguousarray(synthetic.plane_wave(rij, W + (nu - 1) * inc + 1, FS, 0.5, 4.0, baz_deg=60.0, snr_db=6.0, seed=48))
    rij = rij - rij.mean(axis=1, keepdims=True)
    kw = dict(alpha=0.5, overlap=1.0 - inc / float(W))
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    whole = _process(data, rij, W, 8, 2, STEP5, **kw)
    assert int(whole.nwin[0]) == nu and int(whole.inc[0]) == inc
    h = engine.get_handle()
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '1')
    try:
        h.set_option('screen_batch_mb', 1)
        h.set_option('solve_min_units', 1)
        h.set_option('result_tail_units', -1)
        streamed = _process(data, rij, W, 8, 2, STEP5, **kw)
        assert h.result_batches() == len(batches), (h.result_batches(), batches)
        ranges = [tuple(int(v) for v in h.wait_result_batch(k)[:2]) for k in range(h.result_batches())]
    finally:
        h.set_option('screen_batch_mb', 192)
        h.set_option('solve_min_units', 0)
        h.set_option('result_tail_units', 0)
    assert ranges == [(0, 56), (56, 108)], ranges
    _same(streamed, whole, FORM_FIELDS, 'one unit more than a batch')
    _check_consequences(whole, GRID5, STEP5, 2)
    assert np.any(whole.grid_refined_path[0, 56:nu] != 4)


def test_a_candidate_has_the_bits_of_a_grid_point_of_its_slowness():
    """Every candidate of a level, placed as a grid point of a second plan: that plan's map holds the bits of the stencil
    (the centre's among them, which are the first plan's ``grid_fstat``)."""
    data, rij, _ = grt.case_inputs(8, 257, False)
    for taps in (4, 6, 8):
        first = _process(data, rij, 257, taps, 1, STEP5)
        n = int(first.nwin[0])
        assert np.all(first.grid_index[0, :n] >= 0)
        second_grid = np.concatenate([grt.candidates(GRID5[first.grid_index[0, w]], STEP5, 1) for w in range(n)])
        second = engine.process(data, FS, T0, rij, [(None, None)], [257.5 / FS], 0.5, 1.0, prefiltered=True,
                                slowness_grid=second_grid, want_grid_map=True, beam_taps=taps)
        for w in range(n):
            got = second.grid_map[0, w, 9 * w:9 * w + 9]
            assert got.tobytes() == first.grid_refined_stencil[0, w].tobytes(), (taps, w, got, first.grid_refined_stencil[0, w])
        assert np.all(np.isfinite(first.grid_refined_stencil[0, :n]))


def test_a_second_estimator_gets_no_refined_results():
    """Estimator 0 only, as for the grid: the refined results of a pass of two estimators are those of the single call."""
    N, W = 6, 257
    data, rij, _ = grt.case_inputs(N, W, False, seed=46)
    keep = [0, 1, 3, 4, 5]
    h = engine.get_handle()
    prep0 = engine.prepare(N, data.shape[1], FS, rij, [(None, None)], [(W + 0.5) / FS], 0.5, 1.0, prefiltered=True)
    xij1, pair1, xpinv1 = planner.co_array(np.ascontiguousarray(rij[:, keep]))
    engine.launch(h, list(data), prep0, beam_grid=GRID5, beam_taps=8, grid_refine=(3, STEP5),
                  estimators=[dict(lts=None, kept=keep, xij=xij1, pair_idx=pair1, xpinv=xpinv1, eig6=None)])
    h.sync()
    multi = h.fetch_beam_grid_refined()
    h.set_estimators(())
    single = _process(data, rij, W, 8, 3, STEP5)
    n = int(single.nwin[0])
    for got, k in zip(multi, REFINED):
        assert got[0, :n].tobytes() == getattr(single, k)[0, :n].tobytes(), k


# ---- special values ----

def test_a_window_of_zeros_has_no_refined_maximum():
    N, W = 4, 65
    data, rij, inc = grt.case_inputs(N, W, False, seed=47)
    data = np.ascontiguousarray(np.tile(data, 3))
    data[:, 2 * inc - 40:2 * inc + W + 40] = 0.0                                     # window 2 and every tap of it
    res = _process(data, rij, W, 8, 4, STEP5)
    n = int(res.nwin[0])
    assert res.grid_index[0, 2] == -1 and np.count_nonzero(res.grid_index[0, :n] == -1) == 1
    assert np.all(np.isnan(res.grid_refined_slowness[0, 2])) and np.isnan(res.grid_refined_fstat[0, 2])
    assert np.isnan(res.grid_refined_power[0, 2]) and np.all(np.isnan(res.grid_refined_stencil[0, 2]))
    assert np.all(res.grid_refined_path[0, 2] == -1) and res.grid_refined_path.dtype == np.int32
    _check_consequences(res, GRID5, STEP5, 4)


def test_a_nan_sample_in_one_candidates_reach_only():
    """Three elements whose second lies on the diagonal: of the level's candidates only one corner reaches furthest behind
    the window in that element's row.  A NaN there is read by that candidate alone (and by grid points further out): its F
    is NaN, it is never chosen, and the other seven have their ratio."""
    fs, W, taps, K = 16.0, 64, 8, 4
    rij = np.array([[0.0, 4.0, -3.0], [0.0, 4.0, 2.0]])
    rng = np.random.default_rng(9)
    sig = np.convolve(rng.standard_normal(600), np.hanning(9), mode='same')
    clean = np.ascontiguousarray(sig[None, :] + 0.05 * rng.standard_normal((3, 600)))
    ax = np.array([-1.0, 0.0, 1.0])
    grid = np.array([[a, b] for a in ax for b in ax])
    step = np.array([1.0, 1.0])
    first = _process(clean, rij, W, taps, 1, step, grid=grid, fs=fs)
    assert first.grid_index[0, 0] == 4 and np.all(np.isfinite(first.grid_refined_stencil[0, 0]))
    cand = grt.candidates(grid[4], step, 1)
    hi = np.array([W - 1 + grt.delays_of(first.xij, cand[j], fs, 3)[0][1] + K for j in range(9)])       # element 1, window 0
    jn = int(np.argmax(hi))
    assert jn != 4 and np.count_nonzero(hi == hi[jn]) == 1 and hi[jn] > W - 1 + K
    data = clean.copy()
    data[1, hi[jn]] = np.nan
    res = _process(data, rij, W, taps, 1, step, grid=grid, fs=fs)
    st = res.grid_refined_stencil[0, 0]
    assert res.grid_index[0, 0] == 4 and res.grid_fstat[0, 0].tobytes() == first.grid_fstat[0, 0].tobytes()
    assert np.isnan(st[jn]) and not np.any(np.isnan(np.delete(st, jn))) and res.grid_refined_path[0, 0, 0] != jn
    assert np.delete(st, jn).tobytes() == np.delete(first.grid_refined_stencil[0, 0], jn).tobytes()
    # ... and where the NaN-free run chose that very candidate, the run with the NaN takes the best of the others
    others = [j for j in range(9) if j != jn]
    assert res.grid_refined_path[0, 0, 0] == grt.choose([st[j] if j in others else np.nan for j in range(9)], st[4])


def test_a_candidate_with_an_infinite_ratio_is_chosen():
    """Identical traces of small whole numbers: at slowness 0 every sum is exact and D = 0, F = +inf.  The grid holds the eight
    neighbours of 0 at half a step and one far point, not 0 itself: 0 is a candidate of level 1 of whichever of them is
    the maximum, is chosen, and stays through level 2."""
    N, W = 3, 130
    rng = np.random.default_rng(11)
    sig = np.rint(40.0 * np.convolve(rng.standard_normal(700), np.hanning(33), mode='same'))
    data = np.ascontiguousarray(np.tile(sig, (N, 1)))
    rij = synthetic.array_geometry(N, 0.15)
    rij = rij - rij.mean(axis=1, keepdims=True)
    grid = np.array([[a, b] for a in (-0.5, 0.0, 0.5) for b in (-0.5, 0.0, 0.5) if (a, b) != (0.0, 0.0)] + [[3.0, 3.0]])
    step = np.array([1.0, 1.0])
    res = _process(data, rij, W, 8, 2, step, grid=grid)
    n = int(res.nwin[0])
    assert n >= 4 and np.all(res.grid_index[0, :n] >= 0) and np.all(res.grid_index[0, :n] < 8)
    assert np.all(np.isfinite(res.grid_fstat[0, :n]))
    for w in range(n):
        g = grid[res.grid_index[0, w]]
        cand = grt.candidates(g, step, 1)
        j0 = [j for j in range(9) if j != 4 and cand[j, 0] == 0.0 and cand[j, 1] == 0.0]
        assert len(j0) == 1
        assert list(res.grid_refined_path[0, w]) == [j0[0], 4], (w, res.grid_refined_path[0, w])
        assert res.grid_refined_fstat[0, w] == np.inf and np.all(res.grid_refined_slowness[0, w] == 0.0)
        assert res.grid_refined_stencil[0, w, 4] == np.inf and np.all(np.isfinite(np.delete(res.grid_refined_stencil[0, w], 4)))
        assert res.grid_refined_power[0, w] == np.sum(sig[w * int(res.inc[0]):w * int(res.inc[0]) + W] ** 2) / W


# ---- off again, refusals ----

def test_off_after_on_gives_the_bits_of_a_handle_that_never_asked():
    data, rij, _ = grt.case_inputs(4, 257, False)
    first = _process(data, rij, 257, 8, 0)
    on = _process(data, rij, 257, 8, 4, STEP5)
    again = _process(data, rij, 257, 8, 0)
    _same(first, again, PLAIN + GRID)
    _same(first, on, PLAIN + GRID)
    h = again.handle
    assert h.refine_levels == 0
    with pytest.raises(_hip.NblsError) as err:
        h.fetch_beam_grid_refined()
    assert err.value.code == _hip.NBLS_ERR_STATE


def test_refusals_of_the_library():
    h = engine.get_handle()
    data, rij, _ = grt.case_inputs(4, 65, False)
    xij, pair_idx, xpinv = planner.co_array(rij)
    h.set_trace(data, FS)
    h.set_geometry(xij, pair_idx, xpinv)
    plan = lambda: h.plan(None, False, None, None, [65], [32], 40)
    try:
        for levels, step in ((13, (1.0, 1.0)), (-1, (1.0, 1.0)), (4, (0.0, 1.0)), (4, (1.0, np.nan)), (4, (np.inf, 1.0)), (4, (-1.0, 1.0))):
            with pytest.raises(ValueError) as err:
                h.set_beam_grid_refinement(levels, step)
            assert err.value.code == _hip.NBLS_ERR_ARG
        h.set_beam_grid_refinement(4, (1.0, 1.0))
        with pytest.raises(_hip.NblsError) as err:                                   # no grid
            plan()
        assert err.value.code == _hip.NBLS_ERR_STATE and 'nbls_set_beam_grid_refinement' in str(err.value)
        h.set_beam_grid(GRID5)
        with pytest.raises(_hip.NblsError) as err:                                   # no taps: F is piecewise constant
            plan()
        assert err.value.code == _hip.NBLS_ERR_STATE and 'nbls_set_beam_interpolation' in str(err.value)
        h.set_beam_interpolation(8)
        plan()
        h.set_lag_seed([3])
        with pytest.raises(ValueError) as err:                                       # a seed keeps the unrefined maximum
            plan()
        assert err.value.code == _hip.NBLS_ERR_UNSUPPORTED and 'nbls_set_lag_seed' in str(err.value)
        h.set_lag_seed(None)
        # a setter that refuses changes nothing: the next plan still refines with 4 levels
        with pytest.raises(ValueError):
            h.set_beam_grid_refinement(13, (1.0, 1.0))
        plan()
        h.execute()
        h.sync()
        out = h.fetch_beam_grid_refined()
        assert out[3].shape[-1] == 4 and np.any(out[3] >= 0) and h.refine_levels == 4
        # a delay bound of 2^30 samples
        xmax = float(np.abs(xij[:3]).sum(axis=1).max())
        h.set_beam_grid_refinement(1, (2.0 ** 30 / FS / xmax, 2.0 ** 30 / FS / xmax))
        with pytest.raises(ValueError) as err:
            plan()
        assert err.value.code == _hip.NBLS_ERR_ARG and '2^30' in str(err.value)
        h.set_beam_grid_refinement(0, None)
        plan()
        with pytest.raises(_hip.NblsError) as err:
            h.fetch_beam_grid_refined()
        assert err.value.code == _hip.NBLS_ERR_STATE
    finally:
        h.set_lag_seed(None)
        h.set_beam_grid_refinement(0, None)
        h.set_beam_interpolation(0)
        h.set_beam_grid(None)
    plan()


def test_rccl_communicator_refuses_a_refining_plan():
    """A communicator lives as long as its process: a child process over the tests' loopback transport."""
    src = os.path.join(ROOT, 'tests', 'c_caller', 'loopback_rccl.cpp')
    lib = os.path.join(ROOT, 'tests', 'c_caller', 'libloopback_rccl.so')
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.run(['/opt/rocm/bin/hipcc', '-O2', '-shared', '-fPIC', '--offload-arch=gfx950', src, '-o', lib], check=True,
                       timeout=300)
    env = dict(os.environ, NBLS_TEST_TRANSPORT=lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_grid_refine_comm_worker.py')], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and 'GRID_REFINE_COMM_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the demonstration and the public entry points ----

@pytest.fixture(scope='module')
def demo():
    d = stt.demonstration()
    d['data'] = np.ascontiguousarray(d['filt'][:, 300:])                             # windows of 400 samples every 600
    d['st'] = synthetic.make_stream(d['data'], d['fs'], starttime=T0)
    ax = np.arange(-5, 6) * 0.8
    d['coarse'] = np.ascontiguousarray(np.stack(np.meshgrid(ax, ax, indexing='ij'), axis=-1).reshape(-1, 2))
    return d


def test_public_entry_points_on_the_demonstration_trace(demo):
    """11 x 11 points at 0.8 s/km and 4 levels against the 41 x 41 grid at 0.2 s/km, 8 taps: the statements of
    tests/test_grid_refine_truth.py on the GPU's results."""
    d = demo
    st, rij, coarse = d['st'], d['rij'], d['coarse']
    wl, ov = 400.5 / d['fs'], 1.0 - 600.0 / 400.0
    out = ltsva_grid_refined(st, None, None, wl, ov, coarse, rij=rij)
    assert len(out) == 8 + 5 + 7 and len(out[0]) >= 8
    gvel, gbaz, gF, gP, gidx = out[8:13]
    rvel, rbaz, rslow, rF, rP, rpath, rst = out[13:]
    assert rslow.shape == (len(gidx), 2) and rpath.shape == (len(gidx), 4) and rpath.dtype == np.int32 and rst.shape == (len(gidx), 9)
    assert np.all(gidx >= 0) and np.all(rF >= gF)
    step = planner.grid_cells(coarse)[1]
    assert np.allclose(step, 0.8)
    for w in range(len(gidx)):
        assert grt.same_bits(rslow[w], grt.replay(coarse[gidx[w]], step, rpath[w])[-1])
    with np.errstate(divide='ignore'):
        assert np.array_equal(rvel, 1.0 / np.hypot(rslow[:, 0], rslow[:, 1]))
    assert np.array_equal(rbaz, np.mod(np.arctan2(rslow[:, 0], rslow[:, 1]) * 180.0 / np.pi - 360.0, 360.0))
    plain = ltsva_grid(st, None, None, wl, ov, coarse, rij=rij)
    for i in range(8):
        assert np.array_equal(out[i], plain[i], equal_nan=True) if not isinstance(out[i], dict) else out[i] == plain[i]
    fine = ltsva_steered(st, None, None, wl, ov, rij=rij, slowness_grid=d['grid'])
    fidx, fF = fine[14], fine[12]
    err = small_array_statements(d['true'], (d['grid'][fidx[:8]], fF[:8]), (coarse[gidx[:8]], gF[:8]), (rslow[:8], rF[:8]))
    print('100 m array, 8 taps, 8 windows: slowness error median %.3f (41 x 41) %.3f (11 x 11) %.3f (11 x 11 + 4 levels) s/km; '
          'median F %.1f, %.1f, %.1f' % (np.median(err['fine']), np.median(err['coarse']), np.median(err['refined']),
                                         np.median(fF[:8]), np.median(gF[:8]), np.median(rF[:8])))
    # levels, step and taps reach the plan
    two = ltsva_grid_refined(st, None, None, wl, ov, coarse, rij=rij, levels=2, step=(0.4, 0.4), taps=4, grid_map=True)
    assert len(two) == 21 and two[13].shape == (len(gidx), len(coarse)) and two[19].shape == (len(gidx), 2)
    # the batch: three recordings, bit for bit
    sts = [st, synthetic.make_stream(d['data'][:, ::-1].copy(), d['fs'], starttime=T0), st]
    batch = ltsva_grid_refined_batch(sts, None, None, wl, ov, coarse, rij=rij)
    assert len(batch) == 3
    for s, b in zip(sts, batch):
        single = ltsva_grid_refined(s, None, None, wl, ov, coarse, rij=rij)
        assert len(b) == len(single) == 20
        for x, y in zip(b, single):
            assert (x == y) if isinstance(x, dict) else np.array_equal(x, y, equal_nan=True)
    # the narrow-band call: two bands filtered on the GPU
    raw = synthetic.make_stream(synthetic.plane_wave(rij, 6001, 20.0, 0.1, 8.0, baz_deg=225, vel_kms=0.34, snr_db=6.0), 20.0,
                                starttime=T0)
    freqlist, NBANDS, _ = get_freqlist(0.5, 4.0, 'log', 2)
    WINLEN_list = get_winlenlist('adaptive', NBANDS, 20, 30, 20)
    fr = np.logspace(-2, 1, 16)
    args = (WINLEN_list, 0.5, 1.0, raw, None, None, NBANDS, np.zeros(16), np.zeros(16), freqlist, 'log', fr, 'butter', 2, 0.01)
    got = narrow_band_least_squares_grid_refined(*args, rij=rij, slowness_grid=coarse[::2], step=(1.6, 1.6))
    exp = narrow_band_least_squares_grid(*args, rij=rij, slowness_grid=coarse[::2])
    assert len(got) == 9 + 5 + 7 and len(exp) == 14
    for i in (0, 1, 2, 3, 5, 7, 8):
        np.testing.assert_array_equal(got[i], exp[i], err_msg='return %d' % i)
    nwin = np.asarray(got[6])
    gF, gidx, rslow, rF, rpath = got[11], got[13], got[16], got[17], got[19]
    assert rpath.shape == gidx.shape + (4,) and rslow.shape == gidx.shape + (2,) and got[20].shape == gidx.shape + (9,)
    for b in range(NBANDS):
        n = int(nwin[b])
        assert np.all(rF[b, :n] >= gF[b, :n]) and not rF[b, n:].any() and not got[14][b, n:].any() and not rpath[b, n:].any()
        for w in range(n):
            assert grt.same_bits(rslow[b, w], grt.replay(coarse[::2][gidx[b, w]], (1.6, 1.6), rpath[b, w])[-1])
