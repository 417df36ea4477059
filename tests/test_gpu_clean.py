"""The CLEAN-SC components (``nbls_set_capon_clean``, csrc/capon_clean.hip: capon_clean_kernel) against
tests/clean_truth.py: one iteration at a time in long double from the GPU's own R_i (a plan with ``iterations = i`` and the
residual matrix; the prefix property makes that the same computation), with bounds that are derived, never fitted; the tests
print the worst |difference| / bound.  Between the forms of a pass every output is equal bit for bit.  All cases use
prefiltered traces at fs = 20 Hz (tests/clean_cases.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import capon_truth as ct
import clean_cases as cc
import clean_truth as clt
import peaks_truth as pt
from test_clean_truth import STRAY, demo_case, demo_patch, found_every_source, peak_lists_find, source_powers
from narrow_band_least_squares_amd import (engine, planner, synthetic, _hip, ltsva, ltsva_clean, ltsva_clean_batch,
                                           narrow_band_least_squares_clean, clean_sources)

pytestmark = pytest.mark.gpu

FS, FREQ, FLOOR = cc.FS, cc.FREQ, cc.FLOOR
T0 = 17884.0729166667
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLEAN = ('clean_count', 'clean_index', 'clean_power', 'clean_total', 'clean_residual')
CAPON = ('capon_index', 'capon_power', 'bartlett_index', 'bartlett_power')
PLAIN = ('vel', 'baz', 'mdccm', 'sigma_tau', 'mask')


def _process(data, rij, W, Ls, Hs, grid, clean, alpha=1.0, overlap=0.5, csdm=True, **kw):
    res = engine.process(data, FS, T0, rij, [(None, None)], [(W + 0.5) / FS], overlap, alpha, prefiltered=True, capon_grid=grid,
                         capon_freqs=[FREQ], capon_snapshots=(Ls, Hs), want_capon_csdm=csdm, capon_clean=clean, **kw)
    assert int(res.W[0]) == W
    return res


def _same(a, b, keys, label=''):
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        assert x is not None and y is not None, (label, k)
        assert pt.same_bits(x, y), (label, k)


def _check_invariants(res, label=''):
    """What holds for every result: ranks below the count are grid points with a positive power, -1 / NaN beyond; rank 0 is
    the Bartlett maximum; total >= residual >= 0 up to rounding; zeros beyond the band's windows."""
    for b in range(len(res.nwin)):
        n, I = int(res.nwin[b]), res.clean_index.shape[2]
        for w in range(n):
            c = int(res.clean_count[b, w])
            assert 0 <= c <= I, (label, b, w, c)
            assert np.all(res.clean_index[b, w, :c] >= 0) and np.all(res.clean_power[b, w, :c] > 0), (label, b, w)
            assert np.all(res.clean_index[b, w, c:] == -1) and np.all(np.isnan(res.clean_power[b, w, c:])), (label, b, w)
            if c:
                assert res.clean_residual[b, w] <= res.clean_total[b, w] * (1 + 1e-12) and res.clean_residual[b, w] >= -1e-12 * res.clean_total[b, w]
        for k in CLEAN:
            assert not getattr(res, k)[b, n:].any(), (label, k)


def _one_step_walk(label, base, runs, steer, gain, rows_of=None):
    """The one-step check of every window: ``base`` the plan without a request (R_0), ``runs[i]`` the plan with I = i + 1 and the
    residual matrix.  ``rows_of(w)``: the kept elements of window w (KEPT plans: the matrices and the table are compacted to
    them, as the kernel does) -> (windows, updates checked, worst |dR| / bound, waived stop decisions)."""
    n = int(base.nwin[0])
    worst, waived, taken = 0.0, 0, 0
    for w in range(n):
        rows = list(range(base.capon_csdm.shape[2])) if rows_of is None else rows_of(w)
        pick = lambda R: R[np.ix_(rows, rows)]
        a = steer[:, rows]
        p0 = tol0 = None
        eig = 0.0
        for i in range(len(runs)):
            run = runs[i]                                            # the plan with I = i + 1
            full_i = base.capon_csdm[0, w] if i == 0 else runs[i - 1].clean_csdm[0, w]
            R_i = pick(full_i)
            if i > 0 and runs[i - 1].clean_count[0, w] < i:
                assert run.clean_count[0, w] == runs[i - 1].clean_count[0, w]       # stopped before: nothing further happens
                assert pt.same_bits(run.clean_csdm[0, w], full_i)
                continue
            stopped = bool(run.clean_count[0, w] < i + 1)
            lab = '%s w=%d i=%d' % (label, w, i)
            R_n = pick(run.clean_csdm[0, w])
            st = clt.check_step(lab, R_i, a, gain, FLOOR, i, p0, tol0, stopped, int(run.clean_index[0, w, i]),
                                float(run.clean_power[0, w, i]), R_n)
            waived += st['waived']
            if i == 0:
                p0, tol0 = st['p'], st['tol']
            if stopped:
                assert pt.same_bits(R_n, R_i)
                continue
            taken += 1
            worst = max(worst, st['worst'])
            eig += 2.0 * float(st['tolR'].sum())
            assert np.array_equal(R_n, np.conj(R_n.T)) and not R_n.imag.diagonal().any()
            clt.invariants(lab, R_i, R_n, st['tolR'], eig)
    return n, taken, worst, waived


@pytest.mark.parametrize('W,Ls,Hs', cc.SHAPES)
@pytest.mark.parametrize('gain', cc.GAINS)
@pytest.mark.parametrize('G', cc.GRID_SIZES)
@pytest.mark.parametrize('N', cc.ELEMENTS)
def test_one_step_against_the_truth(N, G, gain, W, Ls, Hs):
    data, rij = cc.traces(N, W)
    grid = cc.grid(G)
    base = _process(data, rij, W, Ls, Hs, grid, None)
    runs = [_process(data, rij, W, Ls, Hs, grid, (i, gain, FLOOR, True)) for i in range(1, cc.STEPS + 1)]
    _, steer = runs[0].handle.fetch_capon_tables(0)
    assert int(base.nwin[0]) >= 4
    n, taken, worst, waived = _one_step_walk('N=%d G=%d' % (N, G), base, runs, steer, gain)
    print('one step N=%d G=%d gain=%g W=%d Ls=%d Hs=%d: %d windows, %d updates, worst |dR| / bound %.3g, %d stop decisions waived'
          % (N, G, gain, W, Ls, Hs, n, taken, worst, waived))
    assert taken >= n and 100 * waived <= n


@pytest.mark.parametrize('N,G', [(3, 129), (8, 1257), (32, 128)])
def test_rank_zero_is_the_bartlett_maximum_and_the_prefix_property(N, G):
    data, rij = cc.traces(N, 65)
    grid = cc.grid(G)
    runs = {I: _process(data, rij, 65, 16, 8, grid, (I, 0.5, FLOOR, True)) for I in (1, 2, 5, 32)}
    n = int(runs[32].nwin[0])
    full = runs[32]
    for I, res in runs.items():
        _check_invariants(res, 'I=%d' % I)
        assert pt.same_bits(res.clean_index[0, :n, 0], res.bartlett_index[0, :n])
        assert pt.same_bits(res.clean_power[0, :n, 0], 0.5 * res.bartlett_power[0, :n])
        assert pt.same_bits(res.clean_index[0, :, :I], full.clean_index[0, :, :I].copy())
        assert pt.same_bits(res.clean_power[0, :, :I], full.clean_power[0, :, :I].copy())
        assert np.array_equal(res.clean_count[0], np.minimum(full.clean_count[0], I))
        assert pt.same_bits(res.clean_total, full.clean_total)
        _same(res, full, CAPON + PLAIN, 'I=%d' % I)
    assert np.all(np.diff(np.stack([runs[I].clean_residual[0, :n] for I in (1, 2, 5, 32)]), axis=0) <= 0)


@pytest.mark.parametrize('N', cc.ELEMENTS)
def test_32_iterations_without_a_floor(N):
    data, rij = cc.traces(N, 65)
    res = _process(data, rij, 65, 16, 8, cc.grid(129), (32, 0.5, 0.0, True))
    n = int(res.nwin[0])
    _check_invariants(res)
    assert np.all(res.clean_count[0, :n] == 32)
    for w in range(n):
        ev = np.linalg.eigvalsh(res.clean_csdm[0, w])
        assert ev[0] >= -1e-10 * np.trace(res.capon_csdm[0, w]).real
        assert np.all(np.diff(res.clean_power[0, w]) <= 1e-12 * res.clean_power[0, w, 0])     # with one gain the maxima descend


def test_one_wave_at_a_grid_point_stops_after_one_component():
    grid = cc.grid(129)
    for N in (3, 8):
        data, rij = cc.single_wave(N, 257, 17, grid)
        res = _process(data, rij, 257, 64, 16, grid, (8, 1.0, FLOOR, True))
        n = int(res.nwin[0])
        _check_invariants(res)
        assert np.all(res.clean_count[0, :n] == 1) and np.all(res.clean_index[0, :n, 0] == 17)
        np.testing.assert_allclose(res.clean_power[0, :n, 0], res.clean_total[0, :n], rtol=1e-6)       # (the leakage: clean_cases.single_wave)
        assert np.all(res.clean_residual[0, :n] <= 1e-6 * res.clean_total[0, :n])


def test_degenerate_units():
    data, rij = cc.traces(4, 65, seed=3)
    data = np.tile(data, (1, 4))
    grid = cc.grid(129)
    good = _process(data, rij, 65, 16, 8, grid, (4, 0.5, FLOOR, True))
    n, inc = int(good.nwin[0]), int(good.inc[0])
    gap = data.copy()
    gap[:, 400:800] = 0.0
    res = _process(gap, rij, 65, 16, 8, grid, (4, 0.5, FLOOR, True))
    cover = (ct.snapshot_count(65, 16, 8) - 1) * 8 + 16              # the samples of a window its snapshots read: 64 of the 65
    empty = np.array([w * inc >= 400 and w * inc + cover <= 800 for w in range(n)])
    assert empty.sum() >= 3
    assert np.all(res.clean_count[0, :n][empty] == 0) and np.all(res.clean_index[0, :n][empty] == -1)
    for k in ('clean_power', 'clean_total', 'clean_residual'):
        assert np.all(np.isnan(getattr(res, k)[0, :n][empty])) and np.all(np.isfinite(getattr(res, k)[0, :n][~empty][..., :1]))
    assert not res.clean_csdm[0, :n][empty].any()                    # R_0 of an all-zero window
    bad = data.copy()
    bad[1, 1000] = np.nan
    res = _process(bad, rij, 65, 16, 8, grid, (4, 0.5, FLOOR, True))
    hit = np.array([w * inc <= 1000 < w * inc + cover for w in range(n)])
    assert 1 <= hit.sum() <= 3
    assert np.all(res.clean_count[0, :n][hit] == 0) and np.all(np.isnan(res.clean_total[0, :n][hit]))
    for k in CLEAN + ('clean_csdm',):
        assert pt.same_bits(getattr(res, k)[0, :n][~hit], getattr(good, k)[0, :n][~hit]), k
    _check_invariants(good)


def test_a_grid_of_one_point():
    data, rij = cc.traces(4, 65)
    res = _process(data, rij, 65, 16, 8, cc.grid(1), (3, 0.5, 0.0, False))
    n = int(res.nwin[0])
    assert res.clean_csdm is None
    assert np.all(res.clean_count[0, :n] == 3) and np.all(res.clean_index[0, :n] == 0)
    p = res.clean_power[0, :n]
    np.testing.assert_allclose(p[:, 1], 0.5 * p[:, 0], rtol=1e-12)   # the same beam again: half of what the first left
    np.testing.assert_allclose(p[:, 2], 0.25 * p[:, 0], rtol=1e-12)


def _mistimed(N, npts, bad, seed=900):
    rij = synthetic.array_geometry(N, 1.0)
    data = synthetic.plane_wave(rij, npts, FS, 0.5, 4.0, baz_deg=60.0, snr_db=10.0, seed=seed,
                                timing_error_s=0.25 if bad is not None else 0.0, bad_element=bad)
    return np.ascontiguousarray(data), rij - rij.mean(axis=1, keepdims=True)


@pytest.mark.parametrize('bad', [0, 3, 7])
def test_kept_elements_on_an_lts_plan(bad):
    """The KEPT instance held to (b)'s derived bounds, one step at a time from its own R_i: the matrices and the steering
    table compacted to the elements of the unit's mask, M in the place of N; the residual matrix scattered back with zeros
    for the dropped element; total and residual the mean of the compacted diagonal."""
    N, W, I = 8, 257, 5
    data, rij = _mistimed(N, W * 4 + 1, bad)
    grid = cc.grid(129)
    kw = dict(alpha=0.5, kept=(N - 1, False, True))
    base = _process(data, rij, W, 64, 16, grid, None, **kw)
    runs = [_process(data, rij, W, 64, 16, grid, (i, 0.5, FLOOR, True), **kw) for i in range(1, I + 1)]
    res = runs[-1]
    n = int(res.nwin[0])
    _check_invariants(res)
    _, steer = res.handle.fetch_capon_tables(0)
    for run in runs:
        assert pt.same_bits(run.dropped_mask, base.dropped_mask) and pt.same_bits(run.capon_csdm, base.capon_csdm)
    assert np.any(res.dropped_mask[0, :n] == 1 << bad)
    assert pt.same_bits(res.clean_index[0, :n, 0], res.bartlett_index[0, :n])
    rows_of = lambda w: clt.kept_rows(int(res.dropped_mask[0, w]), N)
    n, taken, worst, waived = _one_step_walk('kept, element %d late' % bad, base, runs, steer, 0.5, rows_of)
    print('KEPT, element %d late: %d windows, %d updates, worst |dR| / bound %.3g, %d stop decisions waived' % (bad, n, taken, worst, waived))
    assert taken >= n and 100 * waived <= n
    for w in range(n):
        rows = rows_of(w)
        gone = [e for e in range(N) if e not in rows]
        for run in runs:
            assert not run.clean_csdm[0, w][gone].any() and not run.clean_csdm[0, w][:, gone].any()
        M = len(rows)
        t0 = tr = 0.0
        for e in rows:                                               # ascending, as the definition sums
            t0 += base.capon_csdm[0, w][e, e].real
            tr += res.clean_csdm[0, w][e, e].real
        assert res.clean_total[0, w] == t0 / M and res.clean_residual[0, w] == tr / M


def test_kept_falls_back_to_the_array_and_nothing_dropped_gives_the_plain_bits():
    N, W = 4, 65
    data, rij = _mistimed(N, W * 8 + 1, 3)
    grid = cc.grid(129)
    plain = _process(data, rij, W, 16, 8, grid, (4, 0.5, FLOOR, True), alpha=0.5)
    # q = 1: every element that lost a pair is named; where fewer than 3 remain the kept set is the whole array
    kept = _process(data, rij, W, 16, 8, grid, (4, 0.5, FLOOR, True), alpha=0.5, kept=(1, False, True))
    n = int(plain.nwin[0])
    whole = np.array([len(clt.kept_rows(int(m), N)) == N for m in kept.dropped_mask[0, :n]])
    assert whole.any() and np.any(kept.dropped_mask[0, :n][whole] != 0)
    for k in CLEAN + ('clean_csdm',):
        assert pt.same_bits(getattr(kept, k)[0, :n][whole], getattr(plain, k)[0, :n][whole]), k
    ols = _process(data, rij, W, 16, 8, grid, (4, 0.5, FLOOR, True), alpha=1.0)
    ols_kept = _process(data, rij, W, 16, 8, grid, (4, 0.5, FLOOR, True), alpha=1.0, kept=(N - 1, False, True))
    assert not ols_kept.dropped_mask.any()
    _same(ols_kept, ols, CLEAN + ('clean_csdm',) + CAPON)


def test_batch_of_three_recordings_equals_three_single_calls():
    recs = [cc.traces(4, 200, seed=910 + i) for i in range(3)]
    rij, grid = recs[0][1], cc.grid(129)
    kw = dict(prefiltered=True, capon_grid=grid, capon_freqs=[FREQ], capon_snapshots=(16, 8), capon_clean=(6, 0.5, FLOOR, True))
    batch = engine.process_batch([list(d) for d, _ in recs], FS, [T0 + i for i in range(3)], rij, [(None, None)], [65.5 / FS], 0.5,
                                 0.5, **kw)
    assert len(batch) == 3
    for got, (d, _) in zip(batch, recs):
        single = engine.process(d, FS, T0, rij, [(None, None)], [65.5 / FS], 0.5, 0.5, **kw)
        _same(got, single, CLEAN + ('clean_csdm',) + CAPON + PLAIN)
        _check_invariants(got)
    assert not np.array_equal(batch[0].clean_power, batch[1].clean_power)


@pytest.mark.parametrize('overlap', [1, -1])
def test_streamed_in_several_batches_equals_the_unstreamed_pass(monkeypatch, overlap):
    data, rij = cc.traces(9, 4000)
    grid = cc.grid(129)
    clean = (6, 0.5, FLOOR, True)
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    whole = _process(data, rij, 1200, 80, 40, grid, clean, alpha=0.5, overlap=0.75)
    h = engine.get_handle()
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '1')
    try:
        h.set_option('screen_batch_mb', 1)
        h.set_option('solve_min_units', 1)
        h.set_option('overlap', overlap)
        streamed = _process(data, rij, 1200, 80, 40, grid, clean, alpha=0.5, overlap=0.75)
        assert h.result_batches() >= 2
    finally:
        h.set_option('screen_batch_mb', 192)
        h.set_option('solve_min_units', 0)
        h.set_option('overlap', 0)
    _same(streamed, whole, CLEAN + ('clean_csdm',) + CAPON + PLAIN)
    _check_invariants(whole)


def test_two_window_slices_add_up_to_the_full_call():
    data, rij = cc.traces(4, 400)
    grid = cc.grid(129)
    full = _process(data, rij, 65, 16, 8, grid, (5, 0.5, FLOOR, True))
    parts = [_process(data, rij, 65, 16, 8, grid, (5, 0.5, FLOOR, True), window_slice=(k, 2)) for k in range(2)]
    n = int(full.nwin[0])
    first = [(n * k) // 2 for k in range(3)]
    for k in CLEAN + ('clean_csdm',):
        for s, part in enumerate(parts):
            a = getattr(part, k)[0]
            assert pt.same_bits(a[first[s]:first[s + 1]], getattr(full, k)[0, first[s]:first[s + 1]]), k
            assert not a[:first[s]].any() and not a[first[s + 1]:].any()      # rows outside a slice stay zero


def test_two_bands_in_one_plan_in_two_rounds_and_alone(monkeypatch):
    """tests/band_batch_cases.py, imported and not edited: its two bands of different W in one plan, in two rounds of one band
    each, and each band in a call of its own."""
    import band_batch_cases as bb
    recs, rij, t0s = bb.recordings()
    kw = dict(bb.CAPON, capon_clean=(6, 0.5, FLOOR, True))
    call = lambda edges, winlens, **k: engine.process(recs[0], bb.FS, t0s[0], rij, edges, winlens, bb.OVERLAP, 0.5, *bb.FILTER,
                                                      **dict(kw, **k))
    both = call(bb.EDGES, bb.WINLENS)
    _check_invariants(both)
    for b in range(2):
        one = call(bb.EDGES[b:b + 1], bb.WINLENS[b:b + 1], capon_freqs=bb.CAPON_FREQS[b:b + 1],
                   capon_snapshots=([bb.CAPON_SNAPSHOTS[0][b]], [bb.CAPON_SNAPSHOTS[1][b]]))
        n = int(both.nwin[b])
        assert n == int(one.nwin[0])                                 # (the calls' vector_len differ: the band's own windows)
        for k in CLEAN + ('clean_csdm',) + CAPON:
            assert pt.same_bits(getattr(both, k)[b, :n].copy(), getattr(one, k)[0, :n].copy()), (b, k)
    nchans, npts = recs[0].shape
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', repr(1.5 * 8.0 * nchans * (npts + 64) / 2.0 ** 30))
    assert engine.max_bands_per_pass(nchans, npts, 0) == 1           # one band per round: two rounds on one handle
    rounds = call(bb.EDGES, bb.WINLENS)
    _same(rounds, both, CLEAN + ('clean_csdm',) + CAPON + PLAIN)


@pytest.mark.parametrize('route', [1, 2])
def test_with_maps_and_peaks_on_both_routes_and_no_side_effects(route):
    data, rij = cc.traces(8, 400)
    grid = planner.slowness_grid(3.07, 13)
    kw = dict(capon_grid=grid, capon_freqs=[FREQ], capon_snapshots=(16, 8), want_capon_csdm=True, prefiltered=True)
    call = lambda **k: engine.process(data, FS, T0, rij, [(None, None)], [65.5 / FS], 0.5, 0.5, **dict(kw, **k))
    clean = (6, 0.5, FLOOR, False)
    alone = call(capon_clean=clean)
    h = engine.get_handle()
    try:
        h.set_option('capon_peak_route', route)
        extras = dict(want_capon_maps=True, capon_peaks=3, capon_peak_floor=0.0, want_beam=True, want_consistency=True)
        with_all = call(capon_clean=clean, **extras)
        without = call(**extras)
    finally:
        h.set_option('capon_peak_route', 0)
    _same(with_all, alone, CLEAN, 'maps and peaks')
    peaks = tuple(w + f for w in ('capon', 'bartlett') for f in engine.PEAK_FIELDS)
    _same(with_all, without, CAPON + PLAIN + peaks + ('capon_map', 'bartlett_map', 'capon_csdm', 'beam_power', 'fstat', 'consistency'))
    assert without.clean_count is None
    with pytest.raises(_hip.NblsError) as err:                       # after on and then off the plan is the plain plan again
        without.handle.fetch_capon_clean()
    assert err.value.code == _hip.NBLS_ERR_STATE
    with pytest.raises(_hip.NblsError) as err:                       # the residual matrix without the flag
        call(capon_clean=clean).handle.fetch_capon_clean_csdm()
    assert err.value.code == _hip.NBLS_ERR_STATE
    plain = call(want_capon_csdm=False, capon_clean=clean)            # the matrix is on the device, but not the caller's
    with pytest.raises(_hip.NblsError) as err:
        plain.handle.fetch_capon_csdm()
    assert err.value.code == _hip.NBLS_ERR_STATE
    _same(plain, alone, CLEAN)


def test_refusal_under_an_rccl_communicator():
    src = os.path.join(ROOT, 'tests', 'c_caller', 'loopback_rccl.cpp')
    lib = os.path.join(ROOT, 'tests', 'c_caller', 'libloopback_rccl.so')
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.run(['/opt/rocm/bin/hipcc', '-O2', '-shared', '-fPIC', '--offload-arch=gfx950', src, '-o', lib], check=True,
                       timeout=300)
    env = dict(os.environ, NBLS_TEST_TRANSPORT=lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_clean_comm_worker.py')], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and 'CLEAN_COMM_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_the_three_public_calls():
    data, rij = cc.traces(6, 400)
    grid = planner.slowness_grid(3.07, 13)
    st = synthetic.make_stream(data, FS, starttime=T0)
    out = ltsva_clean(st, None, None, 65.5 / FS, 0.5, grid, FREQ, alpha=0.5, rij=rij, snapshots=(16, 8), iterations=6)
    plain = ltsva(st, None, None, 65.5 / FS, 0.5, alpha=0.5, rij=rij)
    for a, b in zip(out[:4], plain[:4]):
        assert pt.same_bits(a, b)
    d = out[8]
    n = len(out[0])
    assert d['clean_index'].shape == (n, 6) and d['source_power'].shape == (n, 4) and d['source_slowness'].shape == (n, 4, 2)
    res = _process(data, rij, 65, 16, 8, grid, (6, 0.5, FLOOR, False), alpha=0.5)
    for k in CLEAN:
        assert pt.same_bits(d[k], getattr(res, k)[0, :n]), k
    want = clean_sources(d['clean_index'], d['clean_power'], d['clean_count'], grid, 1.5 * planner.grid_cells(grid)[1].max(), 4)
    for k, a in zip(('source_power', 'source_slowness', 'source_vel', 'source_baz'), want):
        assert pt.same_bits(d[k], a), k
    radius = 1.5 * planner.grid_cells(grid)[1].max()
    everything = clean_sources(d['clean_index'], d['clean_power'], d['clean_count'], grid, radius, 6)[0]
    np.testing.assert_allclose(np.nansum(everything, axis=1), np.nansum(d['clean_power'], axis=1), rtol=1e-12)     # nothing is lost in the merge
    assert pt.same_bits(everything[:, :4].copy(), d['source_power'])
    st2 = synthetic.make_stream(data[:, ::-1].copy(), FS, starttime=T0 + 1)
    batch = ltsva_clean_batch([st, st2], None, None, 65.5 / FS, 0.5, grid, FREQ, alpha=0.5, rij=rij, snapshots=(16, 8), iterations=6)
    for k in d:
        assert pt.same_bits(batch[0][8][k], d[k]), k
    assert not np.array_equal(batch[1][8]['clean_power'], d['clean_power'])
    kept = ltsva_clean(st, None, None, 65.5 / FS, 0.5, grid, FREQ, alpha=0.5, rij=rij, snapshots=(16, 8), iterations=6, kept=True)
    assert kept[8]['kept_count'].shape == (n,)
    fr = np.logspace(-1, 0.5, 16)
    nb = narrow_band_least_squares_clean([10.0, 10.0], 0.5, 1.0, st, None, None, 2, np.zeros(16), np.zeros(16),
                                         np.array([0.5, 1.0, 2.0]), 'log', fr, 'butter', 2, 0.01, rij=rij, slowness_grid=grid,
                                         iterations=4)
    d2 = nb[9]
    assert d2['clean_index'].shape[0] == 2 and d2['clean_index'].shape[2] == 4 and np.all(d2['clean_count'] >= 0)
    assert np.any(d2['clean_count'] > 0) and np.all(np.isfinite(d2['source_power'][d2['clean_count'] == 0]))


@pytest.mark.parametrize('row', [0, 1])
def test_demonstration_on_a_patch(row):
    """Rows 1 and 2 of DESIGN.md section 24.4 (both sources inside a 21 x 21 patch around 60 degrees) through ``ltsva_clean``, the
    statements of tests/test_clean_truth.py::test_demonstration on the GPU's results, the truth being (a) on the GPU's own
    matrices of the same patch: every source found in at least as many windows as the truth less the 2 windows section 18.4
    left itself, in strictly more than the Bartlett peak list finds, for the weaker second wave in at least as many as the
    Capon peak list; the ratio of the median source powers within a factor of two of the truth's; the median power of
    components outside every radius within the bound."""
    rij, data, sources, W, inc = demo_case(row)
    grid, cells = demo_patch()
    st = synthetic.make_stream(data, FS, starttime=T0)
    out = ltsva_clean(st, None, None, W / FS, 0.5, grid, 0.5, alpha=1.0, rij=rij, iterations=32, gain=0.5, floor=0.02,
                      merge_radius=0.45, max_sources=len(sources) + 2)
    d = out[8]
    gpu = sum(found_every_source(d['source_slowness'][w], sources) for w in range(19))
    res = engine.process(data, FS, T0, rij, [(None, None)], [W / FS], 0.5, 1.0, prefiltered=True, capon_grid=grid, capon_freqs=[0.5],
                         capon_snapshots=planner.capon_snapshots(planner.co_array(rij)[0], grid, FS, [0.5], [W]),
                         want_capon_csdm=True, want_capon_maps=True)
    _, steer = res.handle.fetch_capon_tables(0)
    truth, powers, stray, tpowers = 0, [], [], []
    for w in range(19):
        ref = clt.clean_reference(res.capon_csdm[0, w], steer, 32, 0.5, 0.02)
        sl = clean_sources(ref['index'], ref['power'], ref['count'], grid, 0.45, len(sources) + 2)[1]
        truth += found_every_source(sl, sources)
        tpowers.append(source_powers(ref['index'], ref['power'], ref['count'], grid, sources)[0])
        per, outside = source_powers(d['clean_index'][w], d['clean_power'][w], d['clean_count'][w], grid, sources)
        powers.append(per)
        stray.append(outside)
    bartlett = peak_lists_find(res.bartlett_map[0, :19], grid, cells, sources)
    capon = peak_lists_find(res.capon_map[0, :19], grid, cells, sources)
    med, tmed = np.median(np.array(powers), axis=0), np.median(np.array(tpowers), axis=0)
    print('demonstration row %d on the patch: CLEAN-SC GPU %d / 19, truth (a) %d / 19, Capon peaks %d, Bartlett peaks %d; median '
          'source powers GPU %s, truth (a) %s, outside every radius %.4g, residual / total %.3f'
          % (row + 1, gpu, truth, capon, bartlett, np.array2string(med, precision=1), np.array2string(tmed, precision=1),
             np.median(stray), np.median(d['clean_residual'] / d['clean_total'])))
    assert gpu >= truth - 2
    assert gpu > bartlett
    if row == 1:
        assert gpu >= capon
    ratio, tratio = med / med[0], tmed / tmed[0]
    assert np.all(ratio <= 2.0 * tratio) and np.all(ratio >= 0.5 * tratio)
    assert np.median(stray) <= STRAY * med[0]
