"""The eigenvalues and the MUSIC pseudo-spectrum (``nbls_set_capon_music``, csrc/capon_music.hip: capon_music_kernel; DESIGN.md
section 25) against tests/music_truth.py: a long-double Jacobi method on the GPU's own R (fetched with ``want_capon_csdm``), so
that R's own error stays out, with bounds that are derived, never fitted; the tests print the worst |difference| / bound.
D = 1 / P is compared, never P.  Between the forms of a pass every output is equal bit for bit.  All cases use prefiltered
traces at fs = 20 Hz (tests/music_cases.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import capon_truth as ct
import clean_cases as cc
import music_cases as mc
import music_truth as mt
import peaks_truth as pt
from test_clean_truth import demo_case, demo_patch, peak_lists_find
from narrow_band_least_squares_amd import (engine, planner, synthetic, _hip, ltsva, ltsva_music, ltsva_music_batch,
                                           narrow_band_least_squares_music)

pytestmark = pytest.mark.gpu

FS, FREQ = mc.FS, mc.FREQ
T0 = 17884.0729166667
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUSIC = engine.MUSIC_FIELDS
ALL = MUSIC + ('music_map', 'music_vectors')
CAPON = ('capon_index', 'capon_power', 'bartlett_index', 'bartlett_power')
PLAIN = ('vel', 'baz', 'mdccm', 'sigma_tau', 'mask')
CAP = _hip.MUSIC_SWEEP_CAP


def _process(data, rij, W, Ls, Hs, grid, music, alpha=1.0, overlap=0.5, csdm=True, **kw):
    res = engine.process(data, FS, T0, rij, [(None, None)], [(W + 0.5) / FS], overlap, alpha, prefiltered=True, capon_grid=grid,
                         capon_freqs=[FREQ], capon_snapshots=(Ls, Hs), want_capon_csdm=csdm, capon_music=music, **kw)
    assert int(res.W[0]) == W
    return res


def _same(a, b, keys, label=''):
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        assert x is not None and y is not None, (label, k)
        assert pt.same_bits(x, y), (label, k)


def _check_window(label, res, w, steer, truth, compare_d, band=0):
    """One computed window of a plan with the map and the vectors against the truth of its own R -> dict of the worst
    |difference| / bound per quantity.  ``truth``: (lambda, E, sweeps) of ``mt.jacobi`` on the fetched R."""
    R = res.capon_csdm[band, w]
    N = R.shape[0]
    lam, E, _ = truth
    b = mt.bounds(R)
    ev = res.music_eigenvalues[band, w]
    out = {}
    assert np.all(np.diff(ev) <= 0), (label, ev)
    out['lam'] = float(np.max(np.abs(ev.astype(mt.LD) - lam))) / b['lam']
    assert 0 <= res.music_sweeps[band, w] < CAP, (label, res.music_sweeps[band, w])
    M = int(res.music_sources[band, w])
    assert 1 <= M <= N - 1
    P = res.music_map[band, w]
    g = int(res.music_index[band, w])
    assert g == int(np.argmax(P)) and pt.same_bits(res.music_power[band, w], P[g]), (label, g)      # (no NaN in a computed window's map)
    assert np.all(P > 0)
    V = res.music_vectors[band, w].astype(mt.CLD)
    Rl = R.astype(mt.CLD)
    out['resid'] = float(np.sqrt((np.abs(Rl @ V - V * ev[None, :].astype(mt.LD)) ** 2).sum())) / b['resid']
    out['orth'] = float(np.sqrt((np.abs(np.conj(V.T) @ V - np.eye(N)) ** 2).sum())) / b['orth']
    if compare_d:
        sp = mt.spectrum(lam, E, steer, M)
        assert sp['gap'] >= mc.GAP * float(lam[0]), '%s: a condition on the inputs: gap %r' % (label, sp['gap'] / float(lam[0]))
        tol = mt.bounds(R, M, sp['gap'])['D']
        with np.errstate(divide='ignore'):
            D = (mt.LD(1) / P.astype(mt.LD))
        out['D'] = float(np.max(np.abs(D - sp['D']))) / tol
        assert float(sp['D'][g]) <= float(sp['D'].min()) + 2 * tol, label
    for k, v in out.items():
        assert v <= 1.0, '%s: |%s - truth| / bound = %.3g' % (label, k, v)
    return out


@pytest.mark.parametrize('N,G,shape,S', mc.sets())
def test_against_the_truth(N, G, shape, S):
    """Every set of tests/music_cases.py, with M = S and by the rho rule: eigenvalues, vectors, sweeps, the source count from
    the fetched eigenvalues, the arg-max of the fetched map, and D within the bound wherever a gap can exist."""
    W, Ls, Hs = shape
    data, rij = mc.traces(N, W, S)
    grid = mc.grid(G)
    fixed = _process(data, rij, W, Ls, Hs, grid, (S, 0.5, True, True))
    rule = _process(data, rij, W, Ls, Hs, grid, (0, mc.EIG_FLOOR, True, True))
    _, steer = rule.handle.fetch_capon_tables(0)
    n = int(fixed.nwin[0])
    assert 2 <= n <= 4
    assert pt.same_bits(fixed.capon_csdm, rule.capon_csdm)
    _same(fixed, rule, ('music_eigenvalues', 'music_sweeps', 'music_vectors'))
    worst = {}
    for w in range(n):
        truth = mt.jacobi(fixed.capon_csdm[0, w])
        assert fixed.music_sources[0, w] == S
        assert rule.music_sources[0, w] == mt.sources_by_floor(rule.music_eigenvalues[0, w], mc.EIG_FLOOR)
        for name, res, cmp_d in (('M=%d' % S, fixed, mc.has_gap(N, W, Ls, Hs, S)), ('rule', rule, True)):
            got = _check_window('N=%d G=%d W=%d %s w=%d' % (N, G, W, name, w), res, w, steer, truth, cmp_d)
            for k, v in got.items():
                worst[k] = max(worst.get(k, 0.0), v)
    for k in ALL:
        assert not getattr(fixed, k)[0, n:].any(), k
    print('truth N=%d G=%d W=%d Ls=%d Hs=%d S=%d: %d windows, sweeps %d..%d, M by the rule %s; worst |difference| / bound %s'
          % (N, G, W, Ls, Hs, S, n, fixed.music_sweeps[0, :n].min(), fixed.music_sweeps[0, :n].max(), rule.music_sources[0, :n].tolist(),
             ', '.join('%s %.3g' % kv for kv in sorted(worst.items()))))


@pytest.mark.parametrize('Ls,K', [(65, 1), (49, 3)])
def test_rank_deficient_matrices(Ls, K):
    """K = 1 (the snapshot is the window) and K = 3 snapshots at N = 8: N - K eigenvalues within the bound of zero; D is
    compared with M = rank alone."""
    N, W = 8, 65
    assert ct.snapshot_count(W, Ls, 8) == K
    data, rij = mc.traces(N, W, 2)
    grid = mc.grid(129)
    res = _process(data, rij, W, Ls, 8, grid, (K, 0.5, True, True))
    _, steer = res.handle.fetch_capon_tables(0)
    n = int(res.nwin[0])
    worst = {}
    for w in range(n):
        R = res.capon_csdm[0, w]
        truth = mt.jacobi(R)
        lam = truth[0]
        ev = res.music_eigenvalues[0, w]
        b = mt.bounds(R)
        assert np.all(np.abs(ev[K:]) <= b['lam']) and ev[K - 1] > b['lam']
        got = _check_window('K=%d w=%d' % (K, w), res, w, steer, truth, False)
        sp = mt.spectrum(lam, truth[1], steer, K)
        tol = mt.bounds(R, K, sp['gap'])['D']
        got['D'] = float(np.max(np.abs(mt.LD(1) / res.music_map[0, w].astype(mt.LD) - sp['D']))) / tol
        assert got['D'] <= 1.0
        for k, v in got.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print('rank %d at N = 8: sweeps %s, gap / lambda_1 >= %.3g; worst |difference| / bound %s'
          % (K, res.music_sweeps[0, :n].tolist(), sp['gap'] / float(lam[0]), ', '.join('%s %.3g' % kv for kv in sorted(worst.items()))))


def test_degenerate_units():
    data, rij = cc.traces(4, 65, seed=3)
    data = np.tile(data, (1, 4))
    grid = mc.grid(129)
    music = (0, 0.05, True, True)
    good = _process(data, rij, 65, 16, 8, grid, music)
    n, inc = int(good.nwin[0]), int(good.inc[0])
    gap = data.copy()
    gap[:, 400:800] = 0.0
    res = _process(gap, rij, 65, 16, 8, grid, music)
    cover = (ct.snapshot_count(65, 16, 8) - 1) * 8 + 16              # the samples of a window its snapshots read: 64 of the 65
    empty = np.array([w * inc >= 400 and w * inc + cover <= 800 for w in range(n)])
    assert empty.sum() >= 3
    bad = data.copy()
    bad[1, 1000] = np.nan
    nan = _process(bad, rij, 65, 16, 8, grid, music)
    hit = np.array([w * inc <= 1000 < w * inc + cover for w in range(n)])
    assert 1 <= hit.sum() <= 3
    for r, none in ((res, empty), (nan, hit)):
        assert np.all(r.music_sources[0, :n][none] == -1) and np.all(r.music_index[0, :n][none] == -1)
        assert np.all(r.music_sweeps[0, :n][none] == 0)
        for k in ('music_eigenvalues', 'music_power', 'music_map', 'music_vectors'):
            assert np.all(np.isnan(getattr(r, k)[0, :n][none].view(np.float64))), k
        assert np.all(r.music_sources[0, :n][~none] >= 1) and np.all(np.isfinite(r.music_eigenvalues[0, :n][~none]))
    for k in ALL:                                                    # the windows the NaN does not reach are the good call's
        assert pt.same_bits(getattr(nan, k)[0, :n][~hit], getattr(good, k)[0, :n][~hit]), k
    assert np.all(good.music_sources[0, :n] >= 1) and np.all(np.isfinite(good.music_eigenvalues[0, :n]))


MPEAKS = tuple('music' + f for f in engine.PEAK_FIELDS)


@pytest.mark.parametrize('N,points,floor', [(8, 13, 0.0), (4, 21, 0.3), (32, 9, 0.0)])
def test_peaks_against_the_truth_with_the_map_and_through_the_slabs(N, points, floor):
    """The K strongest local maxima of the fetched map under tests/peaks_truth.py, bit for bit; a plan without
    NBLS_MUSIC_MAP takes the slab route and returns the same bits, also with two slabs for all its units; the Capon and
    Bartlett peaks of the plan are what they are without the request."""
    data, rij = cc.traces(N, 400)
    grid = planner.slowness_grid(3.07, points)
    cells = planner.grid_cells(grid)[0]
    K = 3
    kw = dict(capon_peaks=K, capon_peak_floor=0.25)
    kept = _process(data, rij, 65, 16, 8, grid, (2, 0.05, True, False, True, floor), **kw)
    n = int(kept.nwin[0])
    assert n >= 8
    want = pt.peaks_of_maps(kept.music_map[0, :n], cells, K, floor)
    for k, a in zip(MPEAKS, want):
        assert pt.same_bits(getattr(kept, k)[0, :n], a), k
        assert not getattr(kept, k)[0, n:].any(), k
    assert np.all(kept.music_peak_index[0, :n, 0] == kept.music_index[0, :n]) and np.all(kept.music_peak_count[0, :n] >= 1)
    slab = _process(data, rij, 65, 16, 8, grid, (2, 0.05, False, False, True, floor), **kw)
    assert slab.music_map is None
    _same(slab, kept, MPEAKS + MUSIC, 'through the slabs')
    h = engine.get_handle()
    try:
        h.set_option('capon_peak_slabs', 2)
        two = _process(data, rij, 65, 16, 8, grid, (2, 0.05, False, False, True, floor), **kw)
    finally:
        h.set_option('capon_peak_slabs', 0)
    _same(two, kept, MPEAKS + MUSIC, 'two slabs')
    without = _process(data, rij, 65, 16, 8, grid, None, **kw)
    _same(slab, without, tuple(w + f for w in ('capon', 'bartlett') for f in engine.PEAK_FIELDS) + CAPON)
    with pytest.raises(_hip.NblsError) as err:
        without.handle.fetch_capon_music_peaks()
    assert err.value.code == _hip.NBLS_ERR_STATE


def test_peaks_of_degenerate_units_and_without_a_peak_request():
    data, rij = cc.traces(4, 65, seed=3)
    data = np.tile(data, (1, 4))
    data[:, 400:800] = 0.0
    grid = planner.slowness_grid(3.07, 9)
    res = _process(data, rij, 65, 16, 8, grid, (0, 0.05, False, False, True, 0.0), capon_peaks=2)
    n = int(res.nwin[0])
    none = res.music_sources[0, :n] == -1
    assert none.sum() >= 3 and not none.all()
    assert np.all(res.music_peak_count[0, :n][none] == 0) and np.all(res.music_peak_index[0, :n][none] == -1)
    assert np.all(np.isnan(res.music_peak_power[0, :n][none])) and np.all(np.isnan(res.music_peak_offset[0, :n][none]))
    assert np.all(res.music_peak_count[0, :n][~none] >= 1)
    h = res.handle                                                   # the flag without nbls_set_capon_peaks: the library's own refusal
    h.set_capon(grid, [FREQ], [16], [8])
    h.set_capon_music(2, 0.05, False, False, True, 0.0)
    try:
        with pytest.raises(_hip.NblsError) as err:
            h.plan(None, False, None, None, [65], [32], 40)
        assert err.value.code == _hip.NBLS_ERR_STATE and 'nbls_set_capon_peaks' in str(err.value)
    finally:
        h.set_capon(None)
        h.set_capon_music(None)


def test_batch_of_three_recordings_equals_three_single_calls():
    recs = [cc.traces(4, 200, seed=910 + i) for i in range(3)]
    rij, grid = recs[0][1], mc.grid(129)
    grid = planner.slowness_grid(3.07, 11)
    kw = dict(prefiltered=True, capon_grid=grid, capon_freqs=[FREQ], capon_snapshots=(16, 8), capon_peaks=2,
              capon_music=(0, 0.05, True, True, True, 0.0))
    batch = engine.process_batch([list(d) for d, _ in recs], FS, [T0 + i for i in range(3)], rij, [(None, None)], [65.5 / FS], 0.5,
                                 0.5, **kw)
    assert len(batch) == 3
    for got, (d, _) in zip(batch, recs):
        single = engine.process(d, FS, T0, rij, [(None, None)], [65.5 / FS], 0.5, 0.5, **kw)
        _same(got, single, ALL + MPEAKS + CAPON + PLAIN)
    assert not np.array_equal(batch[0].music_power, batch[1].music_power)


@pytest.mark.parametrize('overlap', [1, -1])
def test_streamed_in_several_batches_equals_the_unstreamed_pass(monkeypatch, overlap):
    data, rij = cc.traces(9, 4000)
    grid = planner.slowness_grid(3.07, 11)
    music = (2, 0.05, False, True, True, 0.0)                        # (no map: the peaks go through the slabs)
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    whole = _process(data, rij, 1200, 80, 40, grid, music, alpha=0.5, overlap=0.75, capon_peaks=3)
    h = engine.get_handle()
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '1')
    try:
        h.set_option('screen_batch_mb', 1)
        h.set_option('solve_min_units', 1)
        h.set_option('overlap', overlap)
        streamed = _process(data, rij, 1200, 80, 40, grid, music, alpha=0.5, overlap=0.75, capon_peaks=3)
        assert h.result_batches() >= 2
    finally:
        h.set_option('screen_batch_mb', 192)
        h.set_option('solve_min_units', 0)
        h.set_option('overlap', 0)
    _same(streamed, whole, MUSIC + ('music_vectors',) + MPEAKS + CAPON + PLAIN)


def test_two_window_slices_add_up_to_the_full_call():
    data, rij = cc.traces(4, 400)
    grid = mc.grid(129)
    music = (0, 0.05, True, True)
    full = _process(data, rij, 65, 16, 8, grid, music)
    parts = [_process(data, rij, 65, 16, 8, grid, music, window_slice=(k, 2)) for k in range(2)]
    n = int(full.nwin[0])
    first = [(n * k) // 2 for k in range(3)]
    for k in ALL:
        for s, part in enumerate(parts):
            a = getattr(part, k)[0]
            assert pt.same_bits(a[first[s]:first[s + 1]], getattr(full, k)[0, first[s]:first[s + 1]]), k
            assert not a[:first[s]].any() and not a[first[s + 1]:].any()      # rows outside a slice stay zero


def test_two_bands_in_one_plan_in_two_rounds_and_alone(monkeypatch):
    """tests/band_batch_cases.py, imported and not edited: its two bands of different W and tables in one plan, in two rounds
    of one band each, and each band in a call of its own."""
    import band_batch_cases as bb
    recs, rij, t0s = bb.recordings()
    kw = dict(bb.CAPON, capon_music=(0, 0.05, True, True))
    call = lambda edges, winlens, **k: engine.process(recs[0], bb.FS, t0s[0], rij, edges, winlens, bb.OVERLAP, 0.5, *bb.FILTER,
                                                      **dict(kw, **k))
    both = call(bb.EDGES, bb.WINLENS)
    for b in range(2):
        one = call(bb.EDGES[b:b + 1], bb.WINLENS[b:b + 1], capon_freqs=bb.CAPON_FREQS[b:b + 1],
                   capon_snapshots=([bb.CAPON_SNAPSHOTS[0][b]], [bb.CAPON_SNAPSHOTS[1][b]]))
        n = int(both.nwin[b])
        assert n == int(one.nwin[0])                                 # (the calls' vector_len differ: the band's own windows)
        for k in ALL + CAPON:
            assert pt.same_bits(getattr(both, k)[b, :n].copy(), getattr(one, k)[0, :n].copy()), (b, k)
    assert not np.array_equal(both.music_map[0], both.music_map[1])
    nchans, npts = recs[0].shape
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', repr(1.5 * 8.0 * nchans * (npts + 64) / 2.0 ** 30))
    assert engine.max_bands_per_pass(nchans, npts, 0) == 1           # one band per round: two rounds on one handle
    rounds = call(bb.EDGES, bb.WINLENS)
    _same(rounds, both, ALL + CAPON + PLAIN)


def test_no_side_effects_and_the_fetches_of_other_plans():
    data, rij = cc.traces(8, 400)
    grid = planner.slowness_grid(3.07, 13)
    kw = dict(capon_grid=grid, capon_freqs=[FREQ], capon_snapshots=(16, 8), want_capon_csdm=True, prefiltered=True)
    call = lambda **k: engine.process(data, FS, T0, rij, [(None, None)], [65.5 / FS], 0.5, 0.5, **dict(kw, **k))
    music = (2, 0.05, False, False)
    alone = call(capon_music=music)
    extras = dict(want_capon_maps=True, capon_peaks=3, capon_peak_floor=0.0, want_beam=True, want_consistency=True,
                  capon_clean=(6, 0.5, 0.02, True))
    with_all = call(capon_music=music, **extras)
    without = call(**extras)
    _same(with_all, alone, MUSIC, 'beside everything else')
    peaks = tuple(w + f for w in ('capon', 'bartlett') for f in engine.PEAK_FIELDS)
    _same(with_all, without, CAPON + PLAIN + peaks + engine.CLEAN_FIELDS + ('clean_csdm', 'capon_map', 'bartlett_map', 'capon_csdm',
                                                                            'beam_power', 'fstat', 'consistency'))
    assert without.music_eigenvalues is None and alone.music_map is None and alone.music_vectors is None
    for fetch in (without.handle.fetch_capon_music, without.handle.fetch_capon_music_map, without.handle.fetch_capon_music_vectors):
        with pytest.raises(_hip.NblsError) as err:                   # after on and then off the plan is the plain plan again
            fetch()
        assert err.value.code == _hip.NBLS_ERR_STATE
    h = call(capon_music=music).handle
    for fetch in (h.fetch_capon_music_map, h.fetch_capon_music_vectors):     # the map and the vectors without their flags
        with pytest.raises(_hip.NblsError) as err:
            fetch()
        assert err.value.code == _hip.NBLS_ERR_STATE
    plain = call(want_capon_csdm=False, capon_music=music)           # the matrix is on the device, but not the caller's
    with pytest.raises(_hip.NblsError) as err:
        plain.handle.fetch_capon_csdm()
    assert err.value.code == _hip.NBLS_ERR_STATE
    _same(plain, alone, MUSIC)
    h.set_capon(grid, [FREQ], [16], [8])                             # more sources than N - 1: the library's own refusal
    h.set_capon_music(8)
    try:
        with pytest.raises(ValueError, match='sources') as err:
            h.plan(None, False, None, None, [65], [32], 40)
        assert err.value.code == _hip.NBLS_ERR_ARG
    finally:
        h.set_capon(None)
        h.set_capon_music(None)


def test_refusal_under_an_rccl_communicator():
    src = os.path.join(ROOT, 'tests', 'c_caller', 'loopback_rccl.cpp')
    lib = os.path.join(ROOT, 'tests', 'c_caller', 'libloopback_rccl.so')
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.run(['/opt/rocm/bin/hipcc', '-O2', '-shared', '-fPIC', '--offload-arch=gfx950', src, '-o', lib], check=True,
                       timeout=300)
    env = dict(os.environ, NBLS_TEST_TRANSPORT=lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_music_comm_worker.py')], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and 'MUSIC_COMM_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_the_three_public_calls():
    data, rij = cc.traces(6, 400)
    grid = planner.slowness_grid(3.07, 13)
    st = synthetic.make_stream(data, FS, starttime=T0)
    out = ltsva_music(st, None, None, 65.5 / FS, 0.5, grid, FREQ, alpha=0.5, rij=rij, snapshots=(16, 8), sources=2, maps=True,
                      vectors=True, peaks=3, peak_floor=0.1)
    plain = ltsva(st, None, None, 65.5 / FS, 0.5, alpha=0.5, rij=rij)
    for a, b in zip(out[:4], plain[:4]):
        assert pt.same_bits(a, b)
    d = out[8]
    n = len(out[0])
    assert d['music_eigenvalues'].shape == (n, 6) and d['music_map'].shape == (n, len(grid)) and d['music_vectors'].shape == (n, 6, 6)
    res = _process(data, rij, 65, 16, 8, grid, (2, 0.05, True, True, True, 0.1), alpha=0.5, capon_peaks=3)
    for k in ALL + MPEAKS:
        assert pt.same_bits(d[k], getattr(res, k)[0, :n]), k
    steps = planner.grid_cells(grid)[1]
    first = grid[d['music_peak_index'][:, 0]] + d['music_peak_offset'][:, 0] * steps
    np.testing.assert_allclose(d['music_peak_slowness'][:, 0], first)
    np.testing.assert_allclose(d['music_peak_vel'][:, 0], 1.0 / np.hypot(first[:, 0], first[:, 1]))
    assert d['music_peak_baz'].shape == (n, 3) and 'capon_peak_index' not in d
    assert np.all(d['music_sources'] == 2) and np.all(d['music_index'] == np.argmax(d['music_map'], axis=1))
    s = grid[d['music_index']]
    np.testing.assert_allclose(d['music_vel'], 1.0 / np.hypot(s[:, 0], s[:, 1]))
    st2 = synthetic.make_stream(data[:, ::-1].copy(), FS, starttime=T0 + 1)
    batch = ltsva_music_batch([st, st2], None, None, 65.5 / FS, 0.5, grid, FREQ, alpha=0.5, rij=rij, snapshots=(16, 8), sources=2,
                              maps=True, vectors=True, peaks=3, peak_floor=0.1)
    for k in d:
        assert pt.same_bits(batch[0][8][k], d[k]), k
    assert not np.array_equal(batch[1][8]['music_power'], d['music_power'])
    fr = np.logspace(-1, 0.5, 16)
    nb = narrow_band_least_squares_music([10.0, 10.0], 0.5, 1.0, st, None, None, 2, np.zeros(16), np.zeros(16),
                                         np.array([0.5, 1.0, 2.0]), 'log', fr, 'butter', 2, 0.01, rij=rij, slowness_grid=grid,
                                         peaks=2)
    d2 = nb[9]
    assert d2['music_eigenvalues'].shape[0] == 2 and d2['music_eigenvalues'].shape[2] == 6
    computed = d2['music_sources'] > 0
    assert computed.any() and np.all(d2['music_sources'][computed] <= 5) and np.all(d2['music_index'][computed] >= 0)
    assert np.all(np.diff(d2['music_eigenvalues'][computed], axis=-1) <= 0)
    assert d2['music_peak_index'].shape[2] == 2 and np.all(d2['music_peak_index'][computed][:, 0] == d2['music_index'][computed])
    assert not d2['music_peak_vel'][~computed].any()


def test_demonstration_on_a_patch():
    """Row 2 of DESIGN.md section 25.4 (a second wave 10 dB down, 20 degrees away; both inside a 21 x 21 patch around 60
    degrees) through ``ltsva_music`` with M = 2: the two strongest local maxima of the GPU's map are the two sources in at
    least as many windows as those of the truth's map on the GPU's own matrices, less 2."""
    rij, data, sources, W, inc = demo_case(1)
    grid, cells = demo_patch()
    st = synthetic.make_stream(data, FS, starttime=T0)
    out = ltsva_music(st, None, None, W / FS, 0.5, grid, 0.5, alpha=1.0, rij=rij, sources=2, maps=True)
    d = out[8]
    gpu = peak_lists_find(d['music_map'][:19], grid, cells, sources)
    res = engine.process(data, FS, T0, rij, [(None, None)], [W / FS], 0.5, 1.0, prefiltered=True, capon_grid=grid, capon_freqs=[0.5],
                         capon_snapshots=planner.capon_snapshots(planner.co_array(rij)[0], grid, FS, [0.5], [W]),
                         want_capon_csdm=True, want_capon_maps=True)
    _, steer = res.handle.fetch_capon_tables(0)
    with np.errstate(divide='ignore'):
        maps = [(1.0 / mt.music(res.capon_csdm[0, w], steer, 2)['D']).astype(np.float64) for w in range(19)]
    truth = peak_lists_find(maps, grid, cells, sources)
    capon = peak_lists_find(res.capon_map[0, :19], grid, cells, sources)
    print('demonstration row 2 on the patch: MUSIC M = 2 GPU %d / 19, truth %d / 19, Capon peaks %d; sweeps %d..%d'
          % (gpu, truth, capon, d['music_sweeps'][:19].min(), d['music_sweeps'][:19].max()))
    assert gpu >= truth - 2
