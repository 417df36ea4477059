"""The K strongest peaks of the Capon / Bartlett spectra (``nbls_set_capon_peaks``, csrc/capon.hip: capon_peaks_of; DESIGN.md
section 19).  The peaks are an exact function of the GPU's own maps, so every comparison is bit for bit against
``peaks_truth`` applied to the maps fetched from the same pass: no tolerance.  Between the two routes (the unit's maps in LDS
or in HBM), the slab counts, and the forms of a pass (streamed, batched, window slices) every output is equal bit for bit.
All cases use prefiltered traces at fs = 20 Hz."""
import subprocess

import numpy as np
import pytest

import capon_truth as ct
import peaks_truth as pt
from test_capon_truth import two_source_case, BAZ
from test_peaks_host import build_peaks_caller
from narrow_band_least_squares_amd import (engine, planner, synthetic, _hip, ltsva_capon, ltsva_capon_batch,
                                           narrow_band_least_squares_capon)

pytestmark = pytest.mark.gpu

FS = 20.0
T0 = 17884.0729166667
FREQ = 1.3
PEAKS = tuple(w + f for w in ('capon', 'bartlett') for f in engine.PEAK_FIELDS)
CAPON = ('capon_index', 'capon_power', 'bartlett_index', 'bartlett_power')
PLAIN = ('vel', 'baz', 'mdccm', 'sigma_tau', 'mask')
FLOOR = {1: 1.0, 2: 0.25, 4: 0.25, 8: 0.0}


def _lattice(n0, n1, step=0.5):
    g0, g1 = np.meshgrid((np.arange(n0) - n0 // 2) * step, (np.arange(n1) - n1 // 2) * step, indexing='ij')
    return np.ascontiguousarray(np.stack([g0.ravel(), g1.ravel()], axis=1))


GRIDS = {1: np.zeros((1, 2)), 21: planner.slowness_grid(3.07, 5), 127: _lattice(12, 11)[:127], 128: _lattice(12, 11)[:128],
         129: _lattice(12, 11)[:129], 1257: planner.slowness_grid(4.0, 41)}


def _geometry(N):
    rij = synthetic.array_geometry(N, 1.0)
    return rij - rij.mean(axis=1, keepdims=True)


def _noise(N, npts, seed=1900):
    return np.random.default_rng(seed + N).standard_normal((N, npts)), _geometry(N)


def _wave(N, npts, seed=900, snr_db=6.0):
    rij = synthetic.array_geometry(N, 1.0)
    data = synthetic.plane_wave(rij, npts, FS, 0.5, 4.0, baz_deg=60.0, snr_db=snr_db, seed=seed)
    return data, rij - rij.mean(axis=1, keepdims=True)


def _process(data, rij, W, alpha, Ls, Hs, grid, K, floor=None, delta=0.01, overlap=0.5, maps=True, **kw):
    res = engine.process(data, FS, T0, rij, [(None, None)], [(W + 0.5) / FS], overlap, alpha, prefiltered=True, capon_grid=grid,
                         capon_freqs=[FREQ], capon_snapshots=(Ls, Hs), capon_loading=delta, want_capon_maps=maps,
                         capon_peaks=K, capon_peak_floor=FLOOR.get(K, 0.25) if floor is None else floor, **kw)
    assert int(res.W[0]) == W
    return res


def _against_truth(res, cells, K, floor, label='', band=0):
    """All eight fields of the band against the truth on the pass's own maps; rank 0 is the arg-max; cells beyond nwin are zeros."""
    n = int(res.nwin[band])
    counts = {}
    for name in ('capon', 'bartlett'):
        want = pt.peaks_of_maps(getattr(res, name + '_map')[band, :n], cells, K, floor)
        for field, exp in zip(engine.PEAK_FIELDS, want):
            got = getattr(res, name + field)
            assert pt.same_bits(got[band, :n], exp), '%s %s%s: got %r, the truth has %r' % (label, name, field, got[band, :n], exp)
            assert not got[band, n:].any(), name + field
        assert np.array_equal(getattr(res, name + '_peak_index')[band, :n, 0], getattr(res, name + '_index')[band, :n])
        assert pt.same_bits(getattr(res, name + '_peak_power')[band, :n, 0], getattr(res, name + '_power')[band, :n])
        counts[name] = want[0]
    return counts


def _same(a, b, keys):
    for k in keys:
        assert pt.same_bits(getattr(a, k), getattr(b, k)), k


@pytest.mark.parametrize('G', sorted(GRIDS))
@pytest.mark.parametrize('Ls,Hs', [(16, 1), (64, 1)])
@pytest.mark.parametrize('N', [3, 8, 32])
def test_matches_the_truth(N, Ls, Hs, G):
    """Noise only, so that the maps are full of maxima; the grid sizes are the strides of the 128-thread loop and one real
    grid; K = 1, 2, 8 with the floors 1.0, 0.25 and 0.  At G = 1257 and floor 0 there are more kept peaks than ranks."""
    grid = GRIDS[G]
    cells = planner.grid_cells(grid)[0]
    data, rij = _noise(N, 65 * 3)
    for K in (1, 2, 8):
        res = _process(data, rij, 65, 1.0, Ls, Hs, grid, K)
        assert int(res.nwin[0]) >= 2
        counts = _against_truth(res, cells, K, FLOOR[K], 'N=%d Ls=%d G=%d K=%d' % (N, Ls, G, K))
        assert np.all(counts['capon'] >= 1) and np.all(counts['bartlett'] >= 1)
        if G == 1257 and K == 8:
            print('N=%d Ls=%d: kept peaks per window, Capon %s, Bartlett %s' % (N, Ls, counts['capon'], counts['bartlett']))
            assert counts['capon'].max() > 8 or counts['bartlett'].max() > 8


PLATEAUS = {'block': [(1, 1), (1, 2), (1, 3), (2, 1), (2, 2), (2, 3)], 'L': [(1, 1), (2, 1), (3, 1), (3, 2), (3, 3)],
            'row': [(2, j) for j in range(5)]}


@pytest.mark.parametrize('permuted', [False, True])
@pytest.mark.parametrize('shape', sorted(PLATEAUS))
def test_plateaus_of_equal_values(shape, permuted):
    """Several grid points repeat the wave's own slowness vector: identical steering rows, identical P, and distinct cells
    laid out as a 2 x 3 block, an L and a whole row of a 5 x 5 lattice; the other points lie at least 1 s/km away, where
    the long-double reference has both spectra at most 0.9 of the plateau's.  The plateau holds the maximum, and rank 0 is
    its lowest index.  With the grid in the lattice's own order that point is the plateau's only peak; in a permuted order
    two of its points that are no neighbours may both be peaks, and the truth says which."""
    rij = synthetic.array_geometry(4, 1.0)
    data = synthetic.plane_wave(rij, 65 * 4, FS, 0.5, 4.0, baz_deg=60.0, vel_kms=2.0, snr_db=20.0, seed=900)
    rij = rij - rij.mean(axis=1, keepdims=True)
    rng = np.random.default_rng(77)
    order = rng.permutation(25) if permuted else np.arange(25)
    cells = np.array([(k // 5, k % 5) for k in order], dtype=np.int32)
    wave = np.array([np.sin(np.radians(60.0)), np.cos(np.radians(60.0))]) / 2.0
    ang, rad = rng.uniform(0.0, 2.0 * np.pi, 25), rng.uniform(1.0, 3.0, 25)
    grid = np.round(wave + np.stack([rad * np.sin(ang), rad * np.cos(ang)], axis=1), 3)
    flat = [g for g, c in enumerate(cells) if (int(c[0]), int(c[1])) in PLATEAUS[shape]]
    grid[flat] = wave
    res = _process(data, rij, 65, 1.0, 16, 1, grid, 8, floor=0.0, capon_cells=cells)
    n = int(res.nwin[0])
    for name in ('capon', 'bartlett'):
        m = getattr(res, name + '_map')[0, :n]
        assert np.all(m[:, flat] == m[:, flat[:1]])
        assert np.all(getattr(res, name + '_peak_index')[0, :n, 0] == min(flat))
        if not permuted:
            assert not np.isin(getattr(res, name + '_peak_index')[0, :n, 1:], flat).any()
    _against_truth(res, cells, 8, 0.0, shape)


def test_degenerate_units():
    """A stretch of zeros: both spectra empty.  One element zero throughout without loading (a pivot of exactly 0): the Capon
    peaks are empty, the Bartlett peaks stay."""
    W, Ls, Hs, K = 65, 16, 8, 2
    grid = GRIDS[21]
    cells = planner.grid_cells(grid)[0]
    data, rij = _wave(4, 2401)
    gap = data.copy()
    gap[:, 800:1400] = 0.0
    res = _process(gap, rij, W, 1.0, Ls, Hs, grid, K)
    n, inc = int(res.nwin[0]), int(res.inc[0])
    empty = np.array([w * inc >= 800 and w * inc + W <= 1400 for w in range(n)])
    assert empty.sum() >= 3
    for name in ('capon', 'bartlett'):
        assert np.all(getattr(res, name + '_peak_count')[0, :n][empty] == 0) and np.all(getattr(res, name + '_peak_count')[0, :n][~empty] >= 1)
        assert np.all(getattr(res, name + '_peak_index')[0, :n][empty] == -1)
        assert np.all(np.isnan(getattr(res, name + '_peak_power')[0, :n][empty])) and np.all(np.isnan(getattr(res, name + '_peak_offset')[0, :n][empty]))
    _against_truth(res, cells, K, FLOOR[K], 'empty windows')
    dead = data.copy()
    dead[2] = 0.0
    res = _process(dead, rij, W, 1.0, Ls, Hs, grid, K, delta=0.0)
    assert np.all(res.capon_peak_count[0, :n] == 0) and np.all(res.capon_peak_index[0, :n] == -1) and np.all(np.isnan(res.capon_peak_power[0, :n]))
    assert np.all(res.bartlett_peak_count[0, :n] >= 1) and np.all(res.bartlett_peak_index[0, :n, 0] >= 0)
    _against_truth(res, cells, K, FLOOR[K], 'dead element')


class _options:
    """Options of the shared handle for the plans made inside the block."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            engine.get_handle().set_option(k, v)

    def __exit__(self, *exc):
        engine.get_handle().set_option('capon_peak_route', 0)
        engine.get_handle().set_option('capon_peak_slabs', 0)


@pytest.mark.parametrize('N,G', [(3, 21), (8, 1257), (32, 129)])
def test_both_routes_give_the_same_bits(N, G):
    grid = GRIDS[G]
    cells = planner.grid_cells(grid)[0]
    data, rij = _noise(N, 65 * 4)
    out = {}
    for route in (1, 2):
        with _options(capon_peak_route=route):
            out[route] = _process(data, rij, 65, 1.0, 16, 1, grid, 4)
            out[route, 'no maps'] = _process(data, rij, 65, 1.0, 16, 1, grid, 4, maps=False)
    _against_truth(out[1], cells, 4, 0.25, 'LDS route')
    _same(out[2], out[1], PEAKS + CAPON + PLAIN + ('capon_map', 'bartlett_map'))
    for route in (1, 2):                                             # the HBM route's slab is the unit's rows of the maps, or a scratch
        assert out[route, 'no maps'].capon_map is None
        _same(out[route, 'no maps'], out[1], PEAKS + CAPON + PLAIN)


def test_seams_between_the_launches_of_the_hbm_route():
    """Two slabs for five windows: three launches, and the stream's order hands the slabs on."""
    grid = GRIDS[1257]
    data, rij = _noise(8, 65 * 3)
    out = {}
    for slabs in (2, 256):
        with _options(capon_peak_route=2, capon_peak_slabs=slabs):
            out[slabs] = _process(data, rij, 65, 1.0, 16, 1, grid, 8, maps=False)
    assert int(out[2].nwin[0]) == 5
    _same(out[2], out[256], PEAKS + CAPON + PLAIN)
    with _options(capon_peak_route=2, capon_peak_slabs=2):
        _against_truth(_process(data, rij, 65, 1.0, 16, 1, grid, 8), planner.grid_cells(grid)[0], 8, 0.0, 'two slabs')


def test_lds_route_that_does_not_fit_is_refused_and_the_large_grid_takes_the_hbm_route():
    data, rij = _noise(32, 65 * 2)
    with _options(capon_peak_route=1):
        with pytest.raises(ValueError, match='capon_peak_route 1') as err:
            _process(data, rij, 65, 1.0, 16, 1, _lattice(128, 64, 0.05), 2)
        assert err.value.code == _hip.NBLS_ERR_UNSUPPORTED
    h = engine.get_handle()
    for bad in (('capon_peak_route', 3), ('capon_peak_route', -1), ('capon_peak_slabs', -1), ('capon_peak_slabs', 4097)):
        with pytest.raises(ValueError):
            h.set_option(*bad)
    grid = _lattice(256, 256, 0.03)                                  # 65536 points: 1 MiB of maps per unit
    data, rij = _noise(3, 65 + 32 + 1)
    res = _process(data, rij, 65, 1.0, 16, 1, grid, 2)
    assert int(res.nwin[0]) == 2
    _against_truth(res, planner.grid_cells(grid)[0], 2, 0.25, 'G = 65536')
    slabs = _process(data, rij, 65, 1.0, 16, 1, grid, 2, maps=False)          # ... and in the scratch's slabs instead of the map rows
    assert slabs.capon_map is None
    _same(slabs, res, PEAKS + CAPON + PLAIN)


def test_streamed_in_several_batches_equals_the_unstreamed_pass(monkeypatch):
    data, rij = _wave(9, 24001)
    grid = GRIDS[129]
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    whole = _process(data, rij, 1200, 0.5, 80, 40, grid, 4, overlap=0.75)
    h = engine.get_handle()
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '1')
    try:
        h.set_option('screen_batch_mb', 1)
        h.set_option('solve_min_units', 1)
        streamed = _process(data, rij, 1200, 0.5, 80, 40, grid, 4, overlap=0.75)
        assert h.result_batches() >= 2
    finally:
        h.set_option('screen_batch_mb', 192)
        h.set_option('solve_min_units', 0)
    _same(streamed, whole, PEAKS + CAPON + PLAIN)
    _against_truth(whole, planner.grid_cells(grid)[0], 4, 0.25, 'streamed')


@pytest.mark.parametrize('route,maps', [(0, True), (1, False), (2, False)])
def test_batch_of_three_recordings_equals_three_single_calls(route, maps):
    """Three recordings in one pass (``nbls_set_segments``: result row b * 3 + s): every recording's eight fields, and the
    results beside them, equal the single call's; on the HBM route without the maps the rows' units share the slabs."""
    recs = [_wave(4, 1201, seed=910 + i) for i in range(3)]
    rij, grid = recs[0][1], GRIDS[21]
    kw = dict(prefiltered=True, capon_grid=grid, capon_freqs=[FREQ], capon_snapshots=(16, 8), capon_peaks=3, capon_peak_floor=0.0)
    with _options(capon_peak_route=route, capon_peak_slabs=0 if route != 2 else 8):
        batch = engine.process_batch([list(d) for d, _ in recs], FS, [T0 + i for i in range(3)], rij, [(None, None)], [65.5 / FS],
                                     0.5, 0.5, want_capon_maps=maps, **kw)
    assert len(batch) == 3
    for got, (d, _) in zip(batch, recs):
        single = engine.process(d, FS, T0, rij, [(None, None)], [65.5 / FS], 0.5, 0.5, want_capon_maps=True, **kw)
        _same(got, single, PEAKS + CAPON + PLAIN)
        _against_truth(single, planner.grid_cells(grid)[0], 3, 0.0, 'batch')
        assert np.all(got.capon_peak_count[0, :int(got.nwin[0])] >= 1)
    assert not np.array_equal(batch[0].capon_peak_power, batch[1].capon_peak_power)
    assert not np.array_equal(batch[1].capon_peak_power, batch[2].capon_peak_power)


def test_solves_on_two_streams_share_the_slabs_in_turn(monkeypatch):
    """Window lengths of 30, 140 and 30 s at 100 Hz in one plan: the 140 s band (W = 14 000) takes the general correlator and
    is solved on the pass's first stream, the screened bands, with option overlap, on its second.  Their Capon launches
    share the slabs of the HBM route (four here, so every launch reuses them) and must take them in turn: every field equals
    the LDS route's without overlap."""
    fs = 100.0
    rij = synthetic.array_geometry(8, 1.0, seed=5)
    data = synthetic.plane_wave(rij, 40000, fs, 0.1, 5.0, seed=21)
    rij = rij - rij.mean(axis=1, keepdims=True)
    edges, winlens = [(0.3, 0.6), (0.1, 0.3), (0.6, 1.2)], [30.0, 140.0, 30.0]
    kw = dict(capon_grid=GRIDS[129], capon_freqs=planner.capon_frequencies(edges), capon_snapshots=(256, 128), capon_peaks=4,
              capon_peak_floor=0.0, groups=1)
    call = lambda: engine.process(data, fs, T0, rij, edges, winlens, 0.5, 0.5, 'butter', 2, 0.01, **kw)
    h = engine.get_handle()
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '1')
    try:
        h.set_option('overlap', -1)
        with _options(capon_peak_route=1):
            lds = call()
        h.set_profiling(True)
        h.set_option('overlap', 1)
        with _options(capon_peak_route=2, capon_peak_slabs=4):
            hbm = call()
            tm = h.timings()
    finally:
        h.set_profiling(False)
        h.set_option('overlap', 0)
    assert tm['xcorr_impl'] == 3 and tm['xcorr_fallback_bands'] == 1          # a screened plan with one band on the general correlator
    assert [int(w) for w in hbm.W] == [3000, 14000, 3000]
    _same(hbm, lds, PEAKS + CAPON + PLAIN)
    for b in range(3):
        assert np.all(hbm.capon_peak_count[b, :int(hbm.nwin[b])] >= 1)


def test_two_window_slices_add_up_to_the_full_call():
    data, rij = _wave(4, 2401)
    full = _process(data, rij, 65, 0.5, 16, 8, GRIDS[21], 2)
    parts = [_process(data, rij, 65, 0.5, 16, 8, GRIDS[21], 2, window_slice=(k, 2)) for k in range(2)]
    n = int(full.nwin[0])
    first = [(n * k) // 2 for k in range(3)]
    for k in PEAKS:
        for s, part in enumerate(parts):
            a = getattr(part, k)[0]
            assert pt.same_bits(a[first[s]:first[s + 1]], getattr(full, k)[0, first[s]:first[s + 1]]), k
            assert not a[:first[s]].any() and not a[first[s + 1]:].any()      # rows outside a slice stay zero


def test_a_plan_with_peaks_leaves_every_other_result_as_it_was():
    data, rij = _wave(8, 2401)
    grid = GRIDS[129]
    kw = dict(capon_grid=grid, capon_freqs=[FREQ], capon_snapshots=(16, 8), want_capon_maps=True, want_capon_csdm=True)
    without = engine.process(data, FS, T0, rij, [(None, None)], [65.5 / FS], 0.5, 0.5, prefiltered=True, **kw)
    with_peaks = engine.process(data, FS, T0, rij, [(None, None)], [65.5 / FS], 0.5, 0.5, prefiltered=True, capon_peaks=3, **kw)
    assert without.capon_peak_count is None and with_peaks.capon_peak_index.shape[2] == 3
    _same(with_peaks, without, CAPON + PLAIN + ('capon_map', 'bartlett_map', 'capon_csdm'))
    with pytest.raises(_hip.NblsError) as err:                       # the next plan without a request has no peaks to fetch
        without = engine.process(data, FS, T0, rij, [(None, None)], [65.5 / FS], 0.5, 0.5, prefiltered=True, **kw)
        without.handle.fetch_capon_peaks(0)
    assert err.value.code == _hip.NBLS_ERR_STATE


def _both_in_the_ranks(index, count, grid):
    """``capon_truth.both_found``'s criterion on the returned peaks (the floor 0.25 is in the count already)."""
    if count < 2:
        return False
    sep = abs((BAZ[0] - BAZ[1] + 180.0) % 360.0 - 180.0)
    b = ct.grid_baz(grid, index[:2])
    near = lambda x, y: abs((x - y + 180.0) % 360.0 - 180.0) <= sep / 3.0
    return bool((near(b[0], BAZ[0]) and near(b[1], BAZ[1])) or (near(b[0], BAZ[1]) and near(b[1], BAZ[0])))


def test_two_sources_through_the_public_call():
    """The 21 x 21 patch around the two sources of DESIGN.md section 18.4: the two sources are rank 0 and rank 1 in as many
    windows as the long-double reference finds on the same patch, with no map fetched; peaks=0 returns the keys it returned;
    the narrow-band and the batched call agree with ``ltsva_capon``."""
    rij, data, _, _, W, inc = two_source_case()
    N = rij.shape[1]
    centre = np.array([np.sin(np.radians(np.mean(BAZ))), np.cos(np.radians(np.mean(BAZ)))]) / 0.34
    ax = np.arange(-10, 11) * 0.1
    g0, g1 = np.meshgrid(centre[0] + ax, centre[1] + ax, indexing='ij')
    grid = np.ascontiguousarray(np.stack([g0.ravel(), g1.ravel()], axis=1))
    st = synthetic.make_stream(data, FS, starttime=T0)
    out = ltsva_capon(st, None, None, W / FS, 0.5, grid, 0.5, alpha=1.0, rij=rij, peaks=2)
    cap = out[8]
    assert 'capon_map' not in cap and cap['capon_peak_index'].shape == (19, 2) and cap['capon_peak_offset'].shape == (19, 2, 2)
    xij = planner.co_array(rij)[0]
    Ls, Hs = planner.capon_snapshots(xij, grid, FS, [0.5], [W])
    coef, steer = ct.tables(xij, grid, FS, 0.5, Ls[0], N)
    R, _ = ct.csdm_reference(data, coef, W, inc, 19, int(Hs[0]))
    truth = sum(bool(ct.both_found(ct.spectra_reference(R[w].astype(np.complex128), steer, 0.01)['PC'], grid, (21, 21), BAZ))
                for w in range(19))
    gpu = sum(_both_in_the_ranks(cap['capon_peak_index'][w], cap['capon_peak_count'][w], grid) for w in range(19))
    gpu_b = sum(_both_in_the_ranks(cap['bartlett_peak_index'][w], cap['bartlett_peak_count'][w], grid) for w in range(19))
    print('two sources in ranks 0 and 1: Capon GPU %d / 19, truth %d / 19; Bartlett GPU %d / 19' % (gpu, truth, gpu_b))
    assert truth >= 15 and gpu == truth
    steps = planner.grid_cells(grid)[1]
    np.testing.assert_allclose(steps, [0.1, 0.1], rtol=1e-12)
    found = cap['capon_peak_index'] >= 0
    np.testing.assert_array_equal(cap['capon_peak_slowness'][found],
                                  (grid[cap['capon_peak_index']] + cap['capon_peak_offset'] * steps)[found])
    assert np.all(np.isnan(cap['capon_peak_vel'][~found])) and np.all(np.isfinite(cap['capon_peak_vel'][found]))
    assert np.all(np.abs(cap['capon_peak_offset'][found]) <= 0.5)
    plain = ltsva_capon(st, None, None, W / FS, 0.5, grid, 0.5, alpha=1.0, rij=rij)
    assert sorted(plain[8]) == sorted(['capon_index', 'capon_power', 'bartlett_index', 'bartlett_power', 'capon_vel', 'capon_baz',
                                       'bartlett_vel', 'bartlett_baz'])
    assert set(cap) - set(plain[8]) == {w + f for w in ('capon', 'bartlett')
                                        for f in engine.PEAK_FIELDS + ('_peak_slowness', '_peak_vel', '_peak_baz')}
    for k in plain[8]:
        assert pt.same_bits(plain[8][k], cap[k]), k
    st2 = synthetic.make_stream(data[:, ::-1].copy(), FS, starttime=T0 + 1)
    batch = ltsva_capon_batch([st, st2], None, None, W / FS, 0.5, grid, 0.5, alpha=1.0, rij=rij, peaks=2)
    assert sorted(batch[0][8]) == sorted(cap)
    for k in cap:
        assert pt.same_bits(batch[0][8][k], cap[k]), k
    fr = np.logspace(-1, 0.5, 16)
    pre = engine.process(data, FS, T0, rij, [(0.45, 0.55)], [W / FS], 0.5, 1.0, 'butter', 2, 0.01, capon_grid=grid, capon_freqs=[0.5],
                         capon_snapshots=(int(Ls[0]), int(Hs[0])), capon_peaks=2)
    nb = narrow_band_least_squares_capon([W / FS], 0.5, 1.0, st, None, None, 1, np.zeros(16), np.zeros(16), np.array([0.45, 0.55]),
                                         'log', fr, 'butter', 2, 0.01, rij=rij, slowness_grid=grid, capon_freqs=[0.5],
                                         snapshots=(int(Ls[0]), int(Hs[0])), peaks=2)[9]
    VL = pre.vel.shape[1]
    for k in PEAKS:
        assert pt.same_bits(np.ascontiguousarray(nb[k][:, :VL]), getattr(pre, k)), k
    # ... and with ltsva_capon on the band as the GPU filtered it
    filt = synthetic.make_stream(pre.handle.fetch_filtered(0), FS, starttime=T0)
    lt = ltsva_capon(filt, None, None, W / FS, 0.5, grid, 0.5, alpha=1.0, rij=rij, snapshots=(int(Ls[0]), int(Hs[0])), peaks=2)[8]
    for k in sorted(set(cap) - set(plain[8])):
        assert pt.same_bits(np.ascontiguousarray(nb[k][0, :19]), lt[k]), k
        assert not np.asarray(nb[k])[0, 19:].any(), k


def test_plain_c_caller_runs_and_agrees_with_python():
    binary = build_peaks_caller()
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'PEAKS_CALLER_OK' in r.stdout, r.stdout + r.stderr
    rows = [l.split() for l in r.stdout.splitlines() if l.startswith('P ')]
    NCH, NPTS, W = 3, 401, 65
    s = np.uint32(12345)
    base = np.empty(NCH * NPTS)
    for t in range(NCH * NPTS):
        s = np.uint32((int(s) * 1664525 + 1013904223) & 0xffffffff)
        base[t] = float(int(s) >> 8) / 8388608.0 - 1.0
    data = base.reshape(NCH, NPTS)
    rij = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    cells = np.array([(g // 3, g % 3) for g in range(9)], dtype=np.int32)
    grid = 0.3 * (cells - 1.0)
    res = engine.process(data, FS, T0, rij, [(None, None)], [(W + 0.5) / FS], 0.5, 1.0, prefiltered=True, capon_grid=grid,
                         capon_freqs=[1.0], capon_snapshots=(16, 8), capon_loading=0.01, capon_peaks=2, capon_peak_floor=0.0,
                         capon_cells=cells)
    n = int(res.nwin[0])
    assert len(rows) == 2 * n
    for row in rows:
        w, name = int(row[1]), ('capon', 'bartlett')[int(row[2])]
        idx, pw, off = (getattr(res, name + f)[0, w] for f in engine.PEAK_FIELDS[1:])
        assert int(row[3]) == getattr(res, name + '_peak_count')[0, w] and [int(row[4]), int(row[8])] == list(idx)
        got = np.array([float.fromhex(row[5]), float.fromhex(row[9]), float.fromhex(row[6]), float.fromhex(row[7])])
        assert np.array_equal(got, np.array([pw[0], pw[1], off[0, 0], off[0, 1]]), equal_nan=True)
