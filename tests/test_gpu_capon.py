"""The Capon / Bartlett slowness spectra (``nbls_set_capon``, csrc/capon.hip: capon_kernel) against the
long-double reference of tests/capon_truth.py, in its two stages: the tables within 4 * 2^-52 of NumPy's float64 expression;
R from the plan's own tables and the samples within the stage A bound; both spectra from the GPU's own R within the stage B
bounds (constants derived in capon_truth, never fitted; the tests print the worst |difference| / bound).  An index is
accepted if its power can be the largest within the bounds and must be the reference's where that one leads by more than
both.  Between the forms of a pass (streamed, batched, window slices, with or without the time-domain grid search) every
output is equal bit for bit.  All cases use prefiltered traces at fs = 20 Hz."""
import os
import subprocess
import sys

import numpy as np
import pytest

import capon_truth as ct
from test_capon_host import build_capon_caller
from test_capon_truth import two_source_case, count_both, BAZ
from narrow_band_least_squares_amd import (engine, planner, synthetic, _hip, ltsva, ltsva_capon, ltsva_capon_batch,
                                           narrow_band_least_squares_capon)

pytestmark = pytest.mark.gpu

FS = 20.0
T0 = 17884.0729166667
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, CH = _hip.CAPON_THREADS, _hip.CAPON_CHUNK
GRID = planner.slowness_grid(3.07, 5)                       # 21 points, s = 0 among them
FREQ = 1.3
FIELDS = ('capon_index', 'capon_power', 'bartlett_index', 'bartlett_power', 'capon_map', 'bartlett_map', 'capon_csdm')
PLAIN = ('vel', 'baz', 'mdccm', 'sigma_tau', 'mask')


def _wave(N, npts, seed=900, snr_db=6.0):
    rij = synthetic.array_geometry(N, 1.0)
    data = synthetic.plane_wave(rij, npts, FS, 0.5, 4.0, baz_deg=60.0, snr_db=snr_db, seed=seed)
    return data, rij - rij.mean(axis=1, keepdims=True)


def _process(data, rij, W, alpha, Ls, Hs, grid=GRID, delta=0.01, overlap=0.5, maps=True, csdm=True, **kw):
    res = engine.process(data, FS, T0, rij, [(None, None)], [(W + 0.5) / FS], overlap, alpha, prefiltered=True, capon_grid=grid,
                         capon_freqs=[FREQ], capon_snapshots=(Ls, Hs), capon_loading=delta, want_capon_maps=maps,
                         want_capon_csdm=csdm, **kw)
    assert int(res.W[0]) == W
    return res


def _against_reference(res, filt, grid, Ls, Hs, delta, label='', well_conditioned=True, band=0, freq=FREQ):
    """``band``: the band of the plan whose rows are compared, ``filt`` its samples and ``freq``, ``Ls``, ``Hs`` its tables."""
    N, W, inc, n = filt.shape[0], int(res.W[band]), int(res.inc[band]), int(res.nwin[band])
    coef, steer = res.handle.fetch_capon_tables(band)
    coef_np, steer_np = ct.tables(res.xij, grid, FS, freq, Ls, N)
    assert np.abs(coef - coef_np).max() <= ct.TABLE_TOL and np.abs(steer - steer_np).max() <= ct.TABLE_TOL
    Rref, tolA = ct.csdm_reference(filt, coef, W, inc, n, Hs)
    worst = dict(A=0.0, B=0.0, C=0.0)
    for w in range(n):
        R = res.capon_csdm[band, w]
        d = (R.astype(ct.CLD) - Rref[w])
        ok = tolA[w] > 0
        if ok.any():
            worst['A'] = max(worst['A'], float(np.max(np.maximum(np.abs(d.real), np.abs(d.imag))[ok].astype(np.float64) / tolA[w][ok])))
        assert np.all(np.abs(d.real).astype(np.float64) <= tolA[w]) and np.all(np.abs(d.imag).astype(np.float64) <= tolA[w]), (label, w)
        assert np.array_equal(R, np.conj(R.T))
        ref = ct.spectra_reference(R, steer, delta)
        if well_conditioned and ref['chol_ok']:
            assert ref['kappa'] * N * ct.U < 1e-6, 'a condition on the inputs: change the seed (%s, window %d)' % (label, w)
            if delta > 0:
                assert ref['kappa'] <= (N + delta) / delta * (1 + 1e-6)
        worst['B'] = max(worst['B'], ct.check_spectrum('%s Bartlett w=%d' % (label, w), ref['PB'], ref['tolB'], ref['index_B'],
                                                       int(res.bartlett_index[band, w]), float(res.bartlett_power[band, w]),
                                                       res.bartlett_map[band, w]))
        worst['C'] = max(worst['C'], ct.check_spectrum('%s Capon w=%d' % (label, w), ref['PC'], ref['tolC'], ref['index_C'],
                                                       int(res.capon_index[band, w]), float(res.capon_power[band, w]),
                                                       res.capon_map[band, w]))
    print('%s N=%d W=%d Ls=%d Hs=%d G=%d delta=%g: %d windows, worst |d| / bound: R %.3g, Bartlett %.3g, Capon %.3g'
          % (label, N, W, Ls, Hs, len(grid), delta, n, worst['A'], worst['B'], worst['C']))
    for k in FIELDS:                                                 # cells beyond nwin are zeros
        assert not getattr(res, k)[band, n:].any(), k
    return worst


SHAPES = [(16, 1, 1), (16, 16, 1), (65, 63, 1), (65, 64, 1), (65, 65, 7), (257, 16, 1),
          (65, 65 - (CH - 2), 1), (65, 65 - (CH - 1), 1), (65, 65 - CH, 1)]          # K = chunk - 1, chunk, chunk + 1


@pytest.mark.parametrize('W,Ls,Hs', SHAPES)
@pytest.mark.parametrize('N,alpha', [(3, 1.0), (4, 0.5), (9, 0.5), (32, 1.0)])
def test_matches_the_truth(N, alpha, W, Ls, Hs):
    """The smallest array, LTS's smallest, the bucket solver's first, and 32 elements, where the Cholesky's rows and the LDS
    are full; snapshots of one sample, one snapshot per window (rank one: the loading carries it), lengths around the 64
    lanes, 242 snapshots, and counts around the chunk."""
    K = ct.snapshot_count(W, Ls, Hs)
    assert (W, Ls, Hs) not in SHAPES[6:] or K in (CH - 1, CH, CH + 1)
    data, rij = _wave(N, max(2 * W + W // 2 + 1, 201))
    res = _process(data, rij, W, alpha, Ls, Hs)
    n = int(res.nwin[0])
    assert n >= 2
    _against_reference(res, data, GRID, Ls, Hs, 0.01, label='truth')
    assert np.all(res.capon_index[0, :n] >= 0) and np.all(res.capon_power[0, :n] > 0) and np.all(res.bartlett_power[0, :n] > 0)


@pytest.mark.parametrize('G', [1, T - 1, T + 1, 257])
def test_grid_sizes(G):
    rng = np.random.default_rng(40)
    grid = np.round(rng.uniform(-3.0, 3.0, (257, 2)), 3)[:G]
    data, rij = _wave(4, 65 * 3)
    res = _process(data, rij, 65, 1.0, 16, 8, grid=grid)
    assert res.capon_map.shape[2] == G
    _against_reference(res, data, grid, 16, 8, 0.01, label='G')


@pytest.mark.parametrize('delta', [0.01, 1e-6, 0.0])
def test_loadings(delta):
    """delta = 0: K = 50 >= N snapshots of noisy data."""
    data, rij = _wave(4, 65 * 3, snr_db=0.0)
    res = _process(data, rij, 65, 1.0, 16, 1, delta=delta)
    _against_reference(res, data, GRID, 16, 1, delta, label='loading')


def test_degenerate_units():
    W, Ls, Hs = 65, 16, 8
    data, rij = _wave(4, 2401)
    clean = _process(data, rij, W, 1.0, Ls, Hs)
    n, inc = int(clean.nwin[0]), int(clean.inc[0])
    # (1) a stretch of zeros on every channel: windows inside it have no result at all
    gap = data.copy()
    gap[:, 800:1400] = 0.0
    res = _process(gap, rij, W, 1.0, Ls, Hs)
    empty = np.array([w * inc >= 800 and w * inc + W <= 1400 for w in range(n)])
    assert empty.sum() >= 3
    for k in ('capon_index', 'bartlett_index'):
        assert np.all(getattr(res, k)[0, :n][empty] == -1) and np.all(getattr(res, k)[0, :n][~empty] >= 0)
    for k in ('capon_power', 'bartlett_power', 'capon_map', 'bartlett_map'):
        assert np.all(np.isnan(getattr(res, k)[0, :n][empty])) and np.all(np.isfinite(getattr(res, k)[0, :n][~empty]))
    _against_reference(res, gap, GRID, Ls, Hs, 0.01, label='empty windows', well_conditioned=False)
    # (2) one NaN sample: the windows that hold it are NaN / -1, the neighbours are untouched
    bad = data.copy()
    bad[1, 1000] = np.nan
    res = _process(bad, rij, W, 1.0, Ls, Hs)
    hit = np.array([w * inc <= 1000 < w * inc + W for w in range(n)])
    assert 1 <= hit.sum() <= 3
    assert np.all(res.capon_index[0, :n][hit] == -1) and np.all(res.bartlett_index[0, :n][hit] == -1)
    assert np.all(np.isnan(res.capon_map[0, :n][hit])) and np.all(np.isnan(res.bartlett_power[0, :n][hit]))
    for k in FIELDS:
        np.testing.assert_array_equal(getattr(res, k)[0, :n][~hit], getattr(clean, k)[0, :n][~hit], err_msg=k)
    # (3) one element zero throughout, no loading: a pivot of exactly 0 -> Capon NaN / -1, Bartlett finite; loaded: finite
    dead = data.copy()
    dead[2] = 0.0
    res = _process(dead, rij, W, 1.0, Ls, Hs, delta=0.0)
    assert np.all(res.capon_index[0, :n] == -1) and np.all(np.isnan(res.capon_power[0, :n])) and np.all(np.isnan(res.capon_map[0, :n]))
    assert np.all(res.bartlett_index[0, :n] >= 0) and np.all(np.isfinite(res.bartlett_map[0, :n]))
    _against_reference(res, dead, GRID, Ls, Hs, 0.0, label='dead element', well_conditioned=False)
    res = _process(dead, rij, W, 1.0, Ls, Hs, delta=0.01)
    assert np.all(res.capon_index[0, :n] >= 0) and np.all(np.isfinite(res.capon_map[0, :n]))
    _against_reference(res, dead, GRID, Ls, Hs, 0.01, label='dead element, loaded')


def _same(a, b, keys):
    for k in keys:
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg=k)


def test_streamed_in_several_batches_equals_the_unstreamed_pass(monkeypatch):
    data, rij = _wave(9, 24001)
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    whole = _process(data, rij, 1200, 0.5, 80, 40, overlap=0.75)
    h = engine.get_handle()
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '1')
    try:
        h.set_option('screen_batch_mb', 1)
        h.set_option('solve_min_units', 1)
        streamed = _process(data, rij, 1200, 0.5, 80, 40, overlap=0.75)
        assert h.result_batches() >= 2
    finally:
        h.set_option('screen_batch_mb', 192)
        h.set_option('solve_min_units', 0)
    _same(streamed, whole, FIELDS + PLAIN)
    n = int(whole.nwin[0])
    assert np.all(whole.capon_index[0, :n] >= 0)


def test_batch_of_three_recordings_equals_three_single_calls():
    recs = [_wave(4, 1201, seed=910 + i) for i in range(3)]
    rij = recs[0][1]
    sts = [synthetic.make_stream(d, FS, starttime=T0 + i) for i, (d, _) in enumerate(recs)]
    batch = ltsva_capon_batch(sts, None, None, 65.5 / FS, 0.5, GRID, FREQ, alpha=0.5, rij=rij, snapshots=(16, 8), maps=True)
    assert len(batch) == 3
    for got, st in zip(batch, sts):
        exp = ltsva_capon(st, None, None, 65.5 / FS, 0.5, GRID, FREQ, alpha=0.5, rij=rij, snapshots=(16, 8), maps=True)
        assert len(got) == len(exp) == 9 and sorted(got[8]) == sorted(exp[8]) and len(got[8]) == 10
        for i in (0, 1, 2, 3, 5, 6, 7):
            np.testing.assert_array_equal(got[i], exp[i], err_msg='return %d' % i)
        for k in exp[8]:
            np.testing.assert_array_equal(got[8][k], exp[8][k], err_msg=k)
        assert got[8]['capon_index'].dtype == np.int32 and np.all(got[8]['capon_index'] >= 0)
    assert not np.array_equal(batch[0][8]['capon_power'], batch[1][8]['capon_power'])
    plain = ltsva(sts[0], None, None, 65.5 / FS, 0.5, alpha=0.5, rij=rij)
    for i in (0, 1, 3, 5):
        np.testing.assert_array_equal(plain[i], batch[0][i])


def test_two_window_slices_add_up_to_the_full_call():
    data, rij = _wave(4, 2401)
    full = _process(data, rij, 65, 0.5, 16, 8)
    parts = [_process(data, rij, 65, 0.5, 16, 8, window_slice=(k, 2)) for k in range(2)]
    for k in FIELDS:
        a, b = getattr(parts[0], k), getattr(parts[1], k)
        assert not np.any((a != 0) & (b != 0))                     # rows outside a slice stay zero
        np.testing.assert_array_equal(a + b, getattr(full, k), err_msg=k)


def test_with_and_without_the_grid_search_and_the_seed():
    data, rij = _wave(4, 2401)
    alone = _process(data, rij, 65, 0.5, 16, 8)
    plain = engine.process(data, FS, T0, rij, [(None, None)], [65.5 / FS], 0.5, 0.5, prefiltered=True)
    _same(alone, plain, PLAIN)                                       # the plain results do not know about the spectra
    assert plain.capon_index is None and plain.capon_map is None and plain.capon_csdm is None
    grid2 = planner.slowness_grid(3.0, 3)
    with_grid = _process(data, rij, 65, 0.5, 16, 8, slowness_grid=grid2)
    _same(with_grid, alone, FIELDS + PLAIN)
    assert with_grid.grid_index is not None
    seeded = _process(data, rij, 65, 0.5, 16, 8, slowness_grid=grid2, seed_halfwidths=6)
    _same(seeded, alone, FIELDS)
    just_seeded = engine.process(data, FS, T0, rij, [(None, None)], [65.5 / FS], 0.5, 0.5, prefiltered=True, slowness_grid=grid2,
                                 seed_halfwidths=6)
    _same(seeded, just_seeded, PLAIN + ('grid_index', 'grid_fstat'))


def test_results_that_were_not_asked_for_and_a_pass_without_solve():
    data, rij = _wave(4, 1201)
    engine.process(data, FS, T0, rij, [(None, None)], [65.5 / FS], 0.5, 1.0, prefiltered=True)
    h = engine.get_handle()
    for fetch in (h.fetch_capon, h.fetch_capon_maps, h.fetch_capon_csdm, lambda: h.fetch_capon_tables(0)):
        with pytest.raises(_hip.NblsError) as err:
            fetch()
        assert err.value.code == _hip.NBLS_ERR_STATE
    res = _process(data, rij, 65, 1.0, 16, 8, maps=False, csdm=False)
    h = res.handle
    assert res.capon_map is None and res.capon_csdm is None
    for fetch in (h.fetch_capon_maps, h.fetch_capon_csdm):
        with pytest.raises(_hip.NblsError) as err:
            fetch()
        assert err.value.code == _hip.NBLS_ERR_STATE
    before = h.fetch_capon()
    np.testing.assert_array_equal(before[1], res.capon_power)
    assert np.any(before[1] != 0)
    h.execute(stages=3)                                          # filter and correlation only
    for a, b in zip(h.fetch_capon(), before):
        np.testing.assert_array_equal(a, b)
    h.set_capon(GRID, [FREQ], [16], [8])
    try:
        h.plan(None, False, None, None, [65], [32], 40)
    finally:
        h.set_capon(None)
    assert not any(a.any() for a in h.fetch_capon())             # a fresh plan has zeros until a pass has run the solve stage


def test_refusals_of_the_library():
    data, rij = _wave(4, 1201)
    res = engine.process(data, FS, T0, rij, [(None, None)], [65.5 / FS], 0.5, 1.0, prefiltered=True)
    h = res.handle
    plan = lambda nb=1: h.plan(None, False, None, None, [65] * nb, [32] * nb, 40)
    for bad in (dict(grid=np.zeros((0, 2))), dict(grid=np.zeros((_hip.CAPON_GRID_MAX + 1, 2))), dict(grid=[[np.nan, 0.0]]),
                dict(grid=[[0.0, np.inf]]), dict(freqs=[0.0]), dict(freqs=[np.inf]), dict(freqs=[np.nan]), dict(snap_len=[0]),
                dict(snap_hop=[0]), dict(loading=-0.01), dict(loading=np.nan), dict(loading=np.inf),
                dict(freqs=[], snap_len=[], snap_hop=[])):
        kw = dict(dict(grid=GRID, freqs=[FREQ], snap_len=[16], snap_hop=[8], loading=0.01), **bad)
        with pytest.raises(ValueError):
            h.set_capon(**kw)
    plan()                                                       # the handle is unchanged: the plain plan
    with pytest.raises(_hip.NblsError):
        h.fetch_capon()
    try:
        h.set_capon(GRID, [FREQ, FREQ], [16, 16], [8, 8])        # two bands of tables for a plan of one
        with pytest.raises(ValueError, match='bands'):
            plan()
        h.set_capon(GRID, [FREQ], [66], [8])                     # a snapshot longer than the window
        with pytest.raises(ValueError, match='longer'):
            plan()
        h.set_capon(GRID, [FREQ], [63], [1], loading=0.0)        # K = 3 < N = 4 without loading
        with pytest.raises(ValueError, match='singular'):
            plan()
        h.set_capon(GRID, [FREQ], [62], [1], loading=0.0)        # K = 4
        plan()
        big = np.zeros((_hip.CAPON_GRID_MAX, 2))
        nb = 2 ** 30 // (len(big) * 4 * 16) + 1
        h.set_capon(big, [FREQ] * nb, [16] * nb, [8] * nb)
        with pytest.raises(ValueError, match='1 GiB'):
            plan(nb)
    finally:
        h.set_capon(None)
    fresh = _hip.Handle(0)
    try:
        fresh.set_trace(data, FS)
        fresh.set_capon(GRID, [FREQ], [16], [8])
        with pytest.raises(_hip.NblsError) as err:               # no geometry
            fresh.plan(None, False, None, None, [65], [32], 40)
        assert err.value.code == _hip.NBLS_ERR_STATE
    finally:
        fresh.close()


def test_rccl_communicator_refuses_the_spectra_at_plan_time():
    """A communicator lives as long as its process: a child process over the tests' loopback transport."""
    src = os.path.join(ROOT, 'tests', 'c_caller', 'loopback_rccl.cpp')
    lib = os.path.join(ROOT, 'tests', 'c_caller', 'libloopback_rccl.so')
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.run(['/opt/rocm/bin/hipcc', '-O2', '-shared', '-fPIC', '--offload-arch=gfx950', src, '-o', lib], check=True,
                       timeout=300)
    env = dict(os.environ, NBLS_TEST_TRANSPORT=lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_capon_comm_worker.py')], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and 'CAPON_COMM_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def _count_on_patch(maps, grid, shape):
    return count_both(maps, grid, shape)


def test_two_sources_through_the_public_call():
    """N = 8, a 21 x 21 patch of the grid around the two sources, 19 windows of 2400 samples: the GPU's count of windows
    with both sources is within 1 of the truth's (near-ties at the 0.25 threshold are the only licence), and the truth's is
    at least 15."""
    rij, data, _, _, W, inc = two_source_case()
    N = rij.shape[1]
    centre = np.array([np.sin(np.radians(np.mean(BAZ))), np.cos(np.radians(np.mean(BAZ)))]) / 0.34
    ax = np.arange(-10, 11) * 0.1
    g0, g1 = np.meshgrid(centre[0] + ax, centre[1] + ax, indexing='ij')
    grid = np.ascontiguousarray(np.stack([g0.ravel(), g1.ravel()], axis=1))
    st = synthetic.make_stream(data, FS, starttime=T0)
    out = ltsva_capon(st, None, None, W / FS, 0.5, grid, 0.5, alpha=1.0, rij=rij, maps=True)
    cap = out[8]
    assert cap['capon_map'].shape == (19, 441)
    xij = planner.co_array(rij)[0]
    Ls, Hs = planner.capon_snapshots(xij, grid, FS, [0.5], [W])
    coef, steer = ct.tables(xij, grid, FS, 0.5, Ls[0], N)
    R, _ = ct.csdm_reference(data, coef, W, inc, 19, int(Hs[0]))
    refs = [ct.spectra_reference(R[w].astype(np.complex128), steer, 0.01) for w in range(19)]
    truth = _count_on_patch([r['PC'] for r in refs], grid, (21, 21))
    gpu = _count_on_patch(cap['capon_map'], grid, (21, 21))
    gpu_b = _count_on_patch(cap['bartlett_map'], grid, (21, 21))
    print('two sources on the patch: Capon GPU %d / 19, truth %d / 19; Bartlett GPU %d / 19' % (gpu, truth, gpu_b))
    assert truth >= 15
    assert abs(gpu - truth) <= 1
    vel, baz = cap['capon_vel'], cap['capon_baz']
    assert np.all(np.isfinite(vel)) and np.all((baz > BAZ[0] - 15) & (baz < BAZ[1] + 15))


def test_plain_c_caller_runs_and_agrees_with_python():
    binary = build_capon_caller()
    r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'CAPON_CALLER_OK' in r.stdout, r.stdout + r.stderr
    rows = [l.split() for l in r.stdout.splitlines() if l.startswith('W ')]
    # the caller's trace, geometry and tables, through the Python path
    NCH, NPTS, W, INC = 3, 401, 65, 32
    s = np.uint32(12345)
    base = np.empty(NCH * NPTS)
    for t in range(NCH * NPTS):
        s = np.uint32((int(s) * 1664525 + 1013904223) & 0xffffffff)
        base[t] = float(int(s) >> 8) / 8388608.0 - 1.0
    data = base.reshape(NCH, NPTS)
    rij = np.array([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    grid = np.array([[0.0, 0.0], [-0.3, 0.2], [0.3, -0.2], [1.0, 1.0]])
    res = engine.process(data, FS, T0, rij, [(None, None)], [(W + 0.5) / FS], 0.5, 1.0, prefiltered=True, capon_grid=grid,
                         capon_freqs=[1.0], capon_snapshots=(16, 8), capon_loading=0.01)
    n = int(res.nwin[0])
    assert len(rows) == n
    for w, row in enumerate(rows):
        assert int(row[1]) == w and int(row[2]) == res.capon_index[0, w] and int(row[4]) == res.bartlett_index[0, w]
        assert float.fromhex(row[3]) == res.capon_power[0, w] and float.fromhex(row[5]) == res.bartlett_power[0, w]


def test_narrow_band_call_filters_on_the_gpu_and_pads_with_zeros():
    """Two bands filtered on the GPU, default frequencies and snapshots: the dict of ``narrow_band_least_squares_capon`` is
    what ``engine.process`` gives for the same keywords, bit for bit; each band agrees with the reference on the filtered
    samples the kernel read; cells beyond a band's windows are zeros."""
    data, rij = _wave(4, 2401)
    st = synthetic.make_stream(data, FS, starttime=T0)
    freqlist = np.array([0.5, 1.5, 4.0])
    fr = np.logspace(-1, 0.5, 16)
    winlens = [257.5 / FS, 65.5 / FS]
    out = narrow_band_least_squares_capon(winlens, 0.5, 1.0, st, None, None, 2, np.zeros(16), np.zeros(16),
                                          freqlist, 'log', fr, 'butter', 2, 0.01, rij=rij, slowness_grid=GRID, maps=True)
    assert len(out) == 10
    cap = out[9]
    edges = [(0.5, 1.5), (1.5, 4.0)]
    f = planner.capon_frequencies(edges)
    snaps = planner.capon_snapshots(planner.co_array(rij)[0], GRID, FS, f, [257, 65])
    res = engine.process(data, FS, T0, rij, edges, winlens, 0.5, 1.0, 'butter', 2, 0.01, capon_grid=GRID, capon_freqs=f,
                         capon_snapshots=snaps, want_capon_maps=True, want_capon_csdm=True)
    assert [int(w) for w in res.W] == [257, 65] and res.nwin[0] != res.nwin[1]
    VL = res.vel.shape[1]                                            # (the reference's rows are longer than the longest band)
    assert out[0].shape[1] >= VL
    for k in ('capon_index', 'capon_power', 'bartlett_index', 'bartlett_power', 'capon_map', 'bartlett_map'):
        np.testing.assert_array_equal(cap[k][:, :VL], getattr(res, k), err_msg=k)
    np.testing.assert_array_equal(out[0][:, :VL], res.vel)
    for b in range(2):
        n = int(res.nwin[b])
        assert np.all(cap['capon_index'][b, :n] >= 0) and np.all(np.isfinite(cap['capon_vel'][b, :n]) | (cap['capon_vel'][b, :n] == np.inf))
        for k in cap:
            assert not np.asarray(cap[k])[b, n:].any(), k
        filt = res.handle.fetch_filtered(b)
        coef, steer = res.handle.fetch_capon_tables(b)
        coef_np, steer_np = ct.tables(res.xij, GRID, FS, f[b], snaps[0][b], 4)
        assert np.abs(coef - coef_np).max() <= ct.TABLE_TOL and np.abs(steer - steer_np).max() <= ct.TABLE_TOL
        Rref, tolA = ct.csdm_reference(filt, coef, int(res.W[b]), int(res.inc[b]), n, int(snaps[1][b]))
        for w in range(n):
            d = res.capon_csdm[b, w].astype(ct.CLD) - Rref[w]
            assert np.all(np.abs(d.real).astype(np.float64) <= tolA[w]) and np.all(np.abs(d.imag).astype(np.float64) <= tolA[w])
            ref = ct.spectra_reference(res.capon_csdm[b, w], steer, 0.01)
            ct.check_spectrum('band %d w=%d Capon' % (b, w), ref['PC'], ref['tolC'], ref['index_C'], int(res.capon_index[b, w]),
                              float(res.capon_power[b, w]), res.capon_map[b, w])
            ct.check_spectrum('band %d w=%d Bartlett' % (b, w), ref['PB'], ref['tolB'], ref['index_B'], int(res.bartlett_index[b, w]),
                              float(res.bartlett_power[b, w]), res.bartlett_map[b, w])
