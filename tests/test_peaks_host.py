"""Host side of the peak request of the Capon / Bartlett spectra (``nbls_set_capon_peaks``): the planner's
lattice, every ``ValueError`` before any GPU call, the header's declarations and their bindings, the public keywords, and the
plain C caller.  CPU only."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import narrow_band_least_squares_amd as pkg
from narrow_band_least_squares_amd import _hip, engine, lts_array, planner, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, 'tests', 'c_caller')
LIBDIR = os.path.join(ROOT, 'narrow_band_least_squares_amd', 'csrc')
SYMBOLS = ['nbls_set_capon_peaks', 'nbls_fetch_capon_peaks']
FS = 20.0
GRID = planner.slowness_grid(3.0, 5)


def test_grid_cells_of_a_slowness_grid_are_the_meshgrid_indices():
    for s, n in ((3.0, 5), (4.0, 9), (4.0, 41), (3.07, 5)):
        grid = planner.slowness_grid(s, n)
        cells, steps = planner.grid_cells(grid)
        ax = np.linspace(-s, s, n)
        i0, i1 = np.meshgrid(np.arange(n), np.arange(n), indexing='ij')
        keep = np.hypot(ax[i0.ravel()], ax[i1.ravel()]) <= s
        assert cells.dtype == np.int32 and cells.flags.c_contiguous and steps.dtype == np.float64
        np.testing.assert_array_equal(cells, np.stack([i0.ravel(), i1.ravel()], axis=1)[keep])
        np.testing.assert_allclose(steps, [2 * s / (n - 1)] * 2, rtol=1e-12)


def test_grid_cells_of_other_lattices():
    # a sub-sampled lattice: the step is the smallest difference that occurs, the cells skip
    grid = np.array([[0.0, 0.0], [0.5, 0.0], [1.5, 0.25], [3.0, 1.0]])
    cells, steps = planner.grid_cells(grid)
    np.testing.assert_array_equal(cells, [[0, 0], [1, 0], [3, 1], [6, 4]])
    np.testing.assert_array_equal(steps, [0.5, 0.25])
    # a one-point axis, and one point
    cells, steps = planner.grid_cells([[1.0, 2.0], [1.0, 2.5], [1.0, 4.0]])
    np.testing.assert_array_equal(cells, [[0, 0], [0, 1], [0, 4]])
    np.testing.assert_array_equal(steps, [0.0, 0.5])
    cells, steps = planner.grid_cells([[0.3, -0.2]])
    np.testing.assert_array_equal(cells, [[0, 0]])
    np.testing.assert_array_equal(steps, [0.0, 0.0])
    # values within 1e-9 of the span count as equal
    cells, steps = planner.grid_cells([[0.0, 0.0], [1.0, 0.0], [1.0 + 1e-10, 1.0], [2.0, 1.0]])
    np.testing.assert_array_equal(cells, [[0, 0], [1, 0], [1, 1], [2, 1]])
    np.testing.assert_allclose(steps, [1.0, 1.0], rtol=1e-9)


def test_grid_cells_refuses():
    with pytest.raises(ValueError, match='lattice'):
        planner.grid_cells([[0.0, 0.0], [1.0, 0.0], [1.5 + 1e-3, 0.0], [2.5 + 1e-3, 0.0]])       # 1e-3 step off
    with pytest.raises(ValueError, match='share'):
        planner.grid_cells([[0.0, 0.0], [1.0, 1.0], [1.0, 1.0]])
    with pytest.raises(ValueError, match='32768|lattice steps'):
        planner.grid_cells([[0.0, 0.0], [1.0, 0.0], [32768.0, 0.0]])
    planner.grid_cells([[0.0, 0.0], [1.0, 0.0], [32767.0, 0.0]])
    for bad in (np.zeros((0, 2)), [[np.nan, 0.0]], np.zeros((3, 3)), 'x'):
        with pytest.raises(ValueError):
            planner.grid_cells(bad)


CELLS = planner.grid_cells(GRID)[0]
BAD = [dict(K=0), dict(K=9), dict(K=-1), dict(K=2.0), dict(K=True), dict(K='2'), dict(floor=-0.01), dict(floor=1.01),
       dict(floor=np.nan), dict(floor='x'), dict(floor=None), dict(cells=CELLS[:-1]), dict(cells=CELLS.astype(float)),
       dict(cells=CELLS.ravel()), dict(cells=np.where(CELLS == 0, -1, CELLS)), dict(cells=CELLS + 32768 - 4),
       dict(cells=np.vstack([CELLS[:-1], CELLS[:1]])), dict(cells='x'), dict(grid_len=len(GRID) + 1)]


@pytest.mark.parametrize('bad', BAD, ids=[','.join(b) + str(i) for i, b in enumerate(BAD)])
def test_check_capon_peaks_refuses(bad):
    good = dict(grid_len=len(GRID), cells=CELLS, K=2, floor=0.25)
    planner.check_capon_peaks(**good)
    with pytest.raises(ValueError):
        planner.check_capon_peaks(**dict(good, **bad))


def test_check_capon_peaks_returns():
    c, K, f = planner.check_capon_peaks(len(GRID), CELLS.tolist(), np.int64(8), 1)
    assert c.dtype == np.int32 and c.flags.c_contiguous and K == 8 and isinstance(K, int) and f == 1.0 and isinstance(f, float)
    np.testing.assert_array_equal(c, CELLS)
    planner.check_capon_peaks(len(GRID), CELLS + 32767 - 4, 1, 0.0)
    assert planner.MAX_CAPON_PEAKS == _hip.CAPON_PEAKS_MAX


def _no_gpu(monkeypatch):
    def boom(*a, **k):
        raise AssertionError('a GPU call was made')
    monkeypatch.setattr(engine, 'get_handle', boom)
    monkeypatch.setattr(engine, 'start_upload', boom)


def test_every_value_error_comes_before_any_gpu_call(monkeypatch):
    _no_gpu(monkeypatch)
    rij = synthetic.array_geometry(4, 1.0)
    data = np.random.default_rng(3).standard_normal((4, 1201))
    st = synthetic.make_stream(data, FS)
    ragged = np.random.default_rng(4).uniform(-3.0, 3.0, (21, 2))                   # no lattice
    call = lambda **kw: engine.process(data, FS, 0.0, rij, [(None, None)], [65.5 / FS], 0.5, 1.0, prefiltered=True,
                                       **dict(dict(capon_grid=GRID, capon_freqs=[1.0], capon_snapshots=(16, 8), capon_peaks=2), **kw))
    for bad in (dict(capon_peaks=9), dict(capon_peaks=-1), dict(capon_peaks=1.5), dict(capon_peaks=True), dict(capon_peak_floor=2.0),
                dict(capon_peak_floor=np.nan), dict(capon_cells=CELLS[:-1]), dict(capon_cells=np.zeros((len(GRID), 2), dtype=int)),
                dict(capon_cells=CELLS - 1), dict(capon_grid=ragged), dict(capon_grid=None, capon_freqs=None, capon_snapshots=None),
                dict(capon_peaks=0, capon_cells=CELLS)):
        with pytest.raises(ValueError):
            call(**bad)
    with pytest.raises(ValueError):
        engine.process_batch([list(data), list(data)], FS, [0.0, 1.0], rij, [(None, None)], [65.5 / FS], 0.5, 1.0, prefiltered=True,
                             capon_grid=GRID, capon_freqs=[1.0], capon_snapshots=(16, 8), capon_peaks=9)
    for bad in (dict(peaks=9), dict(peaks=-1), dict(peaks='two'), dict(peak_floor=1.5), dict(peak_floor=np.nan),
                dict(slowness_grid=ragged)):
        kw = dict(dict(slowness_grid=GRID, freq=1.0, peaks=2), **bad)
        with pytest.raises(ValueError):
            lts_array.ltsva_capon(st, None, None, 65.5 / FS, 0.5, kw.pop('slowness_grid'), kw.pop('freq'), rij=rij, **kw)
        kw = dict(dict(slowness_grid=GRID, freq=1.0, peaks=2), **bad)
        with pytest.raises(ValueError):
            lts_array.ltsva_capon_batch([st, st], None, None, 65.5 / FS, 0.5, kw.pop('slowness_grid'), kw.pop('freq'), rij=rij, **kw)
    fr = np.logspace(-1, 0.5, 16)
    args = ([10.0, 10.0], 0.5, 1.0, st, None, None, 2, np.zeros(16), np.zeros(16), np.array([0.5, 1.0, 2.0]), 'log', fr, 'butter', 2, 0.01)
    for bad in (dict(peaks=9), dict(peak_floor=-0.5), dict(slowness_grid=ragged)):
        with pytest.raises(ValueError):
            pkg.narrow_band_least_squares_capon(*args, rij=rij, **dict(dict(slowness_grid=GRID, peaks=2), **bad))


def test_process_segmented_refuses_the_peaks_with_the_spectra(monkeypatch):
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', '1e-9')
    _no_gpu(monkeypatch)
    rij = synthetic.array_geometry(4, 1.0)
    data = np.random.default_rng(3).standard_normal((4, 1201))
    with pytest.raises(ValueError, match='time-segmented'):
        engine.process(data, FS, 0.0, rij, [(0.5, 2.0)], [65.5 / FS], 0.5, 1.0, 'butter', 2, 0.01, capon_grid=GRID, capon_freqs=[1.0],
                       capon_snapshots=(16, 8), capon_peaks=2)
    with pytest.raises(ValueError, match='capon_grid'):
        engine.process(data, FS, 0.0, rij, [(0.5, 2.0)], [65.5 / FS], 0.5, 1.0, 'butter', 2, 0.01, capon_peaks=2)


def test_header_declares_and_the_binding_knows_every_entry_point():
    header = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    for sym in SYMBOLS:
        assert re.search(r'^int %s\(nbls_handle\* h' % sym, header, re.M), sym
        assert sym in _hip.EXPORTS
    assert re.search(r'^#define NBLS_CAPON_PEAKS_MAX %d$' % _hip.CAPON_PEAKS_MAX, header, re.M)
    lib = _hip.load_library()
    for sym in SYMBOLS:
        assert getattr(lib, sym).argtypes is not None, sym
    assert callable(_hip.Handle.set_capon_peaks) and callable(_hip.Handle.fetch_capon_peaks)


def test_public_names_and_keywords():
    for name in ('ltsva_capon', 'ltsva_capon_batch', 'narrow_band_least_squares_capon'):
        par = inspect.signature(getattr(pkg, name)).parameters
        assert list(par)[-2:] == ['peaks', 'peak_floor'] and par['peaks'].default == 0 and par['peak_floor'].default == 0.25, name
    for f in (engine.process, engine.process_batch):
        par = inspect.signature(f).parameters
        assert par['capon_peaks'].default == 0 and par['capon_peak_floor'].default == 0.25 and par['capon_cells'].default is None
    assert callable(planner.grid_cells) and callable(planner.check_capon_peaks) and callable(lts_array.peak_slowness)
    res = engine.new_result(4, 1.0, FS, np.array([65]), np.array([32]), np.array([3]), 5, capon_points=21, capon_peaks=3)
    assert res.capon_peak_count.shape == (1, 5) and res.capon_peak_count.dtype == np.int32
    assert res.bartlett_peak_index.shape == (1, 5, 3) and res.bartlett_peak_index.dtype == np.int32
    assert res.capon_peak_power.shape == (1, 5, 3) and res.bartlett_peak_offset.shape == (1, 5, 3, 2)
    assert engine.new_result(4, 1.0, FS, np.array([65]), np.array([32]), np.array([3]), 5, capon_points=21).capon_peak_count is None


def test_peak_slowness():
    grid = planner.slowness_grid(1.0, 3)                             # 5 points of the 3 x 3 lattice, step 1
    steps = planner.grid_cells(grid)[1]
    idx = np.array([[2, -1]])
    off = np.array([[[0.25, -0.5], [np.nan, np.nan]]])
    s, vel, baz = lts_array.peak_slowness(grid, steps, idx, off)
    np.testing.assert_array_equal(s[0, 0], grid[2] + np.array([0.25, -0.5]))
    assert np.all(np.isnan(s[0, 1])) and np.isnan(vel[0, 1]) and np.isnan(baz[0, 1])
    assert vel[0, 0] == 1.0 / np.hypot(*s[0, 0]) and baz[0, 0] == np.mod(np.arctan2(s[0, 0, 0], s[0, 0, 1]) * 180.0 / np.pi - 360.0, 360.0)
    v0, b0 = lts_array.grid_slowness(grid, np.array([1, 3]))         # offset 0: the grid's own slowness
    _, v1, b1 = lts_array.peak_slowness(grid, steps, np.array([1, 3]), np.zeros((2, 2)))
    np.testing.assert_array_equal(v0, v1)
    np.testing.assert_array_equal(b0, b1)


def build_peaks_caller():
    binary = os.path.join(CDIR, 'peaks_caller')
    cmd = ['gcc', '-O1', '-Wall', '-Wextra', '-Werror', '-std=c11', '-pthread', '-I', os.path.join(ROOT, 'include'),
           os.path.join(CDIR, 'peaks_caller.c'), '-o', binary, '-L', LIBDIR, '-lnbls_hip', '-lm',
           '-Wl,-rpath,$ORIGIN/../../narrow_band_least_squares_amd/csrc', '-Wl,-rpath-link,/opt/rocm/lib']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return binary


def test_plain_c_caller_compiles_and_links():
    binary = build_peaks_caller()
    out = subprocess.run(['nm', '-u', binary], capture_output=True, text=True).stdout
    assert set(SYMBOLS) | {'nbls_set_capon', 'nbls_plan', 'nbls_execute'} <= set(re.findall(r'\b(nbls_[a-z0-9_]+)', out))
