"""Host side of the Capon / Bartlett spectra (``nbls_set_capon``): the planner's functions, every
``ValueError`` before any GPU call, the header's declarations and their bindings, and the plain C caller.  CPU only."""
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
SYMBOLS = ['nbls_set_capon', 'nbls_fetch_capon', 'nbls_fetch_capon_maps', 'nbls_fetch_capon_csdm', 'nbls_fetch_capon_tables']
FS = 20.0
GRID = planner.slowness_grid(3.0, 5)


def test_public_names():
    for name in ('ltsva_capon', 'ltsva_capon_batch', 'narrow_band_least_squares_capon'):
        assert name in pkg.__all__ and callable(getattr(pkg, name))


def test_header_declares_and_the_binding_knows_every_entry_point():
    header = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    for sym in SYMBOLS:
        assert re.search(r'^int %s\(nbls_handle\* h' % sym, header, re.M), sym
        assert sym in _hip.EXPORTS
    for name, value in (('NBLS_CAPON_GRID_MAX', _hip.CAPON_GRID_MAX), ('NBLS_CAPON_MAX_ELEMENTS', _hip.CAPON_MAX_ELEMENTS),
                        ('NBLS_CAPON_THREADS', _hip.CAPON_THREADS), ('NBLS_CAPON_CHUNK', _hip.CAPON_CHUNK),
                        ('NBLS_CAPON_MAPS', _hip.CAPON_MAPS), ('NBLS_CAPON_CSDM', _hip.CAPON_CSDM)):
        assert re.search(r'^#define %s %d$' % (name, value), header, re.M), name
    assert planner.MAX_CAPON_ELEMENTS == _hip.CAPON_MAX_ELEMENTS
    lib = _hip.load_library()
    for sym in SYMBOLS:
        assert getattr(lib, sym).argtypes is not None, sym


def test_capon_frequencies():
    np.testing.assert_allclose(planner.capon_frequencies([(0.45, 0.55), (1.0, 4.0)]), [np.sqrt(0.45 * 0.55), 2.0], rtol=1e-15)
    for bad in ([], [(0.0, 1.0)], [(1.0, np.inf)], [(1.0,)], 'x', [(None, None)]):
        with pytest.raises(ValueError):
            planner.capon_frequencies(bad)


def test_capon_snapshots():
    rij = synthetic.array_geometry(8, 1.0)
    xij = planner.co_array(rij)[0]
    tau = np.abs(xij[:7] @ GRID.T).max()
    Ls, Hs = planner.capon_snapshots(xij, GRID, FS, [0.5, 4.0, 0.01], [2400, 2400, 2400])
    assert Ls.dtype == np.int32 and Hs.dtype == np.int32
    assert list(Ls) == [max(80, int(np.ceil(2 * FS * tau))), max(10, int(np.ceil(2 * FS * tau))), 2400]
    assert list(Hs) == [l // 2 for l in Ls]
    Ls, Hs = planner.capon_snapshots(xij, [[0.0, 0.0]], 1.0, [4.0], [5])
    assert list(Ls) == [1] and list(Hs) == [1]
    with pytest.raises(ValueError):
        planner.capon_snapshots(xij, GRID, FS, [0.0], [100])
    with pytest.raises(ValueError):
        planner.capon_snapshots(xij, GRID, 0.0, [1.0], [100])
    with pytest.raises(ValueError):
        planner.capon_snapshots(xij, GRID, FS, [1.0, 2.0], [100])


GOOD = dict(nchans=4, grid=GRID, freqs=[1.0], snapshots=(16, 8), loading=0.01, W_list=[65])
BAD = [dict(grid=np.zeros((0, 2))), dict(grid=np.zeros((planner.MAX_GRID_POINTS + 1, 2))), dict(grid=[[np.nan, 0.0]]),
       dict(grid=[[0.0, np.inf]]), dict(grid=np.zeros((3, 3))), dict(freqs=[0.0]), dict(freqs=[-1.0]), dict(freqs=[np.inf]),
       dict(freqs=[np.nan]), dict(freqs=[1.0, 2.0]), dict(freqs=['a']), dict(snapshots=(0, 8)), dict(snapshots=(16, 0)),
       dict(snapshots=(16.5, 8)), dict(snapshots=(66, 8)), dict(snapshots=16), dict(snapshots=([16, 16], 8)),
       dict(loading=-1e-9), dict(loading=np.nan), dict(loading=np.inf), dict(loading=True), dict(loading='x'),
       dict(loading=0.0, snapshots=(63, 1)), dict(nchans=33), dict(nchans=2), dict(maps=1), dict(csdm='yes'),
       dict(grid=np.zeros((65536, 2)), freqs=[1.0] * 257, W_list=[65] * 257)]


@pytest.mark.parametrize('bad', BAD, ids=[','.join(b) + str(i) for i, b in enumerate(BAD)])
def test_check_capon_refuses(bad):
    planner.check_capon(**GOOD)
    with pytest.raises(ValueError):
        planner.check_capon(**dict(GOOD, **bad))


def test_check_capon_returns():
    g, f, ls, hs, d = planner.check_capon(4, GRID.tolist(), [1, 2], (16, [8, 4]), 0, [65, 33])
    assert g.dtype == np.float64 and g.flags.c_contiguous and f.dtype == np.float64 and d == 0.0
    assert ls.dtype == np.int32 and list(ls) == [16, 16] and list(hs) == [8, 4]
    planner.check_capon(4, GRID, [1.0], (62, 1), 0.0, [65])          # K = 4 = N


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
    call = lambda **kw: engine.process(data, FS, 0.0, rij, [(None, None)], [65.5 / FS], 0.5, 1.0, prefiltered=True,
                                       **dict(dict(capon_grid=GRID, capon_freqs=[1.0], capon_snapshots=(16, 8)), **kw))
    for bad in (dict(capon_grid=[[np.nan, 0.0]]), dict(capon_freqs=[0.0]), dict(capon_snapshots=(66, 8)), dict(capon_loading=-1.0),
                dict(capon_freqs=None), dict(capon_snapshots=None), dict(want_capon_maps=2), dict(capon_freqs=[1.0, 2.0]),
                dict(capon_loading=0.0, capon_snapshots=(63, 1)), dict(capon_grid=None, want_capon_maps=True)):
        with pytest.raises(ValueError):
            call(**bad)
    with pytest.raises(ValueError):
        engine.process_batch([list(data), list(data)], FS, [0.0, 1.0], rij, [(None, None)], [65.5 / FS], 0.5, 1.0, prefiltered=True,
                             capon_grid=GRID, capon_freqs=[1.0], capon_snapshots=(66, 8))
    for bad in (dict(slowness_grid=[[np.inf, 0.0]]), dict(freq=-1.0), dict(snapshots=(0, 1)), dict(loading=np.nan), dict(maps='no')):
        kw = dict(dict(slowness_grid=GRID, freq=1.0), **bad)
        with pytest.raises(ValueError):
            lts_array.ltsva_capon(st, None, None, 65.5 / FS, 0.5, kw.pop('slowness_grid'), kw.pop('freq'), rij=rij, **kw)
        kw = dict(dict(slowness_grid=GRID, freq=1.0), **bad)
        with pytest.raises(ValueError):
            lts_array.ltsva_capon_batch([st, st], None, None, 65.5 / FS, 0.5, kw.pop('slowness_grid'), kw.pop('freq'), rij=rij, **kw)
    with pytest.raises(ValueError):
        lts_array.ltsva_capon(synthetic.make_stream(data[:2], FS), None, None, 65.5 / FS, 0.5, GRID, 1.0, rij=rij[:, :2])
    fr = np.logspace(-1, 0.5, 16)
    args = ([10.0, 10.0], 0.5, 1.0, st, None, None, 2, np.zeros(16), np.zeros(16), np.array([0.5, 1.0, 2.0]), 'log', fr, 'butter', 2, 0.01)
    with pytest.raises(TypeError):                                 # the grid is a required keyword
        pkg.narrow_band_least_squares_capon(*args, rij=rij)
    for bad in (dict(slowness_grid=np.zeros((2, 3))), dict(capon_freqs=[1.0]), dict(snapshots=(0, 1)), dict(loading=-1.0), dict(maps=None)):
        with pytest.raises(ValueError):
            pkg.narrow_band_least_squares_capon(*args, rij=rij, **dict(dict(slowness_grid=GRID), **bad))


def test_process_segmented_refuses_capon(monkeypatch):
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', '1e-9')
    _no_gpu(monkeypatch)
    rij = synthetic.array_geometry(4, 1.0)
    data = np.random.default_rng(3).standard_normal((4, 1201))
    with pytest.raises(ValueError, match='time-segmented'):
        engine.process(data, FS, 0.0, rij, [(0.5, 2.0)], [65.5 / FS], 0.5, 1.0, 'butter', 2, 0.01, capon_grid=GRID, capon_freqs=[1.0],
                       capon_snapshots=(16, 8))


def test_plane_waves():
    rij = synthetic.array_geometry(4, 1.0)
    one = synthetic.plane_waves(rij, 2000, FS, 0.5, 2.0, [(60.0, 0.34, 1.0)], snr_db=200.0, seed=5)
    two = synthetic.plane_waves(rij, 2000, FS, 0.5, 2.0, [(60.0, 0.34, 1.0), (200.0, 0.5, 2.0)], snr_db=200.0, seed=5)
    assert one.shape == two.shape == (4, 2000)
    assert abs(one[0].std() - 1.0) < 1e-6 and 2.0 < two[0].std() < 2.5
    spec = np.abs(np.fft.rfft(two[1]))
    f = np.fft.rfftfreq(2000, 1.0 / FS)
    assert spec[(f < 0.45) | (f > 2.05)].max() < 1e-6 * spec.max()
    np.testing.assert_array_equal(two, synthetic.plane_waves(rij, 2000, FS, 0.5, 2.0, [(60.0, 0.34, 1.0), (200.0, 0.5, 2.0)], 200.0, 5))


def build_capon_caller():
    binary = os.path.join(CDIR, 'capon_caller')
    cmd = ['gcc', '-O1', '-Wall', '-Wextra', '-Werror', '-std=c11', '-pthread', '-I', os.path.join(ROOT, 'include'),
           os.path.join(CDIR, 'capon_caller.c'), '-o', binary, '-L', LIBDIR, '-lnbls_hip', '-lm',
           '-Wl,-rpath,$ORIGIN/../../narrow_band_least_squares_amd/csrc', '-Wl,-rpath-link,/opt/rocm/lib']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return binary


def test_plain_c_caller_compiles_and_links():
    binary = build_capon_caller()
    out = subprocess.run(['nm', '-u', binary], capture_output=True, text=True).stdout
    assert set(SYMBOLS) | {'nbls_plan', 'nbls_execute'} <= set(re.findall(r'\b(nbls_[a-z0-9_]+)', out))
