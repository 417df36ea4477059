"""What of the slowness-grid search (``nbls_set_beam_grid``) a box without a GPU can check: the new
Python names and their argument checks, ``planner.slowness_grid``, the five new symbols in the header, the ctypes binding
and the built library, the defining lines shared by DESIGN.md and the header, and a plain-C caller that compiles and
links."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, 'tests', 'c_caller')
LIBDIR = os.path.join(ROOT, 'narrow_band_least_squares_amd', 'csrc')
SYMBOLS = ('nbls_set_beam_grid', 'nbls_fetch_beam_grid', 'nbls_fetch_beam_grid_map', 'nbls_fetch_beam_grid_delays',
           'nbls_beam_grid_lds_bytes')


def test_python_names_and_signatures():
    import narrow_band_least_squares_amd as pkg
    from narrow_band_least_squares_amd import engine, planner, _hip
    for name in ('ltsva_grid', 'narrow_band_least_squares_grid'):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    assert list(inspect.signature(pkg.ltsva_grid).parameters) == ['st', 'lat_list', 'lon_list', 'window_length', 'window_overlap',
                                                                   'slowness_grid', 'alpha', 'rij', 'grid_map']
    sig = inspect.signature(pkg.ltsva_grid).parameters
    assert sig['alpha'].default == 1.0 and sig['rij'].default is None and sig['grid_map'].default is False
    ref_args = list(inspect.signature(pkg.narrow_band_least_squares).parameters)
    sig = inspect.signature(pkg.narrow_band_least_squares_grid)
    assert list(sig.parameters) == ref_args + ['slowness_grid', 'grid_map']
    assert sig.parameters['slowness_grid'].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters['slowness_grid'].default is inspect.Parameter.empty and sig.parameters['grid_map'].default is False
    batch = inspect.signature(pkg.ltsva_batch).parameters
    assert list(batch)[-1] == 'slowness_grid' and batch['slowness_grid'].default is None
    # the reference-named functions and the earlier extensions keep their signatures
    assert list(inspect.signature(pkg.ltsva).parameters) == ['st', 'lat_list', 'lon_list', 'window_length', 'window_overlap',
                                                              'alpha', 'plot_array_coordinates', 'rij']
    for f in (pkg.ltsva, pkg.ltsva_beam, pkg.ltsva_subsample, pkg.ltsva_bounded, pkg.ltsva_multi, pkg.narrow_band_least_squares,
              pkg.narrow_band_least_squares_beam, engine.process_multi):
        assert 'slowness_grid' not in inspect.signature(f).parameters
    for f in (engine.process, engine.process_batch):
        p = inspect.signature(f).parameters
        assert p['slowness_grid'].default is None and p['want_grid_map'].default is False
    assert inspect.signature(engine.process_segmented).parameters['slowness_grid'].default is None
    p = inspect.signature(engine.launch).parameters
    assert p['beam_grid'].default is None and p['beam_grid_map'].default is False
    for name in ('set_beam_grid', 'fetch_beam_grid', 'fetch_beam_grid_map', 'fetch_beam_grid_delays'):
        assert callable(getattr(_hip.Handle, name))
    assert callable(planner.slowness_grid) and callable(planner.check_slowness_grid)
    # under the reference's module names the new functions are attributes of the same modules
    pkg.install_as_reference_modules()
    import lts_array
    import narrow_band_least_squares as nbls_mod
    assert lts_array.ltsva_grid is pkg.ltsva_grid and nbls_mod.narrow_band_least_squares_grid is pkg.narrow_band_least_squares_grid


def test_slowness_grid_of_the_counts():
    from narrow_band_least_squares_amd import planner
    g = planner.slowness_grid(4.0, 41)
    assert g.shape == (1257, 2) and g.dtype == np.float64 and g.flags.c_contiguous
    ax = np.linspace(-4.0, 4.0, 41)
    a, b = np.meshgrid(ax, ax, indexing='ij')
    full = np.stack([a.ravel(), b.ravel()], axis=1)
    np.testing.assert_array_equal(g, full[np.hypot(full[:, 0], full[:, 1]) <= 4.0])
    assert np.any(np.all(g == 0.0, axis=1)) and np.all(np.hypot(g[:, 0], g[:, 1]) <= 4.0)
    assert planner.slowness_grid(1.0, 1).tolist() == [[0.0, 0.0]]
    for bad in ((4.0, 40), (4.0, 0), (4.0, 2.5), (4.0, True), (0.0, 5), (-1.0, 5), (np.inf, 5), (np.nan, 5)):
        with pytest.raises(ValueError):
            planner.slowness_grid(*bad)
    assert planner.check_slowness_grid([[1, 2], [3, 4]]).dtype == np.float64
    for bad in (np.zeros((0, 2)), np.zeros(4), np.zeros((3, 3)), np.zeros((65537, 2)), [[0.0, np.nan]], [[np.inf, 0.0]],
                [[1j, 0.0]], [['a', 'b']], None, np.zeros((2, 2, 2)), np.zeros((2, 2), dtype=bool)):
        with pytest.raises(ValueError):
            planner.check_slowness_grid(bad)
    assert planner.check_slowness_grid(np.zeros((65536, 2))).shape == (65536, 2)


def _stream(nchans, npts=600, fs=20.0):
    from narrow_band_least_squares_amd import synthetic
    return synthetic.make_stream(np.random.default_rng(4).standard_normal((nchans, npts)), fs)


def test_bad_arguments_raise_before_any_gpu_work(monkeypatch):
    import narrow_band_least_squares_amd as pkg
    from narrow_band_least_squares_amd import engine

    def no_gpu(*a, **k):
        raise AssertionError('the GPU was reached')
    monkeypatch.setattr(engine, 'get_handle', no_gpu)
    monkeypatch.setattr(engine, 'start_upload', no_gpu)
    rij = np.array([[0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 1.0, 1.0]])
    grid = np.zeros((3, 2))
    for bad in (np.zeros((3, 3)), np.zeros((0, 2)), [[0.0, np.nan]], [[1j, 0.0]], np.zeros((65537, 2)), None):
        with pytest.raises(ValueError):
            pkg.ltsva_grid(_stream(4), None, None, 10.0, 0.5, bad, rij=rij)
        if bad is not None:
            with pytest.raises(ValueError):
                pkg.ltsva_batch([_stream(4), _stream(4)], None, None, 10.0, 0.5, rij=rij, slowness_grid=bad)
            with pytest.raises(ValueError):
                engine.process(list(np.zeros((4, 600))), 20.0, 0.0, rij, [(None, None)], [10.0], 0.5, 1.0, prefiltered=True,
                               slowness_grid=bad)
            with pytest.raises(ValueError):
                engine.process_batch([list(np.zeros((4, 600)))] * 2, 20.0, [0.0, 0.0], rij, [(None, None)], [10.0], 0.5, 1.0,
                                     prefiltered=True, slowness_grid=bad)
    with pytest.raises(ValueError):
        pkg.ltsva_grid(_stream(4), None, None, 10.0, 0.5, grid, rij=rij, grid_map=1)
    with pytest.raises(ValueError):
        pkg.ltsva_grid(_stream(4), None, None, 10.0, 0.5, grid, alpha=0.3, rij=rij)
    with pytest.raises(ValueError):
        pkg.ltsva_grid(_stream(2), None, None, 10.0, 0.5, grid, rij=rij[:, :2])
    with pytest.raises(ValueError):
        pkg.ltsva_grid(_stream(3), None, None, 10.0, 0.5, grid, alpha=0.75, rij=rij[:, :3])        # LTS needs four elements
    fr = np.logspace(-1, 0.5, 16)
    args = ([10.0, 10.0], 0.5, 1.0, _stream(4), None, None, 2, np.zeros(16), np.zeros(16), np.array([0.5, 1.0, 2.0]), 'log', fr,
            'butter', 2, 0.01)
    with pytest.raises(TypeError):                                 # the grid is a required keyword
        pkg.narrow_band_least_squares_grid(*args, rij=rij)
    with pytest.raises(ValueError):
        pkg.narrow_band_least_squares_grid(*args, rij=rij, slowness_grid=np.zeros((3, 3)))
    with pytest.raises(ValueError):
        pkg.narrow_band_least_squares_grid(*args, rij=rij, slowness_grid=grid, grid_map='yes')
    with pytest.raises(ValueError):
        pkg.narrow_band_least_squares_grid(*(args[:2] + (0.2,) + args[3:]), rij=rij, slowness_grid=grid)
    with pytest.raises(ValueError):                                # response rows of the wrong length
        pkg.narrow_band_least_squares_grid(*(args[:7] + (np.zeros(8), np.zeros(8)) + args[9:]), rij=rij, slowness_grid=grid)
    # the time-segmented fallback keeps the band on the host: it names the limit instead of computing on the host
    with pytest.raises(ValueError, match='time-segmented'):
        engine.process_segmented(list(np.zeros((4, 600))), 20.0, 0.0, rij, [(0.5, 1.0)], [10.0], 0.5, 1.0, 'butter', 2, 0.01,
                                 None, slowness_grid=grid)


def test_grid_slowness_as_the_solve_reports_one():
    from narrow_band_least_squares_amd.lts_array import grid_slowness
    grid = np.array([[0.0, 0.0], [3.0, 4.0], [-2.0, 0.0], [0.0, -0.5]])
    vel, baz = grid_slowness(grid, np.array([-1, 0, 1, 2, 3]))
    assert np.isnan(vel[0]) and np.isnan(baz[0])
    assert vel[1] == np.inf and vel[2] == 0.2 and vel[3] == 0.5 and vel[4] == 2.0
    assert baz[2] == pytest.approx(np.degrees(np.arctan2(3.0, 4.0)), abs=1e-12)
    assert baz[3] == pytest.approx(270.0, abs=1e-12) and baz[4] == pytest.approx(180.0, abs=1e-12)
    assert np.all((baz[1:] >= 0.0) & (baz[1:] < 360.0))


def test_header_binding_and_library_carry_the_symbols():
    from narrow_band_least_squares_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    for s in SYMBOLS:
        assert re.search(r'^int %s\(' % s, header, re.M), s
        assert s in _hip.EXPORTS
    assert re.search(r'^#define NBLS_BEAM_GRID_MAX %d$' % _hip.BEAM_GRID_MAX, header, re.M)
    assert re.search(r'^#define NBLS_BEAM_GRID_WAVES %d$' % _hip.BEAM_GRID_WAVES, header, re.M)
    lib = _hip.load_library()
    for s in SYMBOLS:
        assert getattr(lib, s).argtypes is not None, s
    out = subprocess.run(['nm', '-D', '--defined-only', os.path.join(LIBDIR, 'libnbls_hip.so')], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    defined = set(re.findall(r' T (nbls_[a-z0-9_]+)', out.stdout))
    assert set(SYMBOLS) <= defined
    # the kernel is in the code object of the library (a missing kernel is an error, not a host loop)
    blob = open(os.path.join(LIBDIR, 'libnbls_hip.so'), 'rb').read()
    assert b'beam_grid_kernel' in blob


def test_form_function_is_pure_and_follows_its_rule():
    from narrow_band_least_squares_amd import _hip
    lib = _hip.load_library()
    cap = 156 * 1024
    for nelem, W, halo in ((3, 16, 0), (8, 1200, 128), (8, 1200, 19), (9, 257, 40), (32, 600, 12), (8, 1200, 650), (8, 1200, 700),
                           (4, 65, 2500)):
        need = nelem * (W + 2 * halo) * 8
        assert lib.nbls_beam_grid_lds_bytes(nelem, W, halo) == (need if need <= cap else 0), (nelem, W, halo)
    assert lib.nbls_beam_grid_lds_bytes(8, 1200, 128) == 93184                # the 1 km array of the counts: staged
    for bad in ((0, 16, 0), (3, 0, 0), (3, 16, -1)):
        assert lib.nbls_beam_grid_lds_bytes(*bad) == _hip.NBLS_ERR_ARG


def test_design_and_header_state_the_contract_alike():
    """DESIGN.md section 15 and include/nbls.h carry the same defining lines."""
    header = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert re.search(r'^## 15\.', design, re.M)
    design = design[design.index('## 15.'):]
    flat = lambda s: re.sub(r'[\s*`]+', ' ', s)
    for line in ('d[g][0] = 0, d[g][i] = rint(fs (xij[i-1][0] s_g0 + xij[i-1][1] s_g1))',
                 'x_i[t] = filt[row of element i][s0 + t + d[g][i]]', 'D = N S_t - S_b', 'F(g) = (N - 1) S_b / D',
                 'F(g) = +inf if D <= 0 and S_b > 0', 'F(g) = NaN if S_t == 0 or a NaN sample was read', 'P(g) = S_b / (N^2 W)',
                 'F descending (+inf first), g ascending', '-1 if no g has a non-NaN F', 'H = max |d[g][i]|'):
        assert line in flat(header) and line in flat(design), line


def build_grid_caller():
    binary = os.path.join(CDIR, 'grid_caller')
    cmd = ['gcc', '-O1', '-Wall', '-Wextra', '-Werror', '-std=c11', '-pthread', '-I', os.path.join(ROOT, 'include'),
           os.path.join(CDIR, 'grid_caller.c'), '-o', binary, '-L', LIBDIR, '-lnbls_hip', '-lm',
           '-Wl,-rpath,$ORIGIN/../../narrow_band_least_squares_amd/csrc', '-Wl,-rpath-link,/opt/rocm/lib']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return binary


def test_plain_c_caller_compiles_and_links():
    binary = build_grid_caller()
    out = subprocess.run(['nm', '-u', binary], capture_output=True, text=True).stdout
    assert set(SYMBOLS) | {'nbls_plan', 'nbls_execute'} <= set(re.findall(r'\b(nbls_[a-z0-9_]+)', out))
