"""What of the seeded lag search (``nbls_set_lag_seed``) a box without a GPU can check: the
half-widths of ``planner.seed_halfwidths``, the new Python names, their signatures and argument checks, the new symbols in
the header, the ctypes binding and the built library, the two kernels in the library's code object, the form selector and
the error returns of the setter that need no device."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, 'narrow_band_least_squares_amd', 'csrc')
SYMBOLS = ('nbls_set_lag_seed', 'nbls_lag_seed_form')


def test_seed_halfwidths_values():
    from narrow_band_least_squares_amd import planner
    K = planner.seed_halfwidths([1.1, 1.0, 2.0, 0.5, 19.9, 20.0, 100.0], 40.0)
    assert K.dtype == np.int32
    np.testing.assert_array_equal(K, [18, 20, 10, 40, 1, 1, 1])            # max(1, floor(0.5 fs / fmax))
    np.testing.assert_array_equal(planner.seed_halfwidths([1.1, 2.0], 40.0, 0.25), [9, 5])
    np.testing.assert_array_equal(planner.seed_halfwidths([1.1], 40.0, 1.0), [36])
    np.testing.assert_array_equal(planner.seed_halfwidths(np.array([1.1]), np.float32(40.0), 0.1), [3])
    np.testing.assert_array_equal(planner.seed_halfwidths([1.1], 40.0, 0.125), [4])       # (K = 4 / 9 / 18: 1/8, 1/4, 1/2 period)
    assert planner.seed_halfwidths([1e-12], 40.0).tolist() == [2 ** 31 - 1]   # (clipped to what the C ABI carries)
    for bad in ([], [0.0], [-1.0], [np.nan], [np.inf], ['1.0'], [[1.0]], None, 1.0):
        with pytest.raises(ValueError):
            planner.seed_halfwidths(bad, 40.0)
    for bad in (0, -40.0, np.nan, np.inf, True, '40', None):
        with pytest.raises(ValueError):
            planner.seed_halfwidths([1.0], bad)
    for bad in (0, 0.0, -0.5, 1.5, np.nan, True, '0.5', None):
        with pytest.raises(ValueError):
            planner.seed_halfwidths([1.0], 40.0, bad)


def test_check_seed_halfwidths():
    from narrow_band_least_squares_amd import planner
    k = planner.check_seed_halfwidths(18, 3)
    assert k.dtype == np.int32 and k.tolist() == [18, 18, 18] and k.flags['C_CONTIGUOUS']
    assert planner.check_seed_halfwidths([0, 4, 2 ** 31 - 1], 3).tolist() == [0, 4, 2 ** 31 - 1]
    assert planner.check_seed_halfwidths(np.int64(5), 1).tolist() == [5]
    assert planner.check_seed_halfwidths(planner.seed_halfwidths([1.1, 2.0], 40.0), 2).tolist() == [18, 10]
    for bad in (-1, [1, -1], 2 ** 31, 1.5, [1.0, 2.0], '3', None, [[1, 2]], [1, 2, 3], [], np.nan):
        with pytest.raises(ValueError):
            planner.check_seed_halfwidths(bad, 2)


def test_python_names_and_signatures():
    import narrow_band_least_squares_amd as pkg
    from narrow_band_least_squares_amd import engine, _hip
    for name in ('ltsva_seeded', 'narrow_band_least_squares_seeded'):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    sig = inspect.signature(pkg.ltsva_seeded)
    assert list(sig.parameters) == ['st', 'lat_list', 'lon_list', 'window_length', 'window_overlap', 'slowness_grid',
                                    'halfwidth', 'alpha', 'rij', 'grid_map']
    assert (sig.parameters['alpha'].default, sig.parameters['rij'].default, sig.parameters['grid_map'].default) == (1.0, None, False)
    ref_args = list(inspect.signature(pkg.narrow_band_least_squares).parameters)
    sig = inspect.signature(pkg.narrow_band_least_squares_seeded)
    assert list(sig.parameters) == ref_args + ['slowness_grid', 'period_fraction', 'grid_map']
    for name in ('slowness_grid', 'period_fraction', 'grid_map'):
        assert sig.parameters[name].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters['slowness_grid'].default is inspect.Parameter.empty
    assert sig.parameters['period_fraction'].default == 0.5 and sig.parameters['grid_map'].default is False
    # existing signatures do not change; the forms out of scope get no keyword
    assert list(inspect.signature(pkg.ltsva_grid).parameters) == ['st', 'lat_list', 'lon_list', 'window_length', 'window_overlap',
                                                                   'slowness_grid', 'alpha', 'rij', 'grid_map']
    assert list(inspect.signature(pkg.narrow_band_least_squares_grid).parameters) == ref_args + ['slowness_grid', 'grid_map']
    for f in (pkg.narrow_band_least_squares, pkg.narrow_band_least_squares_parallel, pkg.narrow_band_least_squares_batch,
              pkg.narrow_band_least_squares_multi, pkg.ltsva, pkg.ltsva_batch, pkg.ltsva_multi, pkg.ltsva_grid, pkg.ltsva_bounded):
        assert not {'halfwidth', 'seed_halfwidths', 'period_fraction'} & set(inspect.signature(f).parameters)
    for f in (engine.process, engine.process_batch, engine.process_segmented):
        assert inspect.signature(f).parameters['seed_halfwidths'].default is None
    assert inspect.signature(engine.launch).parameters['lag_seed'].default is None
    assert inspect.signature(_hip.Handle.set_lag_seed).parameters['halfwidth'].default is None
    pkg.install_as_reference_modules()
    import lts_array
    import narrow_band_least_squares as nbls_mod
    assert lts_array.ltsva_seeded is pkg.ltsva_seeded
    assert nbls_mod.narrow_band_least_squares_seeded is pkg.narrow_band_least_squares_seeded


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
    grid = np.array([[0.0, 0.0], [1.0, 0.0]])
    for bad in (-1, 1.5, '4', None, [1, 2], 2 ** 31, np.nan):
        with pytest.raises(ValueError):
            pkg.ltsva_seeded(_stream(4), None, None, 10.0, 0.5, grid, bad, rij=rij)
    for bad_grid in (None, [[0.0, np.nan]], np.zeros((3, 3)), 'grid'):
        with pytest.raises(ValueError):
            pkg.ltsva_seeded(_stream(4), None, None, 10.0, 0.5, bad_grid, 4, rij=rij)
    with pytest.raises(ValueError):
        pkg.ltsva_seeded(_stream(4), None, None, 10.0, 0.5, grid, 4, rij=rij, grid_map=1)
    with pytest.raises(ValueError):
        pkg.ltsva_seeded(_stream(2), None, None, 10.0, 0.5, grid, 4, rij=rij[:, :2])
    with pytest.raises(ValueError):
        pkg.ltsva_seeded(_stream(3), None, None, 10.0, 0.5, grid, 4, alpha=0.75, rij=rij[:, :3])   # LTS needs four elements
    data = list(np.zeros((4, 600)))
    for kw in (dict(seed_halfwidths=4),                                          # no grid
               dict(seed_halfwidths=4, slowness_grid=grid, min_velocity=0.25),   # one restriction at a time
               dict(seed_halfwidths=-1, slowness_grid=grid), dict(seed_halfwidths=[1, 2], slowness_grid=grid),
               dict(seed_halfwidths=0.5, slowness_grid=grid)):
        with pytest.raises(ValueError):
            engine.process(data, 20.0, 0.0, rij, [(None, None)], [10.0], 0.5, 1.0, prefiltered=True, **kw)
        with pytest.raises(ValueError):
            engine.process_batch([data, data], 20.0, [0.0, 0.0], rij, [(None, None)], [10.0], 0.5, 1.0, prefiltered=True, **kw)
    fr = np.logspace(-1, 0.5, 16)
    args = ([10.0, 10.0], 0.5, 1.0, _stream(4), None, None, 2, np.zeros(16), np.zeros(16), np.array([0.5, 1.0, 2.0]), 'log', fr,
            'butter', 2, 0.01)
    with pytest.raises(TypeError):                                 # slowness_grid is required, by keyword
        pkg.narrow_band_least_squares_seeded(*args, rij=rij)
    for bad in (0.0, -0.5, 1.5, np.nan, True, '0.5'):
        with pytest.raises(ValueError):
            pkg.narrow_band_least_squares_seeded(*args, rij=rij, slowness_grid=grid, period_fraction=bad)
    with pytest.raises(ValueError):
        pkg.narrow_band_least_squares_seeded(*args, rij=rij, slowness_grid=[[0.0, np.inf]])
    with pytest.raises(ValueError):
        pkg.narrow_band_least_squares_seeded(*args, rij=rij, slowness_grid=grid, grid_map='yes')
    with pytest.raises(ValueError):
        pkg.narrow_band_least_squares_seeded(*(args[:2] + (0.2,) + args[3:]), rij=rij, slowness_grid=grid)


def test_time_segmented_path_names_the_restriction(monkeypatch):
    from narrow_band_least_squares_amd import engine
    monkeypatch.setattr(engine, 'get_handle', lambda *a, **k: pytest.fail('the GPU was reached'))
    rij = np.array([[0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 1.0, 1.0]])
    with pytest.raises(ValueError, match='time-segmented') as err:
        engine.process_segmented(list(np.zeros((4, 600))), 20.0, 0.0, rij, [(0.5, 1.0)], [10.0], 0.5, 1.0, 'butter', 2, 0.01,
                                 None, seed_halfwidths=np.array([4], dtype=np.int32))
    assert 'seed_halfwidths' in str(err.value)


def test_header_binding_and_library_carry_the_symbols():
    from narrow_band_least_squares_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    assert re.search(r'^int nbls_set_lag_seed\(nbls_handle\* h, const int32_t\* halfwidth, int32_t nbands\);', header, re.M)
    assert re.search(r'^int nbls_lag_seed_form\(int32_t nelem, int32_t W, int32_t max_halfwidth, int32_t halo\);', header, re.M)
    lib = _hip.load_library()
    for s in SYMBOLS:
        assert s in _hip.EXPORTS and getattr(lib, s).argtypes is not None, s
    out = subprocess.run(['nm', '-D', '--defined-only', os.path.join(LIBDIR, 'libnbls_hip.so')], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert set(SYMBOLS) <= set(re.findall(r' T (nbls_[a-z0-9_]+)', out.stdout))
    # the kernels are in the code object of the library (a missing kernel is an error, not a host loop)
    blob = open(os.path.join(LIBDIR, 'libnbls_hip.so'), 'rb').read()
    assert b'xcorr_seeded_staged_kernel' in blob and b'xcorr_seeded_simple_kernel' in blob
    mk = open(os.path.join(LIBDIR, 'Makefile')).read()
    assert 'xcorr_seeded.o' in mk and mk.count('xcorr_seeded.hip') >= 2        # OBJS, the dependency line and DEVSRC


def test_setter_error_returns_that_need_no_device():
    """A NULL handle is NBLS_ERR_ARG whatever the table is (the checks of the table itself need a handle, so a device:
    tests/test_gpu_seeded.py)."""
    from narrow_band_least_squares_amd import _hip
    lib = _hip.load_library()
    t = (ctypes.c_int32 * 2)(4, 4)
    assert lib.nbls_set_lag_seed(None, t, 2) == _hip.NBLS_ERR_ARG
    assert lib.nbls_set_lag_seed(None, None, 0) == _hip.NBLS_ERR_ARG


def _last_fit(N):
    """The largest W whose N windows and N sums of squares, N (W + 1) doubles, fit 156 KiB."""
    return (156 * 1024 // 8) // N - 1


@pytest.mark.parametrize('N', [3, 8, 16, 17, 32])
def test_form_selector(N):
    """``nbls_lag_seed_form``: 1 or 2 only, never 0; monotone in W (once the general form, always the general form); 1 for
    3..16 elements up to the LDS fit; the half-width and the halo do not enter."""
    from narrow_band_least_squares_amd import _hip
    lib = _hip.load_library()
    top = 7000
    forms = np.array([lib.nbls_lag_seed_form(N, W, 18, 128) for W in range(2, top + 1)])
    assert set(forms.tolist()) <= {1, 2}
    assert np.all(np.diff(forms) >= 0)
    if N > 16:
        assert np.all(forms == 2)
    else:
        last = _last_fit(N)
        assert N * (last + 1) * 8 <= 156 * 1024 < N * (last + 2) * 8
        if last <= top:
            assert forms[last - 2] == 1 and forms[last - 1] == 2
        else:
            assert np.all(forms == 1)
        assert _hip.lag_seed_form(N, last) == 1 and _hip.lag_seed_form(N, last + 1) == 2
    for W in (2, 65, 130, 1200):
        assert len({_hip.lag_seed_form(N, W, K, H) for K in (0, 18, 10 ** 6, 2 ** 31 - 1) for H in (0, 7, 2 ** 30)}) == 1


def test_form_selector_edges():
    from narrow_band_least_squares_amd import _hip
    lib = _hip.load_library()
    assert _hip.lag_seed_form(8, 1200, 18, 128) == 1 and _hip.lag_seed_form(17, 1200, 18, 128) == 2
    assert (_hip.lag_seed_form(3, 2), _hip.lag_seed_form(32, 2), _hip.lag_seed_form(16, 2)) == (1, 2, 1)
    for bad in ((2, 16, 3, 0), (33, 16, 3, 0), (0, 16, 3, 0), (8, 1, 0, 0), (8, 0, 0, 0), (8, 16, -1, 0), (8, 16, 0, -1)):
        assert lib.nbls_lag_seed_form(*bad) == _hip.NBLS_ERR_ARG
        with pytest.raises(ValueError):
            _hip.lag_seed_form(*bad)


def test_design_and_header_state_the_contract_alike():
    """DESIGN.md section 16 and include/nbls.h carry the same defining lines."""
    header = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert re.search(r'^## 16\.', design, re.M)
    flat = lambda s: re.sub(r'[\s*`]+', ' ', s)
    for line in ('c = d[g][j] - d[g][i]', 'c\' = min(max(c, -(W-1)), W-1)', 'lo = max(c\' - K, -(W-1)), hi = min(c\' + K, W-1)',
                 'lag = hi - np.argmax(cij[W-1-hi : W-lo])', 'cmax = R(lag) / sqrt(sum a^2 sum b^2)'):
        assert line in flat(header) and line in flat(design), line
