"""What of the bounded lag search (``nbls_set_lag_limits``) a box without a GPU can check: the limit
table of ``planner.lag_limits``, the new Python names, their signatures and argument checks, the new symbols in the header,
the ctypes binding and the built library, the two kernels in the library's code object, and the form selector."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import bounded_truth as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, 'narrow_band_least_squares_amd', 'csrc')
SYMBOLS = ('nbls_set_lag_limits', 'nbls_lag_limit_form')


def test_lag_limits_values():
    from narrow_band_least_squares_amd import planner, synthetic
    xij = np.array([[0.3, 0.4], [0.0, 0.0], [1.0, 0.0], [0.1, 0.0], [-0.06, 0.08]])
    lim = planner.lag_limits(xij, 40.0, 0.25)
    assert lim.dtype == np.int32
    np.testing.assert_array_equal(lim, [81, 1, 161, 17, 17])          # ceil(fs |xij| / v) + 1
    np.testing.assert_array_equal(lim, bt.limits(xij, 40.0, 0.25))
    # cfg-3's geometry at v_min = 0.25 km/s, and the same coordinates scaled by 0.15
    rij = synthetic.array_geometry(8, 1.0)
    x8 = planner.co_array(rij)[0]
    for scale, exp in ((1.0, (23, 94, 250)), (0.15, (5, 15, 39))):
        lim = planner.lag_limits(x8 * scale, 40.0, 0.25)
        assert (lim.min(), int(np.median(lim)), lim.max()) == exp
    assert planner.lag_limits(xij, 40.0, 1e-12).max() == 2 ** 31 - 1   # (clipped to what the C ABI carries)
    for bad in (0, 0.0, -1.0, np.nan, np.inf, True, np.bool_(True), '0.3', None, [0.3]):
        with pytest.raises(ValueError):
            planner.lag_limits(xij, 40.0, bad)
    assert planner.check_min_velocity(np.float32(0.5)) == 0.5 and planner.check_min_velocity(1) == 1.0


def test_python_names_and_signatures():
    import narrow_band_least_squares_amd as pkg
    from narrow_band_least_squares_amd import engine, _hip
    for name in ('ltsva_bounded', 'narrow_band_least_squares_bounded'):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    assert list(inspect.signature(pkg.ltsva_bounded).parameters) == ['st', 'lat_list', 'lon_list', 'window_length',
                                                                      'window_overlap', 'min_velocity', 'alpha', 'rij']
    assert inspect.signature(pkg.ltsva_bounded).parameters['alpha'].default == 1.0
    ref_args = list(inspect.signature(pkg.narrow_band_least_squares).parameters)
    sig = inspect.signature(pkg.narrow_band_least_squares_bounded)
    assert list(sig.parameters) == ref_args + ['min_velocity']
    assert sig.parameters['min_velocity'].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig.parameters['min_velocity'].default is inspect.Parameter.empty
    for f in (pkg.ltsva_batch, pkg.ltsva_multi):
        assert inspect.signature(f).parameters['min_velocity'].default is None
    # the reference-named functions keep their signatures; the narrow-band batch / multi / parallel forms get no bounded form
    assert list(inspect.signature(pkg.ltsva).parameters) == ['st', 'lat_list', 'lon_list', 'window_length', 'window_overlap',
                                                              'alpha', 'plot_array_coordinates', 'rij']
    assert 'rij' == ref_args[-1]
    for f in (pkg.narrow_band_least_squares, pkg.narrow_band_least_squares_parallel, pkg.narrow_band_least_squares_batch,
              pkg.narrow_band_least_squares_multi, pkg.ltsva_beam, pkg.ltsva_subsample):
        assert 'min_velocity' not in inspect.signature(f).parameters
    for f in (engine.process, engine.process_batch, engine.process_multi, engine.process_segmented):
        assert inspect.signature(f).parameters['min_velocity'].default is None
    assert inspect.signature(engine.launch).parameters['lag_limits'].default is None
    assert inspect.signature(_hip.Handle.set_lag_limits).parameters['max_lag'].default is None
    pkg.install_as_reference_modules()
    import lts_array
    import narrow_band_least_squares as nbls_mod
    assert lts_array.ltsva_bounded is pkg.ltsva_bounded
    assert nbls_mod.narrow_band_least_squares_bounded is pkg.narrow_band_least_squares_bounded
    assert lts_array.ltsva is pkg.ltsva


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
    for bad in (0.0, -0.25, np.nan, np.inf, True, '0.25', None):
        with pytest.raises(ValueError):
            pkg.ltsva_bounded(_stream(4), None, None, 10.0, 0.5, bad, rij=rij)
    for bad in (0.0, -0.25, np.nan, True, '0.25'):
        with pytest.raises(ValueError):
            pkg.ltsva_batch([_stream(4), _stream(4)], None, None, 10.0, 0.5, rij=rij, min_velocity=bad)
        with pytest.raises(ValueError):
            pkg.ltsva_multi(_stream(4), None, None, 10.0, 0.5, [1.0, (1.0, (0,))], rij=rij, min_velocity=bad)
        with pytest.raises(ValueError):
            engine.process(list(np.zeros((4, 600))), 20.0, 0.0, rij, [(None, None)], [10.0], 0.5, 1.0, prefiltered=True,
                           min_velocity=bad)
    with pytest.raises(ValueError):
        pkg.ltsva_bounded(_stream(2), None, None, 10.0, 0.5, 0.25, rij=rij[:, :2])
    with pytest.raises(ValueError):
        pkg.ltsva_bounded(_stream(3), None, None, 10.0, 0.5, 0.25, alpha=0.75, rij=rij[:, :3])   # LTS needs four elements
    fr = np.logspace(-1, 0.5, 16)
    args = ([10.0, 10.0], 0.5, 1.0, _stream(4), None, None, 2, np.zeros(16), np.zeros(16), np.array([0.5, 1.0, 2.0]), 'log', fr,
            'butter', 2, 0.01)
    with pytest.raises(TypeError):                                 # min_velocity is required, by keyword
        pkg.narrow_band_least_squares_bounded(*args, rij=rij)
    for bad in (0.0, np.inf, False):
        with pytest.raises(ValueError):
            pkg.narrow_band_least_squares_bounded(*args, rij=rij, min_velocity=bad)
    with pytest.raises(ValueError):
        pkg.narrow_band_least_squares_bounded(*(args[:2] + (0.2,) + args[3:]), rij=rij, min_velocity=0.25)


def test_time_segmented_path_names_the_restriction(monkeypatch):
    from narrow_band_least_squares_amd import engine
    monkeypatch.setattr(engine, 'get_handle', lambda *a, **k: pytest.fail('the GPU was reached'))
    rij = np.array([[0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 1.0, 1.0]])
    with pytest.raises(ValueError, match='time-segmented') as err:
        engine.process_segmented(list(np.zeros((4, 600))), 20.0, 0.0, rij, [(0.5, 1.0)], [10.0], 0.5, 1.0, 'butter', 2, 0.01,
                                 None, min_velocity=0.25)
    assert 'min_velocity' in str(err.value)


def test_header_binding_and_library_carry_the_symbols():
    from narrow_band_least_squares_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    assert re.search(r'^int nbls_set_lag_limits\(nbls_handle\* h, const int32_t\* max_lag, int32_t npairs\);', header, re.M)
    assert re.search(r'^int nbls_lag_limit_form\(int32_t nelem, int32_t W, int32_t min_limit\);', header, re.M)
    lib = _hip.load_library()
    for s in SYMBOLS:
        assert s in _hip.EXPORTS and getattr(lib, s).argtypes is not None, s
    out = subprocess.run(['nm', '-D', '--defined-only', os.path.join(LIBDIR, 'libnbls_hip.so')], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert set(SYMBOLS) <= set(re.findall(r' T (nbls_[a-z0-9_]+)', out.stdout))
    # the kernels are in the code object of the library (a missing kernel is an error, not a host loop)
    blob = open(os.path.join(LIBDIR, 'libnbls_hip.so'), 'rb').read()
    assert b'xcorr_bounded_mfma_kernel' in blob and b'xcorr_bounded_simple_kernel' in blob
    assert 'xcorr_bounded.o' in open(os.path.join(LIBDIR, 'Makefile')).read()


def test_form_selector():
    """``nbls_lag_limit_form``: 0 where the smallest limit reaches W-1; else 1 for 3..16 elements whose zero-padded windows
    fit a CU's LDS — exactly where the route function takes NBLS_ROUTE_MFMA for a forced f64-MFMA pass —, else 2."""
    from narrow_band_least_squares_amd import _hip
    for N in range(3, 33):
        for W in (2, 16, 64, 65, 130, 1200):
            assert _hip.lag_limit_form(N, W, W - 1) == 0 and _hip.lag_limit_form(N, W, 10 ** 6) == 0
            if W > 2:
                assert _hip.lag_limit_form(N, W, W - 2) == (1 if N <= 16 else 2)
                assert _hip.lag_limit_form(N, W, 0) == (1 if N <= 16 else 2)
    # the LDS-fit boundary of every element count: the last window length the matrix-core form takes
    for N in (3, 4, 8, 9, 16):
        t = _hip.route_table(N, 1000, 7000, xcorr_impl=2)
        fits = t['correlator'] == _hip.ROUTE_MFMA
        last = 1000 + int(np.flatnonzero(fits)[-1])
        assert fits[:last - 1000 + 1].all() and not fits[last - 1000 + 1:].any()
        S = 16 // (N - 1)
        cs = lambda W: 16 * (S - 1) + W + 32 + (2 - (16 * (S - 1) + W + 32)) % 32
        lds = lambda W: (N * cs(W) + 17 * N) * 8 + 64 * N
        assert lds(last) <= 160 * 1024 < lds(last + 1)
        assert _hip.lag_limit_form(N, last, 5) == 1 and _hip.lag_limit_form(N, last + 1, 5) == 2
        assert _hip.lag_limit_form(N, last + 1, last) == 0
    assert _hip.lag_limit_form(8, 1200, 39) == 1 and _hip.lag_limit_form(17, 1200, 39) == 2
    for bad in ((2, 16, 3), (33, 16, 3), (8, 1, 0), (8, 16, -1)):
        with pytest.raises(ValueError):
            _hip.lag_limit_form(*bad)


def test_design_and_header_state_the_contract_alike():
    """DESIGN.md section 14 and include/nbls.h carry the same defining lines."""
    header = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert re.search(r'^## 14\.', design, re.M)
    flat = lambda s: re.sub(r'[\s*`]+', ' ', s)
    for line in ('lag = L - np.argmax(cij[W-1-L : W+L])', 'cij = np.correlate(a, b, \'full\') / sqrt(sum a^2 sum b^2)',
                 'cmax = R(lag) / sqrt(sum a^2 sum b^2)', 'lag = min(the plain pass\'s lag, L)'):
        assert line in flat(header) and line in flat(design), line
