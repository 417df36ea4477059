"""What of the sub-sample lag refinement (``nbls_set_lag_refinement``) a box without a GPU can check:
the new Python names, their signatures and argument checks, the three new symbols in the header, the ctypes binding and
the built library, and the kernel in the library's code object."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, 'narrow_band_least_squares_amd', 'csrc')
SYMBOLS = ('nbls_set_lag_refinement', 'nbls_fetch_lag_fraction', 'nbls_est_fetch_lag_fraction')


def test_python_names_and_signatures():
    import narrow_band_least_squares_amd as pkg
    from narrow_band_least_squares_amd import engine, _hip
    for name in ('ltsva_subsample', 'narrow_band_least_squares_subsample'):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    assert list(inspect.signature(pkg.ltsva_subsample).parameters) == ['st', 'lat_list', 'lon_list', 'window_length',
                                                                        'window_overlap', 'alpha', 'rij']
    assert inspect.signature(pkg.ltsva_subsample).parameters['alpha'].default == 1.0
    ref_args = list(inspect.signature(pkg.narrow_band_least_squares).parameters)
    assert list(inspect.signature(pkg.narrow_band_least_squares_subsample).parameters) == ref_args
    for f in (pkg.ltsva_batch, pkg.ltsva_multi):
        assert inspect.signature(f).parameters['subsample'].default is False
        assert inspect.signature(f).parameters['beam'].default is False
    # the reference-named functions keep their signatures
    assert list(inspect.signature(pkg.ltsva).parameters) == ['st', 'lat_list', 'lon_list', 'window_length', 'window_overlap',
                                                              'alpha', 'plot_array_coordinates', 'rij']
    assert 'rij' == ref_args[-1] and 'subsample' not in ref_args
    for f in (engine.process, engine.process_batch, engine.process_multi, engine.process_segmented):
        assert inspect.signature(f).parameters['want_subsample'].default is False
    assert inspect.signature(engine.launch).parameters['subsample'].default is False
    assert inspect.signature(_hip.Handle.fetch_lag_fraction).parameters['e'].default == 0
    assert hasattr(_hip.Handle, 'set_lag_refinement')
    # under the reference's module names the new functions are attributes of the same modules
    pkg.install_as_reference_modules()
    import lts_array
    import narrow_band_least_squares as nbls_mod
    assert lts_array.ltsva_subsample is pkg.ltsva_subsample
    assert nbls_mod.narrow_band_least_squares_subsample is pkg.narrow_band_least_squares_subsample
    assert lts_array.ltsva is pkg.ltsva


def test_result_record_carries_the_fractions_only_with_the_lags():
    from narrow_band_least_squares_amd import engine
    W, inc, nwin = np.array([65]), np.array([32]), np.array([7])
    assert engine.new_result(4, 1.0, 20.0, W, inc, nwin, 9).lag_frac is None
    assert engine.new_result(4, 1.0, 20.0, W, inc, nwin, 9, want_subsample=True).lag_frac is None
    assert engine.new_result(4, 1.0, 20.0, W, inc, nwin, 9, want_lag=True).lag_frac is None
    res = engine.new_result(4, 1.0, 20.0, W, inc, nwin, 9, want_lag=True, want_subsample=True)
    assert res.lag_frac.shape == res.lag.shape == (1, 9, 6) and res.lag_frac.dtype == np.float64 and not res.lag_frac.any()


def _stream(nchans, npts=600, fs=20.0):
    from narrow_band_least_squares_amd import synthetic
    return synthetic.make_stream(np.random.default_rng(4).standard_normal((nchans, npts)), fs)


def test_bad_arguments_raise_before_any_gpu_work(monkeypatch):
    import narrow_band_least_squares_amd as pkg
    from narrow_band_least_squares_amd import engine

    def no_gpu(*a, **k):
        raise AssertionError('the GPU was reached')
    monkeypatch.setattr(engine, 'get_handle', no_gpu)
    rij = np.array([[0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 1.0, 1.0]])
    with pytest.raises(ValueError):
        pkg.ltsva_subsample(_stream(4), None, None, 10.0, 0.5, alpha=0.3, rij=rij)
    with pytest.raises(ValueError):
        pkg.ltsva_subsample(_stream(2), None, None, 10.0, 0.5, alpha=1.0, rij=rij[:, :2])
    with pytest.raises(ValueError):
        pkg.ltsva_subsample(_stream(3), None, None, 10.0, 0.5, alpha=0.75, rij=rij[:, :3])   # LTS needs four elements
    with pytest.raises(ValueError):
        pkg.ltsva_batch([_stream(4), _stream(4, npts=500)], None, None, 10.0, 0.5, rij=rij, subsample=True)
    with pytest.raises(ValueError):
        pkg.ltsva_batch([_stream(4), _stream(4)], None, None, 10.0, 0.5, rij=rij, subsample='yes')
    with pytest.raises(ValueError):
        pkg.ltsva_multi(_stream(4), None, None, 10.0, 0.5, [1.0, 0.75], rij=rij, subsample=1)
    with pytest.raises(ValueError):
        pkg.ltsva_multi(_stream(4), None, None, 10.0, 0.5, [(1.0, (0, 1))], rij=rij, subsample=True)
    fr = np.logspace(-1, 0.5, 16)
    with pytest.raises(ValueError):                                # response rows of the wrong length
        pkg.narrow_band_least_squares_subsample([10.0, 10.0], 0.5, 1.0, _stream(4), None, None, 2, np.zeros(8), np.zeros(8),
                                                np.array([0.5, 1.0, 2.0]), 'log', fr, 'butter', 2, 0.01, rij=rij)
    with pytest.raises(ValueError):
        pkg.narrow_band_least_squares_subsample([10.0, 10.0], 0.5, 0.2, _stream(4), None, None, 2, np.zeros(16), np.zeros(16),
                                                np.array([0.5, 1.0, 2.0]), 'log', fr, 'butter', 2, 0.01, rij=rij)


def test_time_segmented_path_names_the_restriction(monkeypatch):
    from narrow_band_least_squares_amd import engine
    monkeypatch.setattr(engine, 'get_handle', lambda *a, **k: pytest.fail('the GPU was reached'))
    rij = np.array([[0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 1.0, 1.0]])
    with pytest.raises(ValueError, match='time-segmented') as err:
        engine.process_segmented(list(np.zeros((4, 600))), 20.0, 0.0, rij, [(0.5, 1.0)], [10.0], 0.5, 1.0, 'butter', 2, 0.01,
                                 None, want_subsample=True)
    assert 'want_subsample' in str(err.value)


def test_header_binding_and_library_carry_the_symbols():
    from narrow_band_least_squares_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    for s in SYMBOLS:
        assert re.search(r'^int %s\(nbls_handle\* h,' % s, header, re.M), s
        assert s in _hip.EXPORTS
    lib = _hip.load_library()
    for s in SYMBOLS:
        assert getattr(lib, s).argtypes is not None, s
    out = subprocess.run(['nm', '-D', '--defined-only', os.path.join(LIBDIR, 'libnbls_hip.so')], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    defined = set(re.findall(r' T (nbls_[a-z0-9_]+)', out.stdout))
    assert set(SYMBOLS) <= defined
    # the kernel is in the code object of the library (a missing kernel is an error, not a host loop)
    blob = open(os.path.join(LIBDIR, 'libnbls_hip.so'), 'rb').read()
    assert b'refine_lag_kernel' in blob
    # the pure host function that names the kernel's form
    assert 'nbls_refine_lds_bytes' in _hip.EXPORTS and 'nbls_refine_lds_bytes' in defined
    assert re.search(r'^int nbls_refine_lds_bytes\(int32_t nelem, int32_t W\);', header, re.M)
    assert _hip.refine_lds_bytes(8, 1280) == 80 * 1024 and _hip.refine_lds_bytes(8, 1281) == 0


def test_design_and_header_state_the_contract_alike():
    """DESIGN.md section 13 and include/nbls.h carry the same defining lines."""
    header = open(os.path.join(ROOT, 'include', 'nbls.h')).read()
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert re.search(r'^## 13\.', design, re.M)
    flat = lambda s: re.sub(r'[\s*`]+', ' ', s)
    for line in ('Nn = R(l-1) - R(l+1)', 'D = R(l-1) - 2 R(l) + R(l+1)', 'frac = 1/2 Nn / D, clamped to [-1/2, 1/2]',
                 'tau = ((double)lag + frac) / fs'):
        assert line in flat(header) and line in flat(design), line
