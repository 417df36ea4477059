"""What of the beam results (``nbls_set_beam``) a box without a GPU can check: the CPU reference of
tests/beam_truth.py against closed forms, the new Python names and their argument checks, the three new symbols in the
header, the ctypes binding and the built library, and a plain-C caller that compiles and links."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import beam_truth as bt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, 'tests', 'c_caller')
LIBDIR = os.path.join(ROOT, 'narrow_band_least_squares_amd', 'csrc')
SYMBOLS = ('nbls_set_beam', 'nbls_fetch_beam', 'nbls_est_fetch_beam')


def test_reference_identical_channels_line_up_exactly():
    """N copies of one channel, zero delays: b = N x, S_b = N^2 sum x^2 = N S_t, D = 0, fstat = +inf, beam_power = mean x^2."""
    rng = np.random.default_rng(1)
    x = rng.integers(-1000, 1000, 300).astype(np.float64)        # integers: every sum is exact
    for N in (3, 5):
        filt = np.tile(x, (N, 1))
        ref = bt.beam_reference(filt, 20.0, np.ones((N * (N - 1) // 2, 2)), np.zeros((4, 2)), 65, 32, 4)
        for k in range(4):
            assert ref['S_b'][k] == N * ref['S_t'][k] and ref['D'][k] == 0
            assert ref['fstat'][k] == np.inf
            assert ref['beam_power'][k] == np.mean(x[32 * k:32 * k + 65] ** 2)


def test_reference_cancelling_channels_and_empty_window():
    """x, -x and a dead channel: b = 0, S_b = 0, fstat = 0 (D = 3 S_t > 0); an all-zero window: beam_power 0, fstat NaN."""
    rng = np.random.default_rng(2)
    x = rng.integers(-1000, 1000, 200).astype(np.float64)
    x[100:] = 0.0
    filt = np.stack([x, -x, np.zeros_like(x)])
    ref = bt.beam_reference(filt, 20.0, np.ones((3, 2)), np.zeros((2, 2)), 50, 100, 2)
    assert ref['S_b'][0] == 0 and ref['S_t'][0] > 0 and ref['fstat'][0] == 0.0 and ref['beam_power'][0] == 0.0
    assert ref['S_t'][1] == 0 and np.isnan(ref['fstat'][1]) and ref['beam_power'][1] == 0.0


def test_reference_delays_by_hand():
    """Three elements, fs = 20, z = (0.5, -0.25) s/km, xij rows of the pairs (0, 1), (0, 2) = (-1.3, 0.2), (0.45, 0.9):
    tau = 20 (-0.65 - 0.05) = -14 and 20 (0.225 - 0.225) = 0 -> d = (0, -14, 0).  Ties go to even: 20 * 0.125 = 2.5 -> 2,
    20 * 0.175 = 3.5 -> 4.  x_1 is read 14 samples EARLIER; before the trace's start the samples are zeros."""
    xij = np.array([[-1.3, 0.2], [0.45, 0.9], [1.75, 0.7]])
    d, near = bt.delays(xij[:2], (0.5, -0.25), 20.0)
    assert list(d) == [0, -14, 0] and not near
    d, near = bt.delays(np.array([[0.125, 0.0], [0.175, 0.0]]), (1.0, 0.0), 20.0)
    assert list(d) == [0, 2, 4] and near                           # (such a window is left out of a GPU comparison)
    assert bt.delays(xij[:2], (np.inf, 0.0), 20.0)[0] is None
    assert bt.delays(xij[:2], (2.0 ** 30, 0.0), 20.0)[0] is None
    npts, W = 64, 8
    filt = np.zeros((3, npts))
    filt[0] = np.arange(npts) + 1.0
    filt[1] = 100.0 + np.arange(npts)
    filt[2] = -1.0
    ref = bt.beam_reference(filt, 20.0, xij, np.tile([0.5, -0.25], (3, 1)), W, 10, 3)
    # window 0 (s0 = 0): x_1 reads samples -14 .. -7: zeros.  b = x_0 - 1
    t = np.arange(W)
    b0 = (t + 1.0) - 1.0
    assert ref['S_b'][0] == np.sum(b0 ** 2) and ref['S_t'][0] == np.sum((t + 1.0) ** 2) + W
    # window 1 (s0 = 10): x_1 reads samples -4 .. 3: four zeros, then filt[1][0 .. 3]
    x1 = np.concatenate((np.zeros(4), 100.0 + np.arange(4)))
    b1 = (10 + t + 1.0) + x1 - 1.0
    assert ref['S_b'][1] == np.sum(b1 ** 2)
    # window 2 (s0 = 20): x_1 = filt[1][6 .. 13]
    b2 = (20 + t + 1.0) + (100.0 + 6 + t) - 1.0
    assert ref['S_b'][2] == np.sum(b2 ** 2)
    N, S_b, S_t = 3, ref['S_b'][2], ref['S_t'][2]
    assert ref['beam_power'][2] == float(S_b / (9 * W)) and ref['fstat'][2] == float(2 * S_b / (N * S_t - S_b))
    # a NaN sample makes exactly the windows NaN whose reads touch it (x_1 of window 2 reads sample 6, window 1 does not)
    filt[1, 6] = np.nan
    ref = bt.beam_reference(filt, 20.0, xij, np.tile([0.5, -0.25], (3, 1)), W, 10, 3)
    assert np.isnan(ref['fstat'][2]) and np.isnan(ref['beam_power'][2]) and np.isfinite(ref['fstat'][1])


def test_tolerance_is_the_stated_bound():
    rng = np.random.default_rng(3)
    filt = rng.standard_normal((4, 500))
    ref = bt.beam_reference(filt, 20.0, np.zeros((6, 2)), np.zeros((1, 2)), 257, 100, 1)
    N, W = 4, 257
    E = 64.0 * N * W * 2.0 ** -53 * N * float(ref['S_t'][0])
    D, S_b = float(ref['D'][0]), float(ref['S_b'][0])
    assert ref['tol_power'][0] == pytest.approx(E / (N * N * W), rel=1e-12)
    assert ref['tol_fstat'][0] == pytest.approx((N - 1) * (E * D + 2 * E * S_b) / D ** 2, rel=1e-12)
    assert not ref['power_only'][0] and not ref['skip'][0]


def test_python_names_and_signatures():
    import narrow_band_least_squares_amd as pkg
    from narrow_band_least_squares_amd import engine, _hip
    for name in ('ltsva_beam', 'narrow_band_least_squares_beam'):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    assert list(inspect.signature(pkg.ltsva_beam).parameters) == ['st', 'lat_list', 'lon_list', 'window_length',
                                                                   'window_overlap', 'alpha', 'rij']
    ref_args = list(inspect.signature(pkg.narrow_band_least_squares).parameters)
    assert list(inspect.signature(pkg.narrow_band_least_squares_beam).parameters) == ref_args
    for f in (pkg.ltsva_batch, pkg.ltsva_multi):
        assert inspect.signature(f).parameters['beam'].default is False
    # the reference-named functions keep their signatures
    assert list(inspect.signature(pkg.ltsva).parameters) == ['st', 'lat_list', 'lon_list', 'window_length', 'window_overlap',
                                                              'alpha', 'plot_array_coordinates', 'rij']
    for f in (engine.process, engine.process_batch, engine.process_multi, engine.process_segmented):
        assert inspect.signature(f).parameters['want_beam'].default is False
    assert inspect.signature(_hip.Handle.fetch_beam).parameters['e'].default == 0 and hasattr(_hip.Handle, 'set_beam')
    # under the reference's module names the new functions are attributes of the same modules
    pkg.install_as_reference_modules()
    import lts_array
    import narrow_band_least_squares as nbls_mod
    assert lts_array.ltsva_beam is pkg.ltsva_beam and nbls_mod.narrow_band_least_squares_beam is pkg.narrow_band_least_squares_beam
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
    rij = np.array([[0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 1.0, 1.0]])
    with pytest.raises(ValueError):
        pkg.ltsva_beam(_stream(4), None, None, 10.0, 0.5, alpha=0.3, rij=rij)
    with pytest.raises(ValueError):
        pkg.ltsva_beam(_stream(2), None, None, 10.0, 0.5, alpha=1.0, rij=rij[:, :2])
    with pytest.raises(ValueError):
        pkg.ltsva_beam(_stream(3), None, None, 10.0, 0.5, alpha=0.75, rij=rij[:, :3])        # LTS needs four elements
    with pytest.raises(ValueError):
        pkg.ltsva_batch([_stream(4), _stream(4, npts=500)], None, None, 10.0, 0.5, rij=rij, beam=True)
    with pytest.raises(ValueError):
        pkg.ltsva_batch([_stream(4), _stream(4)], None, None, 10.0, 0.5, rij=rij, beam='yes')
    with pytest.raises(ValueError):
        pkg.ltsva_multi(_stream(4), None, None, 10.0, 0.5, [], rij=rij, beam=True)
    with pytest.raises(ValueError):
        pkg.ltsva_multi(_stream(4), None, None, 10.0, 0.5, [(1.0, (0, 1))], rij=rij, beam=True)
    with pytest.raises(ValueError):
        pkg.ltsva_multi(_stream(4), None, None, 10.0, 0.5, [1.0, 0.75], rij=rij, beam=1)
    fr = np.logspace(-1, 0.5, 16)
    with pytest.raises(ValueError):                                # response rows of the wrong length
        pkg.narrow_band_least_squares_beam([10.0, 10.0], 0.5, 1.0, _stream(4), None, None, 2, np.zeros(8), np.zeros(8),
                                           np.array([0.5, 1.0, 2.0]), 'log', fr, 'butter', 2, 0.01, rij=rij)
    with pytest.raises(ValueError):
        pkg.narrow_band_least_squares_beam([10.0, 10.0], 0.5, 0.2, _stream(4), None, None, 2, np.zeros(16), np.zeros(16),
                                           np.array([0.5, 1.0, 2.0]), 'log', fr, 'butter', 2, 0.01, rij=rij)
    # the time-segmented fallback keeps the band on the host: it names the limit instead of computing on the host
    with pytest.raises(ValueError, match='time-segmented'):
        engine.process_segmented(list(np.zeros((4, 600))), 20.0, 0.0, rij, [(0.5, 1.0)], [10.0], 0.5, 1.0, 'butter', 2, 0.01,
                                 None, want_beam=True)


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
    assert b'beam_fstat_kernel' in blob


def build_beam_caller():
    binary = os.path.join(CDIR, 'beam_caller')
    cmd = ['gcc', '-O1', '-Wall', '-Wextra', '-Werror', '-std=c11', '-pthread', '-I', os.path.join(ROOT, 'include'),
           os.path.join(CDIR, 'beam_caller.c'), '-o', binary, '-L', LIBDIR, '-lnbls_hip', '-lm',
           '-Wl,-rpath,$ORIGIN/../../narrow_band_least_squares_amd/csrc', '-Wl,-rpath-link,/opt/rocm/lib']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return binary


def test_plain_c_caller_compiles_and_links():
    binary = build_beam_caller()
    out = subprocess.run(['nm', '-u', binary], capture_output=True, text=True).stdout
    assert {'nbls_set_beam', 'nbls_fetch_beam', 'nbls_plan', 'nbls_execute'} <= set(re.findall(r'\b(nbls_[a-z0-9_]+)', out))
