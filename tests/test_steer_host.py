"""What of the fractional-sample steering (``nbls_set_beam_interpolation``) a box without a GPU can
check: the new Python names, their signatures and argument checks, the two new symbols in the header, the ctypes binding and
the built library, and the compiler's resource report of the new kernel instances."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, 'narrow_band_least_squares_amd', 'csrc')
SYMBOLS = ('nbls_set_beam_interpolation', 'nbls_fetch_beam_grid_coefficients')
LTSVA_ARGS = ['st', 'lat_list', 'lon_list', 'window_length', 'window_overlap']
STEER_ARGS = ['alpha', 'rij', 'taps', 'slowness_grid', 'grid_map', 'subsample', 'kept', 'min_pairs']
STEER_DEFAULTS = dict(alpha=1.0, rij=None, taps=8, slowness_grid=None, grid_map=False, subsample=False, kept=False, min_pairs=None)


def test_python_names_and_signatures():
    import narrow_band_least_squares_amd as pkg
    from narrow_band_least_squares_amd import engine, planner, _hip
    for name in ('ltsva_steered', 'ltsva_steered_batch', 'narrow_band_least_squares_steered'):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    sig = inspect.signature(pkg.ltsva_steered).parameters
    assert list(sig) == LTSVA_ARGS + STEER_ARGS
    sigb = inspect.signature(pkg.ltsva_steered_batch).parameters
    assert list(sigb) == ['streams'] + LTSVA_ARGS[1:] + STEER_ARGS
    for k, v in STEER_DEFAULTS.items():
        assert sig[k].default == v and sigb[k].default == v and type(sig[k].default) is type(v), k
    ref_args = list(inspect.signature(pkg.narrow_band_least_squares).parameters)
    sign = inspect.signature(pkg.narrow_band_least_squares_steered).parameters
    assert list(sign) == ref_args + ['taps', 'slowness_grid', 'grid_map', 'subsample']
    assert sign['taps'].default == 8 and sign['slowness_grid'].default is None
    assert sign['grid_map'].default is False and sign['subsample'].default is False
    assert inspect.signature(engine.launch).parameters['beam_taps'].default == 0
    for f in (engine.process, engine.process_batch, engine.process_segmented):
        assert inspect.signature(f).parameters['beam_taps'].default == 0
    assert list(inspect.signature(planner.check_steering).parameters) == ['taps']
    assert list(inspect.signature(planner.steering_error).parameters) == ['taps', 'f_over_fs']
    assert inspect.signature(_hip.Handle.set_beam_interpolation).parameters['taps'].default == 8
    assert callable(_hip.Handle.fetch_beam_grid_coefficients)
    # the functions that were there keep their signatures
    assert list(inspect.signature(pkg.ltsva).parameters) == LTSVA_ARGS + ['alpha', 'plot_array_coordinates', 'rij']
    assert list(inspect.signature(pkg.ltsva_beam).parameters) == LTSVA_ARGS + ['alpha', 'rij']
    assert list(inspect.signature(pkg.ltsva_grid).parameters) == LTSVA_ARGS + ['slowness_grid', 'alpha', 'rij', 'grid_map']
    assert list(inspect.signature(pkg.ltsva_kept).parameters)[-2:] == ['peaks', 'peak_floor']
    assert list(inspect.signature(pkg.ltsva_batch).parameters)[-1] == 'slowness_grid'
    assert list(inspect.signature(pkg.ltsva_beam_trace).parameters)[-2:] == ['kept', 'min_pairs']
    assert list(inspect.signature(pkg.narrow_band_least_squares_beam).parameters) == ref_args
    assert list(inspect.signature(pkg.narrow_band_least_squares_grid).parameters) == ref_args + ['slowness_grid', 'grid_map']
    for f in (pkg.ltsva, pkg.ltsva_beam, pkg.ltsva_grid, pkg.ltsva_kept, pkg.ltsva_batch, pkg.ltsva_beam_trace, pkg.ltsva_seeded,
              pkg.narrow_band_least_squares, pkg.narrow_band_least_squares_beam, pkg.narrow_band_least_squares_grid):
        assert 'taps' not in inspect.signature(f).parameters
    assert list(inspect.signature(engine.launch).parameters)[-2:] == ['beam_trace', 'beam_taps']
    assert list(inspect.signature(engine.process).parameters)[-2:] == ['want_beam_trace', 'beam_taps']
    pkg.install_as_reference_modules()
    import lts_array
    import narrow_band_least_squares as nbls_mod
    assert lts_array.ltsva_steered is pkg.ltsva_steered
    assert nbls_mod.narrow_band_least_squares_steered is pkg.narrow_band_least_squares_steered


def test_check_steering():
    from narrow_band_least_squares_amd import planner
    for good in (0, 4, 6, 8, np.int32(8)):
        assert planner.check_steering(good) == int(good) and type(planner.check_steering(good)) is int
    for bad in (1, 2, 3, 5, 7, 10, 16, -4, 8.0, '8', None, True, False, [8]):
        with pytest.raises(ValueError):
            planner.check_steering(bad)


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
    bad_kw = [dict(taps=5), dict(taps=8.0), dict(taps=True), dict(taps=None), dict(slowness_grid=np.zeros((3, 3))),
              dict(grid_map=True), dict(slowness_grid=grid, grid_map=1), dict(subsample=1), dict(kept=1), dict(min_pairs=2),
              dict(kept=True, min_pairs=7), dict(alpha=0.3)]
    for kw in bad_kw:
        with pytest.raises(ValueError):
            pkg.ltsva_steered(_stream(4), None, None, 10.0, 0.5, rij=rij, **kw)
        with pytest.raises(ValueError):
            pkg.ltsva_steered_batch([_stream(4), _stream(4)], None, None, 10.0, 0.5, rij=rij, **kw)
    with pytest.raises(ValueError):
        pkg.ltsva_steered(_stream(2), None, None, 10.0, 0.5, rij=rij[:, :2])
    with pytest.raises(ValueError):
        pkg.ltsva_steered(_stream(3), None, None, 10.0, 0.5, alpha=0.75, rij=rij[:, :3])           # LTS needs four elements
    assert pkg.ltsva_steered_batch([], None, None, 10.0, 0.5) == []
    # the engine: taps that are not 0 / 4 / 6 / 8, and steering with nothing to steer
    rows = list(np.zeros((4, 600)))
    for kw in (dict(beam_taps=5, want_beam=True), dict(beam_taps=8), dict(beam_taps=True, want_beam=True)):
        with pytest.raises(ValueError):
            engine.process(rows, 20.0, 0.0, rij, [(None, None)], [10.0], 0.5, 1.0, prefiltered=True, **kw)
        with pytest.raises(ValueError):
            engine.process_batch([rows] * 2, 20.0, [0.0, 0.0], rij, [(None, None)], [10.0], 0.5, 1.0, prefiltered=True, **kw)
    # the time-segmented path keeps the filtered band on the host: refused, as the beam is
    with pytest.raises(ValueError, match='time-segmented'):
        engine.process_segmented(rows, 20.0, 0.0, rij, [(0.5, 2.0)], [10.0], 0.5, 1.0, 'butter', 2, None, 30, beam_taps=8,
                                 slowness_grid=grid)
    fr = np.logspace(-1, 0.5, 16)
    args = ([10.0, 10.0], 0.5, 1.0, _stream(4), None, None, 2, np.zeros(16), np.zeros(16), np.array([0.5, 1.0, 2.0]), 'log', fr,
            'butter', 2, 0.01)
    for kw in (dict(taps=3), dict(taps=8.0), dict(grid_map=True), dict(slowness_grid=np.zeros((2, 3))), dict(subsample=0)):
        with pytest.raises(ValueError):
            pkg.narrow_band_least_squares_steered(*args, rij=rij, **kw)
    with pytest.raises(TypeError):                                 # the extensions are keywords
        pkg.narrow_band_least_squares_steered(*args, rij, 8)


def test_header_declares_and_binding_knows_the_symbols():
    from narrow_band_least_squares_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'nbls.h'), encoding='utf-8').read()
    assert re.search(r'^int nbls_set_beam_interpolation\(nbls_handle\* h, int32_t taps\);', header, re.M)
    assert re.search(r'^int nbls_fetch_beam_grid_coefficients\(nbls_handle\* h, double\* c /\* \[G\]\[N\]\[taps\] \*/\);', header, re.M)
    for s in SYMBOLS:
        assert s in _hip.EXPORTS
    assert _hip.STEER_TAPS == (0, 4, 6, 8)
    # the defining lines of the header name the operations the truth restates
    for phrase in ('n_i = floor(tau_i)', 'mu_i = tau_i - n_i', 'one division', 'a zero coefficient is still', 'floor, not rint'):
        assert phrase in header, phrase


def test_library_exports_and_prototypes():
    import ctypes as C
    from narrow_band_least_squares_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('library not built')
    lib = _hip.load_library()
    dp = C.POINTER(C.c_double)
    assert lib.nbls_set_beam_interpolation.argtypes == [C.c_void_p, C.c_int32]
    assert lib.nbls_fetch_beam_grid_coefficients.argtypes == [C.c_void_p, dp]
    # without a handle both are argument errors, not crashes
    assert lib.nbls_set_beam_interpolation(None, 8) == _hip.NBLS_ERR_ARG
    assert lib.nbls_fetch_beam_grid_coefficients(None, None) == _hip.NBLS_ERR_ARG


def test_new_instances_use_no_scratch_and_spill_nothing(tmp_path):
    """The compiler's resource report of beam_steer.hip (beam.hip built a second time for the interpolated instances of
    beam_fstat_kernel; beam.hip itself still gives its two whole-sample kernels) and beam_grid.hip: every instance without a private segment and without a spilled
    vector register; the grid kernel's sixteen waves keep within 128 VGPRs."""
    hipcc = '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    for src, kernel, count in (('beam_steer.hip', 'beam_fstat_kernel', 6), ('beam_grid.hip', 'beam_grid_kernel', 8)):
        out = tmp_path / (src + '.s')
        subprocess.run([hipcc, '-O3', '-std=c++17', '--offload-arch=gfx950', '-I' + LIBDIR, '-S', '--cuda-device-only',
                        os.path.join(LIBDIR, src), '-o', str(out), '-ffp-contract=off'], check=True,
                       stderr=subprocess.DEVNULL, timeout=900)
        text = out.read_text()
        found = re.findall(r'\.amdhsa_kernel (\S*%s\S*)(.*?)\.end_amdhsa_kernel' % kernel, text, re.S)
        assert len(found) == count, [n for n, _ in found]
        assert sorted(re.search(r'ELi(\d)E', n).group(1) for n, _ in found) == ['0', '0', '4', '4', '6', '6', '8', '8'][8 - count:]
        for name, body in found:
            assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0, name
            if kernel == 'beam_grid_kernel':
                assert int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1)) <= 128, name
        for key in ('vgpr_spill_count', 'private_segment_fixed_size'):
            vals = re.findall(r'\.%s:\s+(\d+)' % key, text)
            assert len(vals) == count and all(int(v) == 0 for v in vals), (src, key, vals)
        if kernel == 'beam_grid_kernel':
            # the taps of the staged form are single ds_read_b64 (256 B/clk/CU): no pair is merged into a half-rate ds_read2
            assert 'ds_read_b64' in text and 'ds_read2' not in text
    mk = open(os.path.join(LIBDIR, 'Makefile'), encoding='utf-8').read()
    assert 'beam_steer.o' in re.search(r'^OBJS = (.*)$', mk, re.M).group(1) and 'beam_steer.hip' in re.search(r'^DEVSRC = (.*)$', mk, re.M).group(1)
    assert re.search(r'^beam_steer\.o: beam_steer\.hip beam\.hip ', mk, re.M)
    for obj in ('beam', 'beam_steer', 'beam_grid'):
        assert re.search(r'^%s\.o:.* steer\.h .*\n\t\$\(HIPCC\) \$\(CXXFLAGS\) \$\(NOFMA\) -c' % obj, mk, re.M), obj
