"""What of the element delays (``nbls_set_element_delays``) a box without a GPU can check: the new
Python names, their signatures and argument checks, the three new symbols and two macros in the header, the ctypes binding
and the built library, ``nbls_element_delay_lds_bytes`` at the 156 KiB edge, the Makefile, and the compiler's resource report
of the eight kernel instances."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import element_delay_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, 'narrow_band_least_squares_amd', 'csrc')
SYMBOLS = ('nbls_set_element_delays', 'nbls_fetch_element_delays', 'nbls_element_delay_lds_bytes')
LTSVA_ARGS = ['st', 'lat_list', 'lon_list', 'window_length', 'window_overlap']
NEW_ARGS = ['alpha', 'rij', 'max_shift', 'kept', 'min_pairs']
NEW_DEFAULTS = dict(alpha=1.0, rij=None, max_shift=None, kept=False, min_pairs=None)


def test_python_names_and_signatures():
    import narrow_band_least_squares_amd as pkg
    from narrow_band_least_squares_amd import engine, planner, _hip
    for name in ('ltsva_element_delays', 'ltsva_element_delays_batch', 'narrow_band_least_squares_element_delays'):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    sig = inspect.signature(pkg.ltsva_element_delays).parameters
    assert list(sig) == LTSVA_ARGS + NEW_ARGS
    sigb = inspect.signature(pkg.ltsva_element_delays_batch).parameters
    assert list(sigb) == ['streams'] + LTSVA_ARGS[1:] + NEW_ARGS
    for k, v in NEW_DEFAULTS.items():
        assert sig[k].default == v and sigb[k].default == v and type(sig[k].default) is type(v), k
    ref_args = list(inspect.signature(pkg.narrow_band_least_squares).parameters)
    sign = inspect.signature(pkg.narrow_band_least_squares_element_delays).parameters
    assert list(sign) == ref_args + ['max_shift', 'kept', 'min_pairs']
    assert sign['max_shift'].default is None and sign['kept'].default is False and sign['min_pairs'].default is None
    assert all(sign[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ('max_shift', 'kept', 'min_pairs'))
    # the engine: the new keywords stand before the pinned tails and are passed by name
    assert list(inspect.signature(engine.launch).parameters)[-4:] == ['element_delays', 'element_delays_kept', 'beam_trace', 'beam_taps']
    assert list(inspect.signature(engine.process).parameters)[-4:] == ['element_max_shift', 'element_delays_kept', 'want_beam_trace',
                                                                       'beam_taps']
    assert list(inspect.signature(engine.launch).parameters)[-2:] == ['beam_trace', 'beam_taps']
    assert list(inspect.signature(engine.process).parameters)[-2:] == ['want_beam_trace', 'beam_taps']
    for f in (engine.process, engine.process_batch, engine.process_segmented):
        assert inspect.signature(f).parameters['element_max_shift'].default is None
    for f in (engine.process, engine.process_batch):
        assert inspect.signature(f).parameters['element_delays_kept'].default is False
    assert inspect.signature(engine.launch).parameters['element_delays'].default is None
    assert inspect.signature(engine.launch).parameters['element_delays_kept'].default is False
    assert inspect.signature(engine.new_result).parameters['want_element_delays'].default is False
    assert list(inspect.signature(planner.element_shifts).parameters) == ['fmax_list', 'fs', 'period_fraction']
    assert inspect.signature(planner.element_shifts).parameters['period_fraction'].default == 0.5
    assert list(inspect.signature(planner.check_element_shifts).parameters) == ['max_shift', 'nbands']
    assert list(inspect.signature(_hip.Handle.set_element_delays).parameters) == ['self', 'max_shift', 'kept']
    assert inspect.signature(_hip.Handle.set_element_delays).parameters['kept'].default is False
    assert callable(_hip.Handle.fetch_element_delays)
    assert _hip.ELEMENT_DELAY_KEPT == 1 and _hip.ELEMENT_DELAY_MAX_SHIFT == 256 == planner.ELEMENT_DELAY_MAX_SHIFT
    # the functions that were there keep their signatures
    assert list(inspect.signature(pkg.ltsva).parameters) == LTSVA_ARGS + ['alpha', 'plot_array_coordinates', 'rij']
    assert list(inspect.signature(pkg.ltsva_beam).parameters) == LTSVA_ARGS + ['alpha', 'rij']
    assert list(inspect.signature(pkg.ltsva_grid).parameters) == LTSVA_ARGS + ['slowness_grid', 'alpha', 'rij', 'grid_map']
    assert list(inspect.signature(pkg.ltsva_kept).parameters)[-2:] == ['peaks', 'peak_floor']
    assert list(inspect.signature(pkg.ltsva_kept_batch).parameters)[-1] == 'peak_floor'
    assert list(inspect.signature(pkg.ltsva_batch).parameters)[-1] == 'slowness_grid'
    assert list(inspect.signature(pkg.ltsva_beam_trace).parameters)[-4:] == ['mdccm_min', 'window', 'kept', 'min_pairs']
    assert list(inspect.signature(pkg.ltsva_steered).parameters) == LTSVA_ARGS + ['alpha', 'rij', 'taps', 'slowness_grid', 'grid_map',
                                                                                 'subsample', 'kept', 'min_pairs']
    assert list(inspect.signature(pkg.narrow_band_least_squares_beam).parameters) == ref_args
    assert list(inspect.signature(pkg.narrow_band_least_squares_grid).parameters) == ref_args + ['slowness_grid', 'grid_map']
    assert list(inspect.signature(pkg.narrow_band_least_squares_beam_trace).parameters) == ref_args + ['mdccm_min', 'window', 'kept']
    assert list(inspect.signature(pkg.narrow_band_least_squares_steered).parameters) == ref_args + ['taps', 'slowness_grid', 'grid_map',
                                                                                                     'subsample']
    for f in (pkg.ltsva, pkg.ltsva_beam, pkg.ltsva_grid, pkg.ltsva_kept, pkg.ltsva_batch, pkg.ltsva_beam_trace, pkg.ltsva_steered,
              pkg.narrow_band_least_squares, pkg.narrow_band_least_squares_beam, pkg.narrow_band_least_squares_steered):
        assert 'max_shift' not in inspect.signature(f).parameters
    import sys
    saved = {k: sys.modules.get(k) for k in ('narrow_band_least_squares', 'helpers', 'lts_array')}
    try:
        pkg.install_as_reference_modules()
        import lts_array
        import narrow_band_least_squares as nb
        assert lts_array.ltsva_element_delays is pkg.ltsva_element_delays
        assert nb.narrow_band_least_squares_element_delays is pkg.narrow_band_least_squares_element_delays
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v


def test_new_result_fields():
    from narrow_band_least_squares_amd import engine
    nwin = np.array([5, 3])
    res = engine.new_result(4, 0.5, 20.0, np.array([64, 64]), np.array([32, 32]), nwin, 8, want_element_delays=True)
    for k, dt in (('element_delay', np.float64), ('element_cc', np.float64), ('element_shift', np.int32)):
        a = getattr(res, k)
        assert a.shape == (2, 8, 4) and a.dtype == dt and not a.any()
    plain = engine.new_result(4, 0.5, 20.0, np.array([64, 64]), np.array([32, 32]), nwin, 8)
    assert plain.element_delay is None and plain.element_cc is None and plain.element_shift is None


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
    bad_kw = [dict(), dict(max_shift=None), dict(max_shift=-1), dict(max_shift=257), dict(max_shift=3.0), dict(max_shift=True),
              dict(max_shift=[3, 3]), dict(max_shift='3'), dict(max_shift=3, kept=1), dict(max_shift=3, min_pairs=2),
              dict(max_shift=3, kept=True, min_pairs=7), dict(max_shift=3, alpha=0.3)]
    for kw in bad_kw:
        with pytest.raises(ValueError):
            pkg.ltsva_element_delays(_stream(4), None, None, 10.0, 0.5, rij=rij, **kw)
        with pytest.raises(ValueError):
            pkg.ltsva_element_delays_batch([_stream(4), _stream(4)], None, None, 10.0, 0.5, rij=rij, **kw)
    with pytest.raises(ValueError, match='max_shift is required'):
        pkg.ltsva_element_delays(_stream(4), None, None, 10.0, 0.5, rij=rij)
    with pytest.raises(ValueError):
        pkg.ltsva_element_delays(_stream(2), None, None, 10.0, 0.5, rij=rij[:, :2], max_shift=3)
    with pytest.raises(ValueError):
        pkg.ltsva_element_delays(_stream(3), None, None, 10.0, 0.5, alpha=0.75, rij=rij[:, :3], max_shift=3)   # LTS needs four elements
    assert pkg.ltsva_element_delays_batch([], None, None, 10.0, 0.5) == []
    # the engine
    rows = list(np.zeros((4, 600)))
    for kw in (dict(element_max_shift=257), dict(element_max_shift=[1, 2]), dict(element_max_shift=2.5),
               dict(element_max_shift=3, element_delays_kept=True),              # KEPT without a plan that names the elements
               dict(element_max_shift=3, element_delays_kept=1), dict(element_delays_kept=True)):
        with pytest.raises(ValueError):
            engine.process(rows, 20.0, 0.0, rij, [(None, None)], [10.0], 0.5, 1.0, prefiltered=True, **kw)
        with pytest.raises(ValueError):
            engine.process_batch([rows] * 2, 20.0, [0.0, 0.0], rij, [(None, None)], [10.0], 0.5, 1.0, prefiltered=True, **kw)
    rij33 = np.random.default_rng(1).standard_normal((2, 33))
    with pytest.raises(ValueError, match='32'):
        engine.process(list(np.zeros((33, 600))), 20.0, 0.0, rij33, [(None, None)], [10.0], 0.5, 1.0, prefiltered=True,
                       element_max_shift=3)
    # the time-segmented path keeps the filtered band on the host: refused, as the beam is
    with pytest.raises(ValueError, match='time-segmented'):
        engine.process_segmented(rows, 20.0, 0.0, rij, [(0.5, 2.0)], [10.0], 0.5, 1.0, 'butter', 2, None, 30,
                                 element_max_shift=np.array([3], dtype=np.int32))
    fr = np.logspace(-1, 0.5, 16)
    args = ([10.0, 10.0], 0.5, 1.0, _stream(4), None, None, 2, np.zeros(16), np.zeros(16), np.array([0.5, 1.0, 2.0]), 'log', fr,
            'butter', 2, 0.01)
    for kw in (dict(max_shift=300), dict(max_shift=[1, 2, 3]), dict(max_shift=1.5), dict(kept=1), dict(min_pairs=2),
               dict(kept=True, min_pairs=9)):
        with pytest.raises(ValueError):
            pkg.narrow_band_least_squares_element_delays(*args, rij=rij, **kw)
    with pytest.raises(TypeError):                                 # the extensions are keywords
        pkg.narrow_band_least_squares_element_delays(*args, rij, 3)


def test_header_declares_and_binding_knows_the_symbols():
    from narrow_band_least_squares_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'nbls.h'), encoding='utf-8').read()
    assert re.search(r'^int nbls_set_element_delays\(nbls_handle\* h, const int32_t\* max_shift /\* \[nbands\]; NULL = off \*/, '
                     r'int32_t nbands, int32_t flags\);', header, re.M)
    assert re.search(r'^int nbls_fetch_element_delays\(nbls_handle\* h, double\* delay, double\* cc, int32_t\* shift\);', header, re.M)
    assert re.search(r'^int nbls_element_delay_lds_bytes\(int32_t nelem, int32_t W, int32_t max_shift\);', header, re.M)
    assert re.search(r'^#define NBLS_ELEMENT_DELAY_KEPT 1\b', header, re.M)
    assert re.search(r'^#define NBLS_ELEMENT_DELAY_MAX_SHIFT 256\b', header, re.M)
    for s in SYMBOLS:
        assert s in _hip.EXPORTS
    # the defining lines of the header name the operations the truth restates
    for phrase in ('d_m = rint(tau_m), ties to even', 'c descending, |k| ascending, k ascending', 'b_m[t] = b[t] - y_m(0)[t]',
                   'c_m(k) = C_m(k) / sqrt(E_m(k) * E_b,m)', '((((double)(d_m + k*)) + frac) - tau_m) / fs', 'not zero padding'):
        assert phrase in header, phrase


def test_library_exports_prototypes_and_the_lds_formula():
    from narrow_band_least_squares_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('library not built')
    lib = _hip.load_library()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert lib.nbls_set_element_delays.argtypes == [C.c_void_p, ip, C.c_int32, C.c_int32]
    assert lib.nbls_fetch_element_delays.argtypes == [C.c_void_p, dp, dp, ip]
    assert lib.nbls_element_delay_lds_bytes.argtypes == [C.c_int32, C.c_int32, C.c_int32]
    # without a handle both are argument errors, not crashes
    assert lib.nbls_set_element_delays(None, None, 0, 0) == _hip.NBLS_ERR_ARG
    assert lib.nbls_fetch_element_delays(None, None, None, None) == _hip.NBLS_ERR_ARG
    # the pure host function: (nelem (W + 2K) + W) * 8 up to 156 KiB, 0 beyond
    f = lib.nbls_element_delay_lds_bytes
    edge = 156 * 1024
    for N, W, K in cases.SHAPES + cases.BOUNDARY + [(8, 1200, 18), (8, 2400, 18), (1, 1, 0), (3, 19967, 0), (1, 9984, 0)]:
        want = (N * (W + 2 * K) + W) * 8
        assert f(N, W, K) == (want if want <= edge else 0) == cases.lds_bytes(N, W, K), (N, W, K)
    assert f(1, 9984, 0) == edge and f(1, 9985, 0) == 0                  # exactly 156 KiB fits, 16 bytes more do not
    assert f(2, 6656, 0) == edge and f(2, 6655, 1) == 0 and f(2, 6654, 1) == edge - 16
    assert f(8, 1200, 18) == 88704 and f(8, 2400, 18) == 0
    for staged, glob in zip(cases.BOUNDARY[0::2], cases.BOUNDARY[1::2]):
        assert f(*staged) > 0 and f(*glob) == 0
    for bad in ((0, 16, 1), (-1, 16, 1), (4, 0, 1), (4, -5, 1), (4, 16, -1), (4, 16, 257)):
        assert f(*bad) == _hip.NBLS_ERR_ARG, bad
    assert f(4, 16, 256) == (4 * (16 + 512) + 16) * 8


def test_makefile_and_resource_report(tmp_path):
    """csrc/element_delay.hip is built as beam_grid.hip is (without contraction), listed for both libraries, and every
    instance of its kernel has no private segment and spills no vector register; sixteen waves keep within 128 VGPRs."""
    mk = open(os.path.join(LIBDIR, 'Makefile'), encoding='utf-8').read()
    assert 'element_delay.o' in re.search(r'^OBJS = (.*)$', mk, re.M).group(1).split()
    assert 'element_delay.hip' in re.search(r'^DEVSRC = (.*)$', mk, re.M).group(1).split()
    rule = re.search(r'^element_delay\.o: (.*)\n\t(.*)$', mk, re.M)
    grid = re.search(r'^beam_grid\.o: (.*)\n\t(.*)$', mk, re.M)
    assert rule and rule.group(2) == grid.group(2) and '$(NOFMA)' in rule.group(2)
    for dep in ('element_delay.hip', 'nbls_internal.h', 'dev_buf.h', 'wave_ops.h', 'refine_fraction.h', '../../include/nbls.h'):
        assert dep in rule.group(1).split(), dep
    hipcc = '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = tmp_path / 'element_delay.s'
    subprocess.run([hipcc, '-O3', '-std=c++17', '--offload-arch=gfx950', '-I' + LIBDIR, '-S', '--cuda-device-only',
                    os.path.join(LIBDIR, 'element_delay.hip'), '-o', str(out), '-ffp-contract=off'], check=True,
                   stderr=subprocess.DEVNULL, timeout=900)
    text = out.read_text()
    found = re.findall(r'\.amdhsa_kernel (\S*element_delay_kernel\S*)(.*?)\.end_amdhsa_kernel', text, re.S)
    assert len(found) == 8, [n for n, _ in found]                        # staged / global x plain / KEPT x one / four shifts per item
    for name, body in found:
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0, name
        assert int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1)) <= 128, name
        # the static LDS leaves the staged form its 156 KiB of a CU's 160
        assert int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1)) <= 4096, name
    for key in ('vgpr_spill_count', 'private_segment_fixed_size'):
        vals = re.findall(r'\.%s:\s+(\d+)' % key, text)
        assert len(vals) == 8 and all(int(v) == 0 for v in vals), (key, vals)
