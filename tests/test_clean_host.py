"""Host side of the CLEAN-SC components (``nbls_set_capon_clean``): names, signatures and defaults of
everything new, every earlier signature as it was, the header's declarations and their bindings, every ``ValueError`` before
any GPU call, the LDS formula, the Makefile's lines and the compiler's resource report.  CPU only."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import narrow_band_least_squares_amd as pkg
from narrow_band_least_squares_amd import _hip, engine, lts_array, planner, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, 'narrow_band_least_squares_amd', 'csrc')
SYMBOLS = ['nbls_set_capon_clean', 'nbls_fetch_capon_clean', 'nbls_fetch_capon_clean_csdm', 'nbls_capon_clean_lds_bytes']
FS = 20.0
GRID = planner.slowness_grid(3.0, 5)
LTSVA_ARGS = ['st', 'lat_list', 'lon_list', 'window_length', 'window_overlap']


def _defaults(f):
    return {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}


def test_public_names_signatures_and_defaults():
    for name in ('ltsva_clean', 'ltsva_clean_batch', 'narrow_band_least_squares_clean', 'clean_map', 'clean_sources'):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    tail = ['slowness_grid', 'freq', 'alpha', 'rij', 'snapshots', 'iterations', 'gain', 'floor', 'kept', 'min_pairs', 'merge_radius',
            'max_sources']
    assert list(inspect.signature(pkg.ltsva_clean).parameters) == LTSVA_ARGS + tail
    assert list(inspect.signature(pkg.ltsva_clean_batch).parameters) == ['streams'] + LTSVA_ARGS[1:] + tail
    want = dict(alpha=1.0, rij=None, snapshots=None, iterations=16, gain=0.5, floor=0.02, kept=False, min_pairs=None,
                merge_radius=None, max_sources=4)
    assert _defaults(pkg.ltsva_clean) == want and _defaults(pkg.ltsva_clean_batch) == want
    ref_args = list(inspect.signature(pkg.narrow_band_least_squares).parameters)
    sig = inspect.signature(pkg.narrow_band_least_squares_clean)
    assert list(sig.parameters) == ref_args + ['slowness_grid', 'capon_freqs', 'snapshots', 'iterations', 'gain', 'floor',
                                               'merge_radius', 'max_sources']
    for k in list(sig.parameters)[len(ref_args):]:
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert sig.parameters['slowness_grid'].default is inspect.Parameter.empty
    assert (sig.parameters['iterations'].default, sig.parameters['gain'].default, sig.parameters['floor'].default) == (16, 0.5, 0.02)
    assert list(inspect.signature(pkg.clean_map).parameters) == ['index', 'power', 'count', 'G']
    assert list(inspect.signature(pkg.clean_sources).parameters) == ['index', 'power', 'count', 'grid', 'radius', 'max_sources']
    assert list(inspect.signature(_hip.Handle.set_capon_clean).parameters) == ['self', 'iterations', 'gain', 'floor', 'residual']
    assert _defaults(_hip.Handle.set_capon_clean) == dict(gain=0.5, floor=0.02, residual=False)
    assert list(inspect.signature(_hip.Handle.fetch_capon_clean).parameters) == ['self']
    assert list(inspect.signature(planner.check_capon_clean).parameters) == ['iterations', 'gain', 'floor', 'residual', 'has_capon']
    for f in (engine.launch, engine.process, engine.process_batch):
        p = inspect.signature(f).parameters
        assert 'capon_clean' in p and p['capon_clean'].default is None, f.__name__
    p = inspect.signature(engine.new_result).parameters
    assert p['clean_iterations'].default == 0 and p['want_clean_csdm'].default is False


def test_install_as_reference_modules_exports_the_new_functions():
    pkg.install_as_reference_modules()
    import lts_array as la
    import narrow_band_least_squares as nb
    assert la.ltsva_clean is pkg.ltsva_clean and la.ltsva_clean_batch is pkg.ltsva_clean_batch and la.clean_sources is pkg.clean_sources
    assert nb.narrow_band_least_squares_clean is pkg.narrow_band_least_squares_clean


def test_earlier_signatures_and_pinned_tails_are_unchanged():
    ref_args = list(inspect.signature(pkg.narrow_band_least_squares).parameters)
    assert list(inspect.signature(engine.launch).parameters)[-4:] == ['element_delays', 'element_delays_kept', 'beam_trace', 'beam_taps']
    assert list(inspect.signature(engine.process).parameters)[-4:] == ['element_max_shift', 'element_delays_kept', 'want_beam_trace',
                                                                       'beam_taps']
    assert list(inspect.signature(engine.process_batch).parameters)[-4:] == ['element_max_shift', 'element_delays_kept',
                                                                             'want_beam_trace', 'beam_taps']
    assert list(inspect.signature(engine.new_result).parameters)[:7] == ['nchans', 'alpha', 'fs', 'W', 'inc', 'nwin', 'vector_len']
    assert list(inspect.signature(pkg.ltsva).parameters) == LTSVA_ARGS + ['alpha', 'plot_array_coordinates', 'rij']
    assert list(inspect.signature(pkg.ltsva_capon).parameters) == LTSVA_ARGS + ['slowness_grid', 'freq', 'alpha', 'rij', 'snapshots',
                                                                                 'loading', 'maps', 'peaks', 'peak_floor']
    assert list(inspect.signature(pkg.ltsva_kept).parameters)[-2:] == ['peaks', 'peak_floor']
    assert list(inspect.signature(pkg.ltsva_batch).parameters)[-1] == 'slowness_grid'
    assert list(inspect.signature(pkg.narrow_band_least_squares_capon).parameters) == ref_args + [
        'slowness_grid', 'capon_freqs', 'snapshots', 'loading', 'maps', 'peaks', 'peak_floor']
    assert list(inspect.signature(_hip.Handle.set_capon).parameters) == ['self', 'grid', 'freqs', 'snap_len', 'snap_hop', 'loading',
                                                                         'want_maps', 'want_csdm']
    assert list(inspect.signature(planner.check_capon_peaks).parameters) == ['grid_len', 'cells', 'K', 'floor']


def test_header_binding_and_library_agree():
    header = open(os.path.join(ROOT, 'include', 'nbls.h'), encoding='utf-8').read()
    assert re.search(r'^int nbls_set_capon_clean\(nbls_handle\* h, int32_t iterations, double gain, double floor, int32_t flags\);', header, re.M)
    assert re.search(r'^int nbls_fetch_capon_clean\(nbls_handle\* h, int32_t\* count, int32_t\* index, double\* power, double\* total, '
                     r'double\* residual\);', header, re.M)
    assert re.search(r'^int nbls_fetch_capon_clean_csdm\(nbls_handle\* h, double\* R\);', header, re.M)
    assert re.search(r'^int nbls_capon_clean_lds_bytes\(int32_t nelem\);', header, re.M)
    assert re.search(r'^#define NBLS_CAPON_CLEAN_MAX %d$' % _hip.CAPON_CLEAN_MAX, header, re.M)
    assert re.search(r'^#define NBLS_CLEAN_RESIDUAL %d$' % _hip.CLEAN_RESIDUAL, header, re.M)
    assert planner.MAX_CAPON_CLEAN == _hip.CAPON_CLEAN_MAX == 32
    for phrase in ('i > 0 and p_i < f * p_0', 'vr = fma(Rr_jk, ar_k, vr)', 'q = fma(ar_j, vr_j, q)', 's = phi / q',
                   'wr = fma(vi_j, vi_k, vr_j * vr_k)', 'Re R_{i+1},jk = fma(-wr, s, Re R_i,jk)', 'power[i] = phi * p_i',
                   't_0 / N', 'zeros for the dropped ones'):
        assert phrase in header, phrase
    for s in SYMBOLS:
        assert s in _hip.EXPORTS
    lib = _hip.load_library()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert lib.nbls_set_capon_clean.argtypes == [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_int32]
    assert lib.nbls_fetch_capon_clean.argtypes == [C.c_void_p, ip, ip, dp, dp, dp]
    assert lib.nbls_fetch_capon_clean_csdm.argtypes == [C.c_void_p, dp]
    assert lib.nbls_capon_clean_lds_bytes.argtypes == [C.c_int32]
    out = subprocess.run(['nm', '-D', '--defined-only', _hip.LIB_PATH], capture_output=True, text=True).stdout
    assert set(SYMBOLS) <= set(re.findall(r'\b(nbls_[a-z0-9_]+)', out))
    # without a handle: argument errors, not crashes
    assert lib.nbls_set_capon_clean(None, 4, 0.5, 0.02, 0) == _hip.NBLS_ERR_ARG
    assert lib.nbls_fetch_capon_clean(None, None, None, None, None, None) == _hip.NBLS_ERR_ARG
    assert lib.nbls_fetch_capon_clean_csdm(None, None) == _hip.NBLS_ERR_ARG


def test_lds_bytes():
    """(2 N^2 + 2 N + 2 * 128 * N) * 8 bytes: R, v and a column of a per lane; less than capon_kernel's at every N."""
    f = _hip.load_library().nbls_capon_clean_lds_bytes
    for N, want in ((3, 6336), (8, 17536), (32, 82432)):
        assert f(N) == (2 * N * N + 2 * N + 2 * _hip.CAPON_THREADS * N) * 8 == want
    capon = lambda N: (4 * N * N + ((N + 1) & ~1) + max(_hip.CAPON_CHUNK, _hip.CAPON_THREADS) * N * 2) * 8
    for N in range(1, 33):
        assert 0 < f(N) < capon(N), N
    for bad in (0, -1, 33):
        assert f(bad) == _hip.NBLS_ERR_ARG


GOOD = dict(iterations=16, gain=0.5, floor=0.02, residual=False)
BAD = [dict(iterations=0), dict(iterations=33), dict(iterations=-1), dict(iterations=1.5), dict(iterations=True), dict(iterations='4'),
       dict(gain=0.0), dict(gain=1.0000001), dict(gain=-0.5), dict(gain=np.nan), dict(gain='x'), dict(gain=True),
       dict(floor=1.0), dict(floor=-1e-9), dict(floor=np.nan), dict(floor=None), dict(residual=1), dict(residual='yes'),
       dict(has_capon=False)]


@pytest.mark.parametrize('bad', BAD, ids=[','.join(b) + str(i) for i, b in enumerate(BAD)])
def test_check_capon_clean_refuses(bad):
    assert planner.check_capon_clean(**GOOD) == (16, 0.5, 0.02, False)
    with pytest.raises(ValueError):
        planner.check_capon_clean(**dict(GOOD, **bad))


def test_check_capon_clean_returns():
    assert planner.check_capon_clean(1, 1, 0, True) == (1, 1.0, 0.0, True)
    assert planner.check_capon_clean(np.int32(32), np.float32(0.25), 0.5) == (32, 0.25, 0.5, False)


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
    capon = dict(capon_grid=GRID, capon_freqs=[1.0], capon_snapshots=(16, 8))
    call = lambda **kw: engine.process(data, FS, 0.0, rij, [(None, None)], [65.5 / FS], 0.5, 1.0, prefiltered=True, **kw)
    for bad in ((0,), (33,), (4, 0.0), (4, 1.5), (4, 0.5, 1.0), (4, 0.5, -0.1), (4, 0.5, 0.02, 1), (4, 0.5, 0.02, False, 1), (), 2.5, 'x'):
        with pytest.raises(ValueError):
            call(capon_clean=bad, **capon)
        with pytest.raises(ValueError):
            engine.process_batch([list(data), list(data)], FS, [0.0, 1.0], rij, [(None, None)], [65.5 / FS], 0.5, 1.0, prefiltered=True,
                                 capon_clean=bad, **capon)
    with pytest.raises(ValueError, match='Capon'):                   # no spectra to work on
        call(capon_clean=(4, 0.5, 0.02, False))
    with pytest.raises(ValueError):                                  # what the spectra refuse stays refused
        call(capon_clean=4, **dict(capon, capon_snapshots=(66, 8)))
    args = (st, None, None, 65.5 / FS, 0.5, GRID, 1.0)
    for bad in (dict(iterations=0), dict(iterations=40), dict(gain=0), dict(gain=2), dict(floor=1), dict(floor=-1), dict(kept=1),
                dict(min_pairs=2), dict(kept=True, min_pairs=9), dict(max_sources=0), dict(max_sources=1.5), dict(merge_radius=-1.0),
                dict(merge_radius=np.nan), dict(snapshots=(0, 1))):
        with pytest.raises(ValueError):
            pkg.ltsva_clean(*args, rij=rij, **bad)
        with pytest.raises(ValueError):
            pkg.ltsva_clean_batch([st, st], *args[1:], rij=rij, **bad)
    with pytest.raises(ValueError):
        pkg.ltsva_clean(st, None, None, 65.5 / FS, 0.5, np.zeros((2, 3)), 1.0, rij=rij)
    fr = np.logspace(-1, 0.5, 16)
    nargs = ([10.0, 10.0], 0.5, 1.0, st, None, None, 2, np.zeros(16), np.zeros(16), np.array([0.5, 1.0, 2.0]), 'log', fr, 'butter', 2, 0.01)
    with pytest.raises(TypeError):                                   # the grid is a required keyword
        pkg.narrow_band_least_squares_clean(*nargs, rij=rij)
    for bad in (dict(slowness_grid=np.zeros((2, 3))), dict(iterations=0), dict(gain=0.0), dict(floor=1.0), dict(max_sources=0),
                dict(merge_radius='x'), dict(capon_freqs=[1.0]), dict(snapshots=(0, 1))):
        with pytest.raises(ValueError):
            pkg.narrow_band_least_squares_clean(*nargs, rij=rij, **dict(dict(slowness_grid=GRID), **bad))


def test_process_segmented_refuses(monkeypatch):
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', '1e-9')
    _no_gpu(monkeypatch)
    rij = synthetic.array_geometry(4, 1.0)
    data = np.random.default_rng(3).standard_normal((4, 1201))
    with pytest.raises(ValueError, match='time-segmented'):
        engine.process(data, FS, 0.0, rij, [(0.5, 2.0)], [65.5 / FS], 0.5, 1.0, 'butter', 2, 0.01, capon_grid=GRID, capon_freqs=[1.0],
                       capon_snapshots=(16, 8), capon_clean=4)


def test_new_result_fields():
    nwin = np.array([5, 3])
    res = engine.new_result(4, 1.0, FS, np.array([65, 33]), np.array([32, 16]), nwin, 6, capon_points=21, clean_iterations=7,
                            want_clean_csdm=True)
    assert res.clean_count.shape == (2, 6) and res.clean_count.dtype == np.int32
    assert res.clean_index.shape == (2, 6, 7) and res.clean_index.dtype == np.int32 and res.clean_power.shape == (2, 6, 7)
    assert res.clean_total.shape == res.clean_residual.shape == (2, 6)
    assert res.clean_csdm.shape == (2, 6, 4, 4) and res.clean_csdm.dtype == np.complex128
    res = engine.new_result(4, 1.0, FS, np.array([65, 33]), np.array([32, 16]), nwin, 6, capon_points=21)
    for k in engine.CLEAN_FIELDS + ('clean_csdm',):
        assert getattr(res, k) is None, k
    assert engine.new_result(4, 1.0, FS, np.array([65]), np.array([32]), nwin[:1], 6, clean_iterations=3).clean_count is None


def test_makefile_and_resource_report(tmp_path):
    """csrc/capon_clean.hip is built with capon.o's flags and listed for both libraries; both instances of its kernel have no
    private segment, spill no vector register and stay within 128 VGPRs (DESIGN.md section 24.2 records the counts)."""
    mk = open(os.path.join(LIBDIR, 'Makefile'), encoding='utf-8').read()
    assert 'capon_clean.o' in re.search(r'^OBJS = (.*)$', mk, re.M).group(1).split()
    assert 'capon_clean.hip' in re.search(r'^DEVSRC = (.*)$', mk, re.M).group(1).split()
    rule = re.search(r'^capon_clean\.o: (.*)\n\t(.*)$', mk, re.M)
    capon = re.search(r'^capon\.o: (.*)\n\t(.*)$', mk, re.M)
    assert rule and rule.group(2) == capon.group(2) and '$(NOFMA)' in rule.group(2)
    for dep in ('capon_clean.hip', 'capon_point.h', 'nbls_internal.h', 'dev_buf.h', '../../include/nbls.h'):
        assert dep in rule.group(1).split(), dep
    assert 'capon_point.h' in capon.group(1).split()
    assert 'capon_point.h' in re.search(r'^\$\(DEVLIB\): (.*)$', mk, re.M).group(1).split()
    hipcc = '/opt/rocm/bin/hipcc'                                        # (the compiler the Makefile names: no skip without it)
    out = tmp_path / 'capon_clean.s'
    subprocess.run([hipcc, '-O3', '-std=c++17', '--offload-arch=gfx950', '-I' + LIBDIR, '-S', '--cuda-device-only',
                    os.path.join(LIBDIR, 'capon_clean.hip'), '-o', str(out), '-ffp-contract=off'], check=True,
                   stderr=subprocess.DEVNULL, timeout=900)
    text = out.read_text()
    found = re.findall(r'\.amdhsa_kernel (\S*capon_clean_kernel\S*)(.*?)\.end_amdhsa_kernel', text, re.S)
    assert len(found) == 2, [n for n, _ in found]                        # plain and KEPT
    for name, body in found:
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0, name
        assert int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1)) <= 128, name
        assert int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1)) <= 1024, name
    for key in ('vgpr_spill_count', 'private_segment_fixed_size'):
        vals = re.findall(r'\.%s:\s+(\d+)' % key, text)
        assert len(vals) == 2 and all(int(v) == 0 for v in vals), (key, vals)
