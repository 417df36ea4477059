"""Host side of the eigenvalues and the MUSIC spectrum (``nbls_set_capon_music``): names, signatures and
defaults of everything new, every earlier signature as it was, the header's declarations and their bindings, every
``ValueError`` before any GPU call, the LDS formula, the Makefile's lines and the compiler's resource report.  CPU only."""
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
SYMBOLS = ['nbls_set_capon_music', 'nbls_fetch_capon_music', 'nbls_fetch_capon_music_map', 'nbls_fetch_capon_music_vectors',
           'nbls_fetch_capon_music_peaks', 'nbls_capon_music_lds_bytes']
FS = 20.0
GRID = planner.slowness_grid(3.0, 5)
LTSVA_ARGS = ['st', 'lat_list', 'lon_list', 'window_length', 'window_overlap']


def _defaults(f):
    return {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}


def test_public_names_signatures_and_defaults():
    for name in ('ltsva_music', 'ltsva_music_batch', 'narrow_band_least_squares_music'):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    tail = ['slowness_grid', 'freq', 'alpha', 'rij', 'snapshots', 'sources', 'eig_floor', 'maps', 'vectors', 'peaks', 'peak_floor']
    assert list(inspect.signature(pkg.ltsva_music).parameters) == LTSVA_ARGS + tail
    assert list(inspect.signature(pkg.ltsva_music_batch).parameters) == ['streams'] + LTSVA_ARGS[1:] + tail
    want = dict(alpha=1.0, rij=None, snapshots=None, sources=0, eig_floor=0.05, maps=False, vectors=False, peaks=0, peak_floor=0.0)
    assert _defaults(pkg.ltsva_music) == want and _defaults(pkg.ltsva_music_batch) == want
    ref_args = list(inspect.signature(pkg.narrow_band_least_squares).parameters)
    sig = inspect.signature(pkg.narrow_band_least_squares_music)
    assert list(sig.parameters) == ref_args + ['slowness_grid', 'capon_freqs', 'snapshots', 'sources', 'eig_floor', 'maps', 'vectors',
                                               'peaks', 'peak_floor']
    for k in list(sig.parameters)[len(ref_args):]:
        assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert sig.parameters['slowness_grid'].default is inspect.Parameter.empty
    assert (sig.parameters['sources'].default, sig.parameters['eig_floor'].default) == (0, 0.05)
    assert (sig.parameters['peaks'].default, sig.parameters['peak_floor'].default) == (0, 0.0)
    assert list(inspect.signature(_hip.Handle.set_capon_music).parameters) == ['self', 'sources', 'eig_floor', 'maps', 'vectors', 'peaks',
                                                                               'peak_floor']
    assert _defaults(_hip.Handle.set_capon_music) == dict(sources=0, eig_floor=0.05, maps=False, vectors=False, peaks=False, peak_floor=0.0)
    assert list(inspect.signature(_hip.Handle.fetch_capon_music).parameters) == ['self']
    assert list(inspect.signature(_hip.Handle.fetch_capon_music_peaks).parameters) == ['self']
    assert list(inspect.signature(_hip.Handle.fetch_capon_peaks).parameters) == ['self', 'which']
    assert list(inspect.signature(planner.check_capon_music).parameters) == ['nchans', 'sources', 'eig_floor', 'maps', 'vectors', 'peaks',
                                                                             'peak_floor', 'has_capon', 'has_peaks', 'kept_capon',
                                                                             'estimators', 'comm', 'segmented']
    for f in (engine.launch, engine.process, engine.process_batch):
        p = inspect.signature(f).parameters
        assert 'capon_music' in p and p['capon_music'].default is None, f.__name__
    p = inspect.signature(engine.new_result).parameters
    for k in ('want_music', 'want_music_maps', 'want_music_vectors', 'want_music_peaks'):
        assert p[k].default is False, k


def test_install_as_reference_modules_exports_the_new_functions():
    pkg.install_as_reference_modules()
    import lts_array as la
    import narrow_band_least_squares as nb
    assert la.ltsva_music is pkg.ltsva_music and la.ltsva_music_batch is pkg.ltsva_music_batch
    assert nb.narrow_band_least_squares_music is pkg.narrow_band_least_squares_music


def test_earlier_signatures_and_pinned_tails_are_unchanged():
    assert list(inspect.signature(engine.launch).parameters)[-4:] == ['element_delays', 'element_delays_kept', 'beam_trace', 'beam_taps']
    assert list(inspect.signature(engine.process).parameters)[-4:] == ['element_max_shift', 'element_delays_kept', 'want_beam_trace',
                                                                       'beam_taps']
    assert list(inspect.signature(engine.process_batch).parameters)[-4:] == ['element_max_shift', 'element_delays_kept',
                                                                             'want_beam_trace', 'beam_taps']
    assert list(inspect.signature(engine.new_result).parameters)[-6:-4] == ['clean_iterations', 'want_clean_csdm']
    assert list(inspect.signature(pkg.ltsva_clean).parameters)[-4:] == ['kept', 'min_pairs', 'merge_radius', 'max_sources']
    assert list(inspect.signature(_hip.Handle.set_capon_clean).parameters) == ['self', 'iterations', 'gain', 'floor', 'residual']
    assert list(inspect.signature(planner.check_capon_clean).parameters) == ['iterations', 'gain', 'floor', 'residual', 'has_capon']


def test_header_binding_and_library_agree():
    header = open(os.path.join(ROOT, 'include', 'nbls.h'), encoding='utf-8').read()
    assert re.search(r'^int nbls_set_capon_music\(nbls_handle\* h, int32_t sources, double eig_floor, double peak_floor, int32_t flags\);',
                     header, re.M)
    assert re.search(r'^int nbls_fetch_capon_music\(nbls_handle\* h, double\* eigenvalues, int32_t\* sources, int32_t\* sweeps, '
                     r'int32_t\* index, double\* power\);', header, re.M)
    assert re.search(r'^int nbls_fetch_capon_music_map\(nbls_handle\* h, double\* map\);', header, re.M)
    assert re.search(r'^int nbls_fetch_capon_music_vectors\(nbls_handle\* h, double\* E\);', header, re.M)
    assert re.search(r'^int nbls_fetch_capon_music_peaks\(nbls_handle\* h, int32_t\* count, int32_t\* index, double\* power, double\* offset\);',
                     header, re.M)
    assert re.search(r'^int nbls_fetch_capon_peaks\(nbls_handle\* h, int32_t which /\* 0 Capon, 1 Bartlett \*/,', header, re.M)
    assert re.search(r'^int nbls_capon_music_lds_bytes\(int32_t nelem\);', header, re.M)
    assert re.search(r'^#define NBLS_MUSIC_PEAKS %d$' % _hip.MUSIC_PEAKS, header, re.M)
    assert re.search(r'^#define NBLS_MUSIC_SWEEP_CAP %d$' % _hip.MUSIC_SWEEP_CAP, header, re.M)
    assert re.search(r'^#define NBLS_MUSIC_MAP %d$' % _hip.MUSIC_MAP, header, re.M)
    assert re.search(r'^#define NBLS_MUSIC_VECTORS %d$' % _hip.MUSIC_VECTORS, header, re.M)
    assert re.search(r'^#define NBLS_MUSIC_STOP_SQUARED 0x1p-92$', header, re.M)
    for phrase in ('t = sign(tau) / (|tau| + sqrt(fma(tau, tau, 1)))', 'tau = (A_qq - A_pp) / (2 g)', 'off(A) <= 2^-46 ||R||_F',
                   'value descending, then the', 'clamp(#{k : lambda_k >= rho * lambda_1}, 1, N - 1)', 'D = 0 gives +inf',
                   'zi = fma(-Im e_ik, Re a_i, zi)', 'P(g) = 1 / (d / N)', '{(k + r) mod m, (k - r) mod m}'):
        assert phrase in header, phrase
    for s in SYMBOLS:
        assert s in _hip.EXPORTS
    lib = _hip.load_library()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert lib.nbls_set_capon_music.argtypes == [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_int32]
    assert lib.nbls_fetch_capon_music.argtypes == [C.c_void_p, dp, ip, ip, ip, dp]
    assert lib.nbls_fetch_capon_music_map.argtypes == [C.c_void_p, dp]
    assert lib.nbls_fetch_capon_music_vectors.argtypes == [C.c_void_p, dp]
    assert lib.nbls_fetch_capon_music_peaks.argtypes == [C.c_void_p, ip, ip, dp, dp]
    assert lib.nbls_capon_music_lds_bytes.argtypes == [C.c_int32]
    out = subprocess.run(['nm', '-D', '--defined-only', _hip.LIB_PATH], capture_output=True, text=True).stdout
    assert set(SYMBOLS) <= set(re.findall(r'\b(nbls_[a-z0-9_]+)', out))
    # without a handle: argument errors, not crashes
    assert lib.nbls_set_capon_music(None, 2, 0.05, 0.0, 0) == _hip.NBLS_ERR_ARG
    assert lib.nbls_fetch_capon_music(None, None, None, None, None, None) == _hip.NBLS_ERR_ARG
    assert lib.nbls_fetch_capon_music_map(None, None) == _hip.NBLS_ERR_ARG
    assert lib.nbls_fetch_capon_music_vectors(None, None) == _hip.NBLS_ERR_ARG
    assert lib.nbls_fetch_capon_music_peaks(None, None, None, None, None) == _hip.NBLS_ERR_ARG


def test_lds_bytes():
    """(4 N^2 + 2 * 128 * N + 4 N + 4) * 8 bytes: A, E, a column of a per lane, the rotations, the eigenvalues and their order;
    within a workgroup's 160 KiB at every N."""
    f = _hip.load_library().nbls_capon_music_lds_bytes
    for N, want in ((3, 6560), (8, 18720), (32, 99360)):
        assert f(N) == (4 * N * N + 2 * _hip.CAPON_THREADS * N + 4 * N + 4) * 8 == want
    for N in range(3, 33):
        assert 0 < f(N) <= 160 * 1024 - 1024, N
    for bad in (0, -1, 2, 33):
        assert f(bad) == _hip.NBLS_ERR_ARG


GOOD = dict(nchans=8, sources=0, eig_floor=0.05, maps=False, vectors=False, peaks=True, peak_floor=0.0)
BAD = [dict(nchans=2), dict(nchans=33), dict(nchans=8.0), dict(nchans=True), dict(sources=-1), dict(sources=8), dict(sources=1.5),
       dict(sources=True), dict(sources='2'), dict(sources=None), dict(eig_floor=0.0), dict(eig_floor=1.0), dict(eig_floor=-0.1),
       dict(eig_floor=np.nan), dict(eig_floor='x'), dict(eig_floor=None), dict(maps=1), dict(maps='yes'), dict(vectors=0),
       dict(vectors=None), dict(peaks=1), dict(peaks='K'), dict(peak_floor=1.0), dict(peak_floor=-0.1), dict(peak_floor=np.nan),
       dict(peak_floor=None), dict(has_peaks=False), dict(has_capon=False), dict(kept_capon=True), dict(estimators=True), dict(comm=True), dict(segmented=True)]


@pytest.mark.parametrize('bad', BAD, ids=[','.join(b) + str(i) for i, b in enumerate(BAD)])
def test_check_capon_music_refuses(bad):
    assert planner.check_capon_music(**GOOD) == (0, 0.05, False, False, True, 0.0)
    with pytest.raises(ValueError):
        planner.check_capon_music(**dict(GOOD, **bad))


def test_check_capon_music_returns():
    assert planner.check_capon_music(8, 7, 0.5, True, True) == (7, 0.5, True, True, False, 0.0)
    assert planner.check_capon_music(np.int64(3), np.int32(2), 7.0) == (2, 7.0, False, False, False, 0.0)     # a fixed M does not read the floor
    assert planner.check_capon_music(32, 31, peaks=True, peak_floor=0.5) == (31, 0.05, False, False, True, 0.5)
    assert planner.check_capon_music(8, 2, has_peaks=False) == (2, 0.05, False, False, False, 0.0)        # no peaks asked: none needed


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
    for bad in ((-1,), (4,), (0, 0.0), (0, 1.0), (1.5,), (2, 0.05, 1), (2, 0.05, False, 'x'), (2, 0.05, False, False, 1), (2, 0.05, False, False, True),
                (2, 0.05, False, False, False, 1.0), (2, 0.05, False, False, False, 0.0, 1), (), 2.5, 'x'):
        with pytest.raises(ValueError):
            call(capon_music=bad, **capon)
        with pytest.raises(ValueError):
            engine.process_batch([list(data), list(data)], FS, [0.0, 1.0], rij, [(None, None)], [65.5 / FS], 0.5, 1.0, prefiltered=True,
                                 capon_music=bad, **capon)
    with pytest.raises(ValueError, match='Capon'):                   # no spectra to work on
        call(capon_music=(2, 0.05, False, False))
    with pytest.raises(ValueError, match='full array'):              # the spectra of the kept elements
        call(capon_music=2, kept=(1, False, True), **capon)
    with pytest.raises(ValueError):                                  # what the spectra refuse stays refused
        call(capon_music=2, **dict(capon, capon_snapshots=(66, 8)))
    args = (st, None, None, 65.5 / FS, 0.5, GRID, 1.0)
    for bad in (dict(sources=-1), dict(sources=4), dict(sources=2.0), dict(eig_floor=0), dict(eig_floor=1), dict(maps=1),
                dict(vectors='x'), dict(peaks=9), dict(peaks=-1), dict(peaks=2, peak_floor=1.0), dict(peak_floor='x'),
                dict(snapshots=(0, 1))):
        with pytest.raises(ValueError):
            pkg.ltsva_music(*args, rij=rij, **bad)
        with pytest.raises(ValueError):
            pkg.ltsva_music_batch([st, st], *args[1:], rij=rij, **bad)
    with pytest.raises(ValueError):
        pkg.ltsva_music(st, None, None, 65.5 / FS, 0.5, np.zeros((2, 3)), 1.0, rij=rij)
    fr = np.logspace(-1, 0.5, 16)
    nargs = ([10.0, 10.0], 0.5, 1.0, st, None, None, 2, np.zeros(16), np.zeros(16), np.array([0.5, 1.0, 2.0]), 'log', fr, 'butter', 2, 0.01)
    with pytest.raises(TypeError):                                   # the grid is a required keyword
        pkg.narrow_band_least_squares_music(*nargs, rij=rij)
    for bad in (dict(slowness_grid=np.zeros((2, 3))), dict(sources=4), dict(sources=-1), dict(eig_floor=0.0), dict(maps=1),
                dict(vectors=2), dict(peaks=9), dict(peak_floor=1.0), dict(capon_freqs=[1.0]), dict(snapshots=(0, 1))):
        with pytest.raises(ValueError):
            pkg.narrow_band_least_squares_music(*nargs, rij=rij, **dict(dict(slowness_grid=GRID), **bad))


def test_process_segmented_refuses(monkeypatch):
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', '1e-9')
    _no_gpu(monkeypatch)
    rij = synthetic.array_geometry(4, 1.0)
    data = np.random.default_rng(3).standard_normal((4, 1201))
    with pytest.raises(ValueError, match='time-segmented'):
        engine.process(data, FS, 0.0, rij, [(0.5, 2.0)], [65.5 / FS], 0.5, 1.0, 'butter', 2, 0.01, capon_grid=GRID, capon_freqs=[1.0],
                       capon_snapshots=(16, 8), capon_music=2)


def test_new_result_fields():
    nwin = np.array([5, 3])
    res = engine.new_result(4, 1.0, FS, np.array([65, 33]), np.array([32, 16]), nwin, 6, capon_points=21, want_music=True,
                            want_music_maps=True, want_music_vectors=True)
    assert res.music_eigenvalues.shape == (2, 6, 4) and res.music_power.shape == (2, 6)
    for k in ('music_sources', 'music_sweeps', 'music_index'):
        assert getattr(res, k).shape == (2, 6) and getattr(res, k).dtype == np.int32
    assert res.music_map.shape == (2, 6, 21)
    assert res.music_vectors.shape == (2, 6, 4, 4) and res.music_vectors.dtype == np.complex128
    assert res.music_peak_count is None
    res = engine.new_result(4, 1.0, FS, np.array([65, 33]), np.array([32, 16]), nwin, 6, capon_points=21, capon_peaks=3, want_music=True,
                            want_music_peaks=True)
    assert res.music_peak_count.shape == (2, 6) and res.music_peak_index.shape == (2, 6, 3) and res.music_peak_offset.shape == (2, 6, 3, 2)
    assert res.music_peak_index.dtype == np.int32 and res.capon_peak_power.shape == res.music_peak_power.shape
    res = engine.new_result(4, 1.0, FS, np.array([65, 33]), np.array([32, 16]), nwin, 6, capon_points=21, want_music=True)
    assert res.music_map is None and res.music_vectors is None and res.music_eigenvalues is not None
    res = engine.new_result(4, 1.0, FS, np.array([65, 33]), np.array([32, 16]), nwin, 6, capon_points=21)
    for k in engine.MUSIC_FIELDS + ('music_map', 'music_vectors', 'music_peak_count', 'music_peak_offset'):
        assert getattr(res, k) is None, k
    assert engine.new_result(4, 1.0, FS, np.array([65]), np.array([32]), nwin[:1], 6, want_music=True).music_eigenvalues is None


def test_makefile_and_resource_report(tmp_path):
    """csrc/capon_music.hip is built with capon.o's flags and listed for both libraries; its kernel has no private segment,
    spills no vector register and stays within 128 VGPRs (DESIGN.md section 25.2 records the counts)."""
    mk = open(os.path.join(LIBDIR, 'Makefile'), encoding='utf-8').read()
    assert 'capon_music.o' in re.search(r'^OBJS = (.*)$', mk, re.M).group(1).split()
    assert 'capon_music.hip' in re.search(r'^DEVSRC = (.*)$', mk, re.M).group(1).split()
    rule = re.search(r'^capon_music\.o: (.*)\n\t(.*)$', mk, re.M)
    capon = re.search(r'^capon\.o: (.*)\n\t(.*)$', mk, re.M)
    assert rule and rule.group(2) == capon.group(2) and '$(NOFMA)' in rule.group(2)
    for dep in ('capon_music.hip', 'capon_point.h', 'capon_peaks.h', 'nbls_internal.h', 'dev_buf.h', '../../include/nbls.h'):
        assert dep in rule.group(1).split(), dep
    assert 'capon_peaks.h' in capon.group(1).split()
    assert 'capon_peaks.h' in re.search(r'^\$\(DEVLIB\): (.*)$', mk, re.M).group(1).split()
    hipcc = '/opt/rocm/bin/hipcc'                                        # (the compiler the Makefile names: no skip without it)
    out = tmp_path / 'capon_music.s'
    subprocess.run([hipcc, '-O3', '-std=c++17', '--offload-arch=gfx950', '-I' + LIBDIR, '-S', '--cuda-device-only',
                    os.path.join(LIBDIR, 'capon_music.hip'), '-o', str(out), '-ffp-contract=off'], check=True,
                   stderr=subprocess.DEVNULL, timeout=900)
    text = out.read_text()
    found = re.findall(r'\.amdhsa_kernel (\S*capon_music_kernel\S*)(.*?)\.end_amdhsa_kernel', text, re.S)
    assert len(found) == 2, [n for n, _ in found]                        # plain and with peaks
    for name, body in found:
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0, name
        assert int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1)) <= 128, name
        assert int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1)) <= 1024, name
    for key in ('vgpr_spill_count', 'private_segment_fixed_size'):
        vals = re.findall(r'\.%s:\s+(\d+)' % key, text)
        assert len(vals) == 2 and all(int(v) == 0 for v in vals), (key, vals)
