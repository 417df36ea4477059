"""What of the kept-element results (``nbls_set_kept_elements``) a box without a GPU can check:
``planner.check_kept``'s refusals, the new Python names and their argument checks, the two new symbols in the header, the
ctypes prototypes and the built library, and the compiler's resource report of the new kernel instances."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, 'narrow_band_least_squares_amd', 'csrc')
SYMBOLS = ('nbls_set_kept_elements', 'nbls_fetch_kept_elements')
GRID = np.array([[a, b] for a in (-1.0, 0.0, 1.0) for b in (-1.0, 0.0, 1.0)])


def test_check_kept():
    from narrow_band_least_squares_amd import planner
    assert planner.check_kept(8) == (7, True, False)                       # the default: every pair of the element
    assert planner.check_kept(8, None, False, True) == (7, False, True)
    assert planner.check_kept(8, 1) == (1, True, False) and planner.check_kept(8, 6, beam=False) == (6, False, False)
    assert planner.check_kept(32, np.int64(31), np.bool_(True), np.bool_(False)) == (31, True, False)
    assert planner.check_kept(3, 2) == (2, True, False)
    for bad in (dict(min_pairs=0), dict(min_pairs=-1), dict(min_pairs=8), dict(min_pairs=7.0), dict(min_pairs=True),
                dict(min_pairs='all'), dict(beam=1), dict(beam=None), dict(capon='yes'), dict(capon=0)):
        with pytest.raises(ValueError):
            planner.check_kept(8, **bad)
    for nchans in (2, 33, 0, -4, 8.0, True):
        with pytest.raises(ValueError):
            planner.check_kept(nchans)


def test_python_names_and_signatures():
    import narrow_band_least_squares_amd as pkg
    from narrow_band_least_squares_amd import engine, _hip
    for name in ('ltsva_kept', 'ltsva_kept_batch', 'narrow_band_least_squares_kept'):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    tail = ['min_pairs', 'beam', 'slowness_grid', 'freq', 'snapshots', 'loading', 'maps', 'peaks', 'peak_floor']
    sig = inspect.signature(pkg.ltsva_kept).parameters
    assert list(sig) == ['st', 'lat_list', 'lon_list', 'window_length', 'window_overlap', 'alpha', 'rij'] + tail
    assert sig['min_pairs'].default is None and sig['beam'].default is True and sig['slowness_grid'].default is None
    assert sig['peaks'].default == 0 and sig['peak_floor'].default == 0.25 and sig['loading'].default == 0.01
    sig = inspect.signature(pkg.ltsva_kept_batch).parameters
    assert list(sig) == ['streams', 'lat_list', 'lon_list', 'window_length', 'window_overlap', 'alpha', 'rij'] + tail
    ref_args = list(inspect.signature(pkg.narrow_band_least_squares).parameters)
    sig = inspect.signature(pkg.narrow_band_least_squares_kept).parameters
    assert list(sig) == ref_args + ['min_pairs', 'beam', 'slowness_grid', 'capon_freqs', 'snapshots', 'loading', 'maps', 'peaks',
                                    'peak_floor']
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(sig)[len(ref_args):])
    for f in (engine.process, engine.process_batch, engine.launch):
        assert inspect.signature(f).parameters['kept'].default is None
    assert inspect.signature(engine.new_result).parameters['want_kept'].default is False
    assert callable(_hip.Handle.set_kept_elements) and callable(_hip.Handle.fetch_kept_elements)
    assert (_hip.KEPT_BEAM, _hip.KEPT_CAPON) == (1, 2)
    # the functions that were there keep their signatures
    assert list(inspect.signature(pkg.ltsva).parameters) == ['st', 'lat_list', 'lon_list', 'window_length', 'window_overlap',
                                                              'alpha', 'plot_array_coordinates', 'rij']
    assert list(inspect.signature(pkg.ltsva_beam).parameters) == ['st', 'lat_list', 'lon_list', 'window_length', 'window_overlap',
                                                                   'alpha', 'rij']
    assert list(inspect.signature(pkg.ltsva_capon).parameters)[-2:] == ['peaks', 'peak_floor']


def test_new_result_carries_the_two_arrays_only_when_asked():
    from narrow_band_least_squares_amd import engine
    nwin = np.array([5, 3])
    res = engine.new_result(4, 0.5, 20.0, np.array([64, 64]), np.array([32, 32]), nwin, 8, want_kept=True)
    assert res.dropped_mask.shape == res.kept_count.shape == (2, 8)
    assert res.dropped_mask.dtype == np.uint32 and res.kept_count.dtype == np.int32 and not res.dropped_mask.any()
    res = engine.new_result(4, 0.5, 20.0, np.array([64, 64]), np.array([32, 32]), nwin, 8)
    assert res.dropped_mask is None and res.kept_count is None


def test_returns_kept_unpacks_the_mask():
    from narrow_band_least_squares_amd import engine, lts_array
    res = engine.new_result(5, 0.5, 20.0, np.array([64]), np.array([32]), np.array([3]), 4, want_beam=True, want_kept=True)
    res.dropped_mask[0, :3] = [0, 1 << 4, (1 << 0) | (1 << 2)]
    res.kept_count[0, :3] = [5, 4, 3]
    out = lts_array._returns_kept(res, 5, True, {}, n=3)
    assert out['dropped_elements'].dtype == bool and out['dropped_elements'].shape == (3, 5)
    assert out['dropped_elements'].tolist() == [[False] * 5, [False] * 4 + [True], [True, False, True, False, False]]
    assert out['kept_count'].tolist() == [5, 4, 3] and out['fstat'].shape == (3,) and 'capon_index' not in out


def _stream(nchans, npts=600, fs=20.0):
    from narrow_band_least_squares_amd import synthetic
    return synthetic.make_stream(np.random.default_rng(4).standard_normal((nchans, npts)), fs)


def test_bad_arguments_raise_before_any_gpu_work(monkeypatch):
    import narrow_band_least_squares_amd as pkg
    from narrow_band_least_squares_amd import engine

    def no_gpu(*a, **k):
        raise AssertionError('the GPU was reached')
    monkeypatch.setattr(engine, 'get_handle', no_gpu)
    rij = np.array([[0.0, 1.0, 0.0, 1.0, 0.5], [0.0, 0.0, 1.0, 1.0, 0.3]])
    for bad in (dict(min_pairs=0), dict(min_pairs=5), dict(min_pairs=2.5), dict(beam='yes'), dict(freq=1.0), dict(maps=True),
                dict(peaks=2), dict(slowness_grid=GRID), dict(slowness_grid=GRID, freq=1.0, peaks=9),
                dict(slowness_grid=GRID, freq=-1.0), dict(slowness_grid=GRID, freq=1.0, maps='no'), dict(alpha=0.3)):
        with pytest.raises(ValueError):
            pkg.ltsva_kept(_stream(5), None, None, 10.0, 0.5, **dict(dict(alpha=0.5, rij=rij), **bad))
        with pytest.raises(ValueError):
            pkg.ltsva_kept_batch([_stream(5), _stream(5)], None, None, 10.0, 0.5, **dict(dict(alpha=0.5, rij=rij), **bad))
    with pytest.raises(ValueError):
        pkg.ltsva_kept(_stream(3), None, None, 10.0, 0.5, alpha=0.5, rij=rij[:, :3])             # LTS needs four elements
    assert pkg.ltsva_kept_batch([], None, None, 10.0, 0.5) == []
    data = np.random.default_rng(3).standard_normal((5, 600))
    call = lambda **kw: engine.process(data, 20.0, 0.0, rij, [(None, None)], [10.0], 0.5, 0.5, prefiltered=True, **kw)
    for bad in (dict(kept=(4, True, False)),                                                   # the beam flag without want_beam
                dict(kept=(4, False, True)),                                                   # the Capon flag without capon_grid
                dict(kept=(5, False, False)), dict(kept=(4, False)), dict(kept=7), dict(kept=(4, 1, False), want_beam=True)):
        with pytest.raises(ValueError):
            call(**bad)
    with pytest.raises(ValueError):
        engine.process_batch([list(data), list(data)], 20.0, [0.0, 1.0], rij, [(None, None)], [10.0], 0.5, 0.5, prefiltered=True,
                             kept=(4, True, False))
    fr = np.logspace(-1, 0.5, 16)
    args = ([10.0, 10.0], 0.5, 0.5, _stream(5), None, None, 2, np.zeros(16), np.zeros(16), np.array([0.5, 1.0, 2.0]), 'log', fr,
            'butter', 2, 0.01)
    for bad in (dict(min_pairs=9), dict(beam=0), dict(maps=True), dict(peaks=1), dict(slowness_grid=GRID, peaks=11)):
        with pytest.raises(ValueError):
            pkg.narrow_band_least_squares_kept(*args, rij=rij, **bad)
    with pytest.raises(TypeError):                                 # the new arguments are keyword-only
        pkg.narrow_band_least_squares_kept(*args, rij, 4)


def test_the_time_segmented_path_refuses(monkeypatch):
    from narrow_band_least_squares_amd import engine
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', '1e-9')
    monkeypatch.setattr(engine, 'get_handle', lambda *a, **k: (_ for _ in ()).throw(AssertionError('the GPU was reached')))
    rij = np.array([[0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 1.0, 1.0]])
    data = np.random.default_rng(3).standard_normal((4, 1201))
    with pytest.raises(ValueError, match='time-segmented'):
        engine.process(data, 20.0, 0.0, rij, [(0.5, 2.0)], [3.0], 0.5, 0.5, 'butter', 2, 0.01, want_beam=True, kept=(3, True, False))


def test_header_binding_and_library_carry_the_symbols():
    from narrow_band_least_squares_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'nbls.h'), encoding='utf-8').read()
    for s in SYMBOLS:
        assert re.search(r'^int %s\(nbls_handle\* h,' % s, header, re.M), s
        assert s in _hip.EXPORTS
    assert re.search(r'^#define NBLS_KEPT_BEAM 1$', header, re.M) and re.search(r'^#define NBLS_KEPT_CAPON 2$', header, re.M)
    lib = _hip.load_library()
    assert lib.nbls_set_kept_elements.argtypes == [C.c_void_p, C.c_int32, C.c_int32]
    assert lib.nbls_fetch_kept_elements.argtypes == [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]
    out = subprocess.run(['nm', '-D', '--defined-only', os.path.join(LIBDIR, 'libnbls_hip.so')], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    assert set(SYMBOLS) <= set(re.findall(r' T (nbls_[a-z0-9_]+)', out.stdout))
    # the kernels are in the code object of the library (a missing kernel is an error, not a host loop)
    blob = open(os.path.join(LIBDIR, 'libnbls_hip.so'), 'rb').read()
    assert b'kept_elements_kernel' in blob


def test_the_setter_refuses_without_a_gpu_what_needs_none():
    """``nbls_set_kept_elements`` checks its arguments before it touches the handle: a NULL handle is an argument error."""
    from narrow_band_least_squares_amd import _hip
    lib = _hip.load_library()
    assert lib.nbls_set_kept_elements(None, 1, 0) == _hip.NBLS_ERR_ARG
    assert lib.nbls_fetch_kept_elements(None, None, None) == _hip.NBLS_ERR_ARG


def test_new_instances_use_no_scratch_and_spill_nothing(tmp_path):
    """The compiler's resource report of kept.hip, beam.hip and capon.hip: every instance, the KEPT ones included, without a
    private segment — the gather of a steering row through the index list has not turned y into scratch."""
    hipcc = '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    want = {'kept.hip': ('kept_elements_kernel', 3, []), 'beam.hip': ('beam_fstat_kernel', 2, ['-ffp-contract=off']),
            'capon.hip': ('capon_kernel', 6, ['-ffp-contract=off'])}
    for src, (kernel, count, flags) in want.items():
        out = tmp_path / (src + '.s')
        subprocess.run([hipcc, '-O3', '-std=c++17', '--offload-arch=gfx950', '-I' + LIBDIR, '-S', '--cuda-device-only',
                        os.path.join(LIBDIR, src), '-o', str(out)] + flags, check=True, stderr=subprocess.DEVNULL, timeout=900)
        text = out.read_text()
        found = re.findall(r'\.amdhsa_kernel (\S*%s\S*)(.*?)\.end_amdhsa_kernel' % kernel, text, re.S)
        assert len(found) == count, [n for n, _ in found]
        for name, body in found:
            assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0, name
        # (a scalar register parked in a vector lane is no scratch: the HBM-route KEPT instance of capon_kernel has one)
        for key in ('vgpr_spill_count', 'private_segment_fixed_size'):
            vals = re.findall(r'\.%s:\s+(\d+)' % key, text)
            assert len(vals) == count and all(int(v) == 0 for v in vals), (src, key, vals)
