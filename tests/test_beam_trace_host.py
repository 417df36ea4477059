"""What of the beam trace (``nbls_set_beam_trace``) a box without a GPU can check:
``planner.check_beam_trace``'s refusals, the new Python names and their argument checks, the two new symbols in the header,
the ctypes prototypes and the built library, the compiler's resource report of the two kernel instances, and the seam list
of tests/beam_trace_cases.py against the tile constants in csrc/beam_trace.hip."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import beam_trace_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, 'narrow_band_least_squares_amd', 'csrc')
SYMBOLS = ('nbls_set_beam_trace', 'nbls_fetch_beam_trace')


def test_check_beam_trace():
    from narrow_band_least_squares_amd import planner
    table, gate, kept = planner.check_beam_trace([16, 8])
    assert table.shape == (24,) and table.dtype == np.float64 and gate != gate and kept is False
    np.testing.assert_array_equal(table[:16], planner.beam_trace_window(16))
    np.testing.assert_array_equal(table[16:], planner.beam_trace_window(8))
    table, gate, kept = planner.check_beam_trace(np.array([4, 3]), 'boxcar', 0.6, True, has_kept=True)
    assert np.array_equal(table, np.ones(7)) and gate == 0.6 and kept is True
    assert planner.check_beam_trace([4], mdccm_min=float('nan'))[1] != planner.check_beam_trace([4], mdccm_min=float('nan'))[1]
    assert planner.check_beam_trace([4], mdccm_min=np.float64(0))[1] == 0.0
    own = planner.check_beam_trace([3, 2], [[0.0, 1.0, 0.0], [2.0, 0.5]])[0]            # the table itself, per band ...
    np.testing.assert_array_equal(own, [0.0, 1.0, 0.0, 2.0, 0.5])
    np.testing.assert_array_equal(planner.check_beam_trace([3, 2], own)[0], own)         # ... or flat
    for bad in (dict(window='hamming'), dict(window=np.ones(23)), dict(window=np.ones(25)),
                dict(window=np.r_[np.ones(16), np.zeros(8)]),                           # a band's table all zero
                dict(window=np.r_[np.ones(23), -1.0]), dict(window=np.r_[np.ones(23), np.nan]),
                dict(window=np.r_[np.ones(23), np.inf]), dict(window=7),
                dict(mdccm_min='0.5'), dict(mdccm_min=True), dict(kept=1), dict(kept=True),   # kept without a plan that names the elements
                dict(window_slice=(0, 2)), dict(estimators=[(0.5, [1])]), dict(comm=True)):
        with pytest.raises(ValueError):
            planner.check_beam_trace([16, 8], **bad)
    for W in ([], [0], [16, -1], [16.0], 16):
        with pytest.raises(ValueError):
            planner.check_beam_trace(W)


def test_python_names_and_signatures():
    import narrow_band_least_squares_amd as pkg
    from narrow_band_least_squares_amd import engine, planner, _hip
    for name in ('ltsva_beam_trace', 'ltsva_beam_trace_batch', 'narrow_band_least_squares_beam_trace'):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    sig = inspect.signature(pkg.ltsva_beam_trace).parameters
    assert list(sig) == ['st', 'lat_list', 'lon_list', 'window_length', 'window_overlap', 'alpha', 'rij', 'mdccm_min', 'window',
                         'kept', 'min_pairs']
    assert sig['alpha'].default == 1.0 and sig['mdccm_min'].default is None and sig['window'].default == 'hann'
    assert sig['kept'].default is False and sig['min_pairs'].default is None
    ref_args = list(inspect.signature(pkg.narrow_band_least_squares).parameters)
    sig = inspect.signature(pkg.narrow_band_least_squares_beam_trace).parameters
    assert list(sig) == ref_args + ['mdccm_min', 'window', 'kept']
    assert sig['mdccm_min'].default is None and sig['window'].default == 'hann' and sig['kept'].default is False
    sigb = inspect.signature(pkg.ltsva_beam_trace_batch).parameters
    assert list(sigb) == ['streams'] + list(inspect.signature(pkg.ltsva_beam_trace).parameters)[1:]
    assert all(sigb[k].default == v.default for k, v in inspect.signature(pkg.ltsva_beam_trace).parameters.items() if k != 'st')
    for f in (engine.process, engine.process_batch, engine.process_multi, engine.process_segmented):
        assert inspect.signature(f).parameters['want_beam_trace'].default is None
    assert inspect.signature(engine.launch).parameters['beam_trace'].default is None
    assert inspect.signature(engine.new_result).parameters['beam_trace_npts'].default == 0
    assert inspect.signature(engine.max_bands_per_pass).parameters['trace_rows'].default == 0
    assert callable(_hip.Handle.set_beam_trace) and callable(_hip.Handle.fetch_beam_trace) and _hip.BEAM_TRACE_KEPT == 1
    assert callable(planner.beam_trace_window) and callable(planner.check_beam_trace)
    # under the reference's module names too
    import sys
    saved = {k: sys.modules.get(k) for k in ('narrow_band_least_squares', 'helpers', 'lts_array')}
    try:
        pkg.install_as_reference_modules()
        import lts_array
        import narrow_band_least_squares as nb
        assert lts_array.ltsva_beam_trace is pkg.ltsva_beam_trace
        assert nb.narrow_band_least_squares_beam_trace is pkg.narrow_band_least_squares_beam_trace
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    # the functions that were there keep their signatures
    assert list(inspect.signature(pkg.ltsva).parameters) == ['st', 'lat_list', 'lon_list', 'window_length', 'window_overlap',
                                                              'alpha', 'plot_array_coordinates', 'rij']
    assert list(inspect.signature(pkg.ltsva_beam).parameters) == ['st', 'lat_list', 'lon_list', 'window_length', 'window_overlap',
                                                                   'alpha', 'rij']
    assert list(inspect.signature(pkg.ltsva_kept).parameters)[-2:] == ['peaks', 'peak_floor']
    assert list(inspect.signature(pkg.ltsva_batch).parameters)[-1] == 'slowness_grid'
    assert list(inspect.signature(pkg.ltsva_kept_batch).parameters)[-1] == 'peak_floor'


def test_new_result_and_the_band_budget(monkeypatch):
    from narrow_band_least_squares_amd import engine
    nwin = np.array([5, 3])
    res = engine.new_result(4, 0.5, 20.0, np.array([64, 64]), np.array([32, 32]), nwin, 8, beam_trace_npts=301)
    assert res.beam_trace.shape == (2, 301) and res.beam_trace.dtype == np.float64 and not res.beam_trace.any()
    assert engine.new_result(4, 0.5, 20.0, np.array([64, 64]), np.array([32, 32]), nwin, 8).beam_trace is None
    # the trace is one more row per band and recording beside the N filtered ones
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', repr(10 * 8.0 * 4 * (1000 + 64) / 2.0 ** 30))
    assert engine.max_bands_per_pass(4, 1000) == 10 and engine.max_bands_per_pass(4, 1000, 1) == 8
    assert engine.max_bands_per_pass(3 * 4, 1000, 3) == 2


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
    for bad in (dict(window='hamming'), dict(window=np.ones(7)), dict(mdccm_min='x'), dict(kept=1), dict(min_pairs=3),
                dict(kept=True, min_pairs=9), dict(alpha=0.3)):
        with pytest.raises(ValueError):
            pkg.ltsva_beam_trace(_stream(5), None, None, 10.0, 0.5, **dict(dict(alpha=0.5, rij=rij), **bad))
    with pytest.raises(ValueError):
        pkg.ltsva_beam_trace(_stream(3), None, None, 10.0, 0.5, alpha=0.5, rij=rij[:, :3])       # LTS needs four elements
        for streams in ([_stream(5), _stream(5)], [_stream(5)]):
            with pytest.raises(ValueError):
                pkg.ltsva_beam_trace_batch(streams, None, None, 10.0, 0.5, **dict(dict(alpha=0.5, rij=rij), **bad))
    assert pkg.ltsva_beam_trace_batch([], None, None, 10.0, 0.5) == []
    data = np.random.default_rng(3).standard_normal((5, 600))
    call = lambda **kw: engine.process(data, 20.0, 0.0, rij, [(None, None)], [10.0], 0.5, 0.5, prefiltered=True, **kw)
    for bad in (dict(want_beam_trace=dict(kept=True)),                       # the kept flag without kept=
                dict(want_beam_trace='hamming'), dict(want_beam_trace=dict(windows='hann')), dict(want_beam_trace=3),
                dict(want_beam_trace=True, window_slice=(0, 2))):
        with pytest.raises(ValueError):
            call(**bad)
    with pytest.raises(ValueError):
        engine.process_batch([list(data), list(data)], 20.0, [0.0, 1.0], rij, [(None, None)], [10.0], 0.5, 0.5, prefiltered=True,
                             want_beam_trace=dict(kept=True))
    with pytest.raises(ValueError, match='want_beam_trace'):
        engine.process_multi(data, 20.0, [0.0], [rij], [(None, None)], [10.0], 0.5, [(0.5, [])], prefiltered=True,
                             want_beam_trace=True)
    fr = np.logspace(-1, 0.5, 16)
    args = ([10.0, 10.0], 0.5, 0.5, _stream(5), None, None, 2, np.zeros(16), np.zeros(16), np.array([0.5, 1.0, 2.0]), 'log', fr,
            'butter', 2, 0.01)
    for bad in (dict(window='hamming'), dict(window=np.ones(200)), dict(mdccm_min='x'), dict(kept=0)):
        with pytest.raises(ValueError):
            pkg.narrow_band_least_squares_beam_trace(*args, rij=rij, **bad)
    with pytest.raises(TypeError):                                 # the new arguments are keyword-only
        pkg.narrow_band_least_squares_beam_trace(*args, rij, 0.5)


def test_the_time_segmented_path_refuses(monkeypatch):
    from narrow_band_least_squares_amd import engine
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', '1e-9')
    monkeypatch.setattr(engine, 'get_handle', lambda *a, **k: (_ for _ in ()).throw(AssertionError('the GPU was reached')))
    rij = np.array([[0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 1.0, 1.0]])
    data = np.random.default_rng(3).standard_normal((4, 1201))
    with pytest.raises(ValueError, match='want_beam_trace.*time-segmented'):
        engine.process(data, 20.0, 0.0, rij, [(0.5, 2.0)], [3.0], 0.5, 1.0, 'butter', 2, 0.01, want_beam_trace=True)


def test_header_binding_and_library_carry_the_symbols():
    from narrow_band_least_squares_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'nbls.h'), encoding='utf-8').read()
    for s in SYMBOLS:
        assert re.search(r'^int %s\(nbls_handle\* h,' % s, header, re.M), s
        assert s in _hip.EXPORTS
    assert re.search(r'^#define NBLS_BEAM_TRACE_KEPT 1$', header, re.M)
    lib = _hip.load_library()
    dp = C.POINTER(C.c_double)
    assert lib.nbls_set_beam_trace.argtypes == [C.c_void_p, dp, C.c_int64, C.c_double, C.c_int32]
    assert lib.nbls_fetch_beam_trace.argtypes == [C.c_void_p, C.c_int32, dp]
    out = subprocess.run(['nm', '-D', '--defined-only', os.path.join(LIBDIR, 'libnbls_hip.so')], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    exported = set(re.findall(r' T (nbls_[a-z0-9_]+)', out.stdout))
    assert set(SYMBOLS) <= exported
    # header and exports agree: every nbls_ function the library exports is declared in the header
    declared = set(re.findall(r'^[a-z][a-z0-9_ ]*\**\s*\**(nbls_[a-z0-9_]+)\(', header, re.M))
    assert exported <= declared, sorted(exported - declared)
    # the kernel is in the code object of the library (a missing kernel is an error, not a host loop)
    blob = open(os.path.join(LIBDIR, 'libnbls_hip.so'), 'rb').read()
    assert b'beam_trace_kernel' in blob


def test_the_calls_refuse_without_a_gpu_what_needs_none():
    from narrow_band_least_squares_amd import _hip
    lib = _hip.load_library()
    w = np.ones(4)
    assert lib.nbls_set_beam_trace(None, w.ctypes.data_as(C.POINTER(C.c_double)), 4, 0.5, 0) == _hip.NBLS_ERR_ARG
    assert lib.nbls_fetch_beam_trace(None, 0, w.ctypes.data_as(C.POINTER(C.c_double))) == _hip.NBLS_ERR_ARG


def test_new_instances_use_no_scratch_and_spill_nothing(tmp_path):
    """The compiler's resource report of beam_trace.hip: both instances without a private segment, without LDS."""
    hipcc = '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = tmp_path / 'beam_trace.s'
    subprocess.run([hipcc, '-O3', '-std=c++17', '--offload-arch=gfx950', '-I' + LIBDIR, '-S', '--cuda-device-only',
                    os.path.join(LIBDIR, 'beam_trace.hip'), '-o', str(out), '-ffp-contract=off'], check=True,
                   stderr=subprocess.DEVNULL, timeout=900)
    text = out.read_text()
    found = re.findall(r'\.amdhsa_kernel (\S*beam_trace_kernel\S*)(.*?)\.end_amdhsa_kernel', text, re.S)
    assert len(found) == 2, [n for n, _ in found]
    for name, body in found:
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0, name
        assert int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1)) == 0, name
    for key in ('vgpr_spill_count', 'private_segment_fixed_size'):
        vals = re.findall(r'\.%s:\s+(\d+)' % key, text)
        assert len(vals) == 2 and all(int(v) == 0 for v in vals), (key, vals)
    # no fused multiply-add of doubles outside the expansion of the one division per sample (v_div_scale ... v_div_fixup):
    # the file is built without contraction, as the Makefile says
    rest = re.sub(r'v_div_scale_f64.*?v_div_fixup_f64', '', text, flags=re.S)
    assert 'v_div_fixup_f64' in text and not re.search(r'v_fma_f64|v_fmac_f64', rest)
    mk = open(os.path.join(LIBDIR, 'Makefile'), encoding='utf-8').read()
    assert re.search(r'^beam_trace\.o:.*\n\t\$\(HIPCC\) \$\(CXXFLAGS\) \$\(NOFMA\) -c', mk, re.M)
    assert 'beam_trace.o' in re.search(r'^OBJS = (.*)$', mk, re.M).group(1) and 'beam_trace.hip' in re.search(r'^DEVSRC = (.*)$', mk, re.M).group(1)


def test_seam_list_is_held_to_the_kernels_tile():
    src = open(os.path.join(LIBDIR, 'beam_trace.hip'), encoding='utf-8').read()
    threads = int(re.search(r'constexpr int BT_THREADS = (\d+);', src).group(1))
    spt = int(re.search(r'constexpr int BT_SPT = (\d+);', src).group(1))
    assert re.search(r'constexpr int BT_TILE = BT_THREADS \* BT_SPT;', src)
    assert (threads, spt) == (cases.THREADS, cases.SPT) and cases.TILE == threads * spt and cases.WAVE_SPAN == 64 * spt
    assert re.search(r'__launch_bounds__\(BT_THREADS\)', src)
    T = cases.TILE
    Ws = {c[2] for c in cases.SEAMS}
    assert {16, 255, 256, 257, T - 1, T, T + 1} <= Ws and cases.WAVE_SPAN == 256
    npts = {c[4] for c in cases.SEAMS}
    assert any(n < T for n in npts) and any(n % T == T - 1 for n in npts) and any(n % T == 1 for n in npts)
    assert {0.0, 0.5, 0.75, 0.9} <= {c[3] for c in cases.SEAMS}
    labels = ' | '.join(c[0] for c in cases.SEAMS)
    for word in ('tail no window covers', 'straddles', 'fall off both ends'):
        assert word in labels, word
    from narrow_band_least_squares_amd import planner
    for label, N, W, overlap, n, scale in cases.SEAMS:
        Wp, inc, nwin = planner.window_plan(n, cases.FS, (W + 0.5) / cases.FS, overlap)[:3]
        assert int(Wp) == W and nwin >= 2, label
        if 'tail' in label:
            assert (nwin - 1) * inc + W < n - 16, label
        if 'straddles' in label:
            assert any(w * inc < T <= w * inc + W - 1 for w in range(nwin)), label
        if 'both ends' in label:
            D = cases.exact_geometry(N, scale)[2]
            assert D.min() < -8 and D.max() > 8 and (nwin - 1) * inc + W - 1 + D.max() >= n, label
    for N in cases.EXACT_N:
        rij, slow, D = cases.exact_geometry(N)
        assert rij.shape == (2, N) and np.abs(D).max() <= 3 and np.linalg.matrix_rank(planner.co_array(rij)[0]) == 2
