"""What of the closure results (``nbls_set_closure``) a box without a GPU can check: the new Python
names and their argument checks, the three new symbols in the header, the ctypes binding and the built library, the
defining lines shared by the header and DESIGN.md, a plain-C caller that compiles and links, and the compiler's resource
report of the kernel."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, 'tests', 'c_caller')
LIBDIR = os.path.join(ROOT, 'narrow_band_least_squares_amd', 'csrc')
SYMBOLS = ('nbls_set_closure', 'nbls_fetch_closure', 'nbls_est_fetch_closure')
DEFINITION = (
    't_ij     plan without lag refinement:  t_ij = lag[k(i,j)]                     (int32, exactly the lag of nbls_fetch / nbls_est_fetch)',
    '         plan with lag refinement:     t_ij = (double)lag[k(i,j)] + frac[k(i,j)]   (the sum every other site forms, un-fused double)',
    'closure  c_ijk = (t_ij + t_jk) − t_ik           for i < j < k;  T = N (N−1)(N−2) / 6 triplets',
    'sums     Q = Σ_{i<j<k} c_ijk²,   E_m = Σ_{triplets that contain element m} c_ijk²,   T_m = (N−1)(N−2) / 2',
    'outputs  consistency            = sqrt(Q / T) / fs                          seconds, [rows][VL]',
    '         closure_max            = max_{i<j<k} |c_ijk| / fs                  seconds, [rows][VL]',
    '         element_consistency[m] = sqrt(E_m / T_m) / fs                      seconds, [rows][VL][N]',
)


def test_python_names_and_signatures():
    import narrow_band_least_squares_amd as pkg
    from narrow_band_least_squares_amd import engine, _hip
    for name in ('ltsva_consistency', 'narrow_band_least_squares_consistency'):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    sig = inspect.signature(pkg.ltsva_consistency).parameters
    assert list(sig) == ['st', 'lat_list', 'lon_list', 'window_length', 'window_overlap', 'alpha', 'rij', 'subsample']
    assert sig['alpha'].default == 1.0 and sig['rij'].default is None and sig['subsample'].default is False
    ref_args = list(inspect.signature(pkg.narrow_band_least_squares).parameters)
    sig = inspect.signature(pkg.narrow_band_least_squares_consistency)
    assert list(sig.parameters) == ref_args + ['subsample']
    assert sig.parameters['subsample'].kind is inspect.Parameter.KEYWORD_ONLY and sig.parameters['subsample'].default is False
    multi = inspect.signature(pkg.ltsva_multi).parameters
    assert list(multi)[-1] == 'consistency' and multi['consistency'].default is False
    # the reference-named functions and ltsva_batch keep their signatures
    assert list(inspect.signature(pkg.ltsva).parameters) == ['st', 'lat_list', 'lon_list', 'window_length', 'window_overlap',
                                                              'alpha', 'plot_array_coordinates', 'rij']
    assert ref_args == ['WINLEN_list', 'WINOVER', 'ALPHA', 'st', 'lat_list', 'lon_list', 'NBANDS', 'w', 'h', 'freqlist',
                        'FREQ_BAND_TYPE', 'freq_resp_list', 'FILTER_TYPE', 'FILTER_ORDER', 'FILTER_RIPPLE', 'rij']
    assert list(inspect.signature(pkg.ltsva_batch).parameters) == ['streams', 'lat_list', 'lon_list', 'window_length',
                                                                    'window_overlap', 'alpha', 'rij', 'beam', 'subsample',
                                                                    'min_velocity', 'slowness_grid']
    for f in (engine.new_result, engine.process, engine.process_batch, engine.process_multi, engine.process_segmented):
        assert inspect.signature(f).parameters['want_consistency'].default is False
    assert inspect.signature(engine.launch).parameters['closure'].default is False
    assert inspect.signature(_hip.Handle.fetch_closure).parameters['e'].default == 0 and hasattr(_hip.Handle, 'set_closure')
    pkg.install_as_reference_modules()
    import lts_array
    import narrow_band_least_squares as nbls_mod
    assert lts_array.ltsva_consistency is pkg.ltsva_consistency
    assert nbls_mod.narrow_band_least_squares_consistency is pkg.narrow_band_least_squares_consistency
    assert lts_array.ltsva is pkg.ltsva


def test_new_result_carries_the_three_arrays_only_when_asked():
    from narrow_band_least_squares_amd import engine
    nwin = np.array([5, 3])
    res = engine.new_result(4, 1.0, 20.0, np.array([64, 64]), np.array([32, 32]), nwin, 8, want_consistency=True)
    assert res.consistency.shape == res.closure_max.shape == (2, 8) and res.element_consistency.shape == (2, 8, 4)
    assert not res.consistency.any() and not res.element_consistency.any()
    res = engine.new_result(4, 1.0, 20.0, np.array([64, 64]), np.array([32, 32]), nwin, 8)
    assert res.consistency is None and res.closure_max is None and res.element_consistency is None


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
        pkg.ltsva_consistency(_stream(4), None, None, 10.0, 0.5, rij=rij, subsample='yes')
    with pytest.raises(ValueError):
        pkg.ltsva_consistency(_stream(4), None, None, 10.0, 0.5, rij=rij, subsample=1)
    with pytest.raises(ValueError):
        pkg.ltsva_consistency(_stream(2), None, None, 10.0, 0.5, alpha=1.0, rij=rij[:, :2])
    with pytest.raises(ValueError):
        pkg.ltsva_consistency(_stream(3), None, None, 10.0, 0.5, alpha=0.75, rij=rij[:, :3])        # LTS needs four elements
    with pytest.raises(ValueError):
        pkg.ltsva_consistency(_stream(4), None, None, 10.0, 0.5, alpha=0.3, rij=rij)
    with pytest.raises(ValueError):
        pkg.ltsva_multi(_stream(4), None, None, 10.0, 0.5, [1.0, 0.75], rij=rij, consistency=1)
    with pytest.raises(ValueError):
        pkg.ltsva_multi(_stream(4), None, None, 10.0, 0.5, [(1.0, (0, 1))], rij=rij, consistency=True)
    fr = np.logspace(-1, 0.5, 16)
    args = ([10.0, 10.0], 0.5, 1.0, None, None, None, 2, np.zeros(16), np.zeros(16), np.array([0.5, 1.0, 2.0]), 'log', fr,
            'butter', 2, 0.01)
    with pytest.raises(ValueError):
        pkg.narrow_band_least_squares_consistency(*args[:3], _stream(4), *args[4:], rij=rij, subsample='no')
    with pytest.raises(ValueError):
        pkg.narrow_band_least_squares_consistency(*args[:3], _stream(2), *args[4:], rij=rij[:, :2])
    with pytest.raises(ValueError):
        pkg.narrow_band_least_squares_consistency(*args[:2], 0.75, _stream(3), *args[4:], rij=rij[:, :3])
    with pytest.raises(ValueError):
        pkg.narrow_band_least_squares_consistency(*args[:2], 0.2, _stream(4), *args[4:], rij=rij)
    with pytest.raises(TypeError):                                 # subsample is keyword-only
        pkg.narrow_band_least_squares_consistency(*args[:3], _stream(4), *args[4:], rij, True)
    # the time-segmented fallback correlates slice by slice: it names the limit instead of computing on the host
    with pytest.raises(ValueError, match='time-segmented'):
        engine.process_segmented(list(np.zeros((4, 600))), 20.0, 0.0, rij, [(0.5, 1.0)], [10.0], 0.5, 1.0, 'butter', 2, 0.01,
                                 None, want_consistency=True)


def test_header_binding_and_library_carry_the_symbols():
    from narrow_band_least_squares_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'nbls.h'), encoding='utf-8').read()
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
    assert b'closure_kernel' in blob


def test_header_and_design_state_the_same_definition():
    header = open(os.path.join(ROOT, 'include', 'nbls.h'), encoding='utf-8').read()
    design = open(os.path.join(ROOT, 'DESIGN.md'), encoding='utf-8').read()
    kernel = open(os.path.join(LIBDIR, 'closure.hip'), encoding='utf-8').read()
    for line in DEFINITION:
        assert line in header, line
        assert line in design, line
        assert line in kernel, line


def build_closure_caller():
    binary = os.path.join(CDIR, 'closure_caller')
    cmd = ['gcc', '-O1', '-Wall', '-Wextra', '-Werror', '-std=c11', '-pthread', '-I', os.path.join(ROOT, 'include'),
           os.path.join(CDIR, 'closure_caller.c'), '-o', binary, '-L', LIBDIR, '-lnbls_hip', '-lm',
           '-Wl,-rpath,$ORIGIN/../../narrow_band_least_squares_amd/csrc', '-Wl,-rpath-link,/opt/rocm/lib']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return binary


def test_plain_c_caller_compiles_and_links():
    binary = build_closure_caller()
    out = subprocess.run(['nm', '-u', binary], capture_output=True, text=True).stdout
    assert {'nbls_set_closure', 'nbls_fetch_closure', 'nbls_est_fetch_closure', 'nbls_plan', 'nbls_execute'} <= \
        set(re.findall(r'\b(nbls_[a-z0-9_]+)', out))


def test_closure_kernel_uses_no_scratch_and_spills_nothing(tmp_path):
    """Both instances (whole-sample and refined) from the compiler's resource report: no private segment, no spills."""
    hipcc = '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = tmp_path / 'closure.s'
    subprocess.run([hipcc, '-O3', '-std=c++17', '--offload-arch=gfx950', '-I' + LIBDIR, '-S', '--cuda-device-only',
                    os.path.join(LIBDIR, 'closure.hip'), '-o', str(out), '-ffp-contract=off'], check=True,
                   stderr=subprocess.DEVNULL, timeout=600)
    text = out.read_text()
    found = re.findall(r'\.amdhsa_kernel (\S*closure_kernel\S*)(.*?)\.end_amdhsa_kernel', text, re.S)
    assert len(found) == 2, [n for n, _ in found]
    for name, body in found:
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0, name
    for key in ('sgpr_spill_count', 'vgpr_spill_count', 'private_segment_fixed_size'):
        vals = re.findall(r'\.%s:\s+(\d+)' % key, text)
        assert len(vals) == 2 and all(int(v) == 0 for v in vals), (key, vals)
