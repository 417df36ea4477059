"""What of the refinement of the grid maximum (``nbls_set_beam_grid_refinement``) a box without a GPU
can check: the new Python names, their signatures and argument checks, the three symbols in the header, the ctypes binding
and the built library, the request's way onto a handle and off it, its row of result fields, the LDS formula and the
compiler's resource report of the new kernel."""
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, 'narrow_band_least_squares_amd', 'csrc')
SYMBOLS = ('nbls_set_beam_grid_refinement', 'nbls_fetch_beam_grid_refined', 'nbls_beam_grid_refine_lds_bytes')
LTSVA_ARGS = ['st', 'lat_list', 'lon_list', 'window_length', 'window_overlap']
REFINE_ARGS = ['slowness_grid', 'alpha', 'rij', 'levels', 'step', 'taps', 'grid_map']
REFINE_DEFAULTS = dict(alpha=1.0, rij=None, levels=4, step=None, taps=8, grid_map=False)
FIELDS = (('grid_refined_slowness', (2,), np.float64), ('grid_refined_fstat', (), np.float64), ('grid_refined_power', (), np.float64),
          ('grid_refined_path', ('R',), np.int32), ('grid_refined_stencil', (9,), np.float64))
GRID = np.array([[a, b] for a in (-1.0, 0.0, 1.0) for b in (-0.5, 0.0, 0.5)])


def test_python_names_and_signatures():
    import narrow_band_least_squares_amd as pkg
    from narrow_band_least_squares_amd import engine, planner, _hip
    from narrow_band_least_squares_amd.call_requests import Requests
    for name in ('ltsva_grid_refined', 'ltsva_grid_refined_batch', 'narrow_band_least_squares_grid_refined'):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    sig = inspect.signature(pkg.ltsva_grid_refined).parameters
    sigb = inspect.signature(pkg.ltsva_grid_refined_batch).parameters
    assert list(sig) == LTSVA_ARGS + REFINE_ARGS and list(sigb) == ['streams'] + LTSVA_ARGS[1:] + REFINE_ARGS
    assert sig['slowness_grid'].default is inspect.Parameter.empty
    for k, v in REFINE_DEFAULTS.items():
        assert sig[k].default == v and sigb[k].default == v and type(sig[k].default) is type(v), k
    ref_args = list(inspect.signature(pkg.narrow_band_least_squares).parameters)
    sign = inspect.signature(pkg.narrow_band_least_squares_grid_refined).parameters
    assert list(sign) == ref_args + ['slowness_grid', 'levels', 'step', 'taps', 'grid_map']
    for k in ('slowness_grid', 'levels', 'step', 'taps', 'grid_map'):
        assert sign[k].kind is inspect.Parameter.KEYWORD_ONLY
    assert sign['slowness_grid'].default is inspect.Parameter.empty and sign['levels'].default == 4 and sign['step'].default is None
    assert sign['taps'].default == 8 and sign['grid_map'].default is False
    assert list(inspect.signature(planner.check_grid_refinement).parameters) == ['levels', 'step', 'grid', 'taps', 'has_seed']
    assert list(inspect.signature(_hip.Handle.set_beam_grid_refinement).parameters) == ['self', 'levels', 'step']
    assert callable(_hip.Handle.fetch_beam_grid_refined)
    for f in (engine.process, engine.process_batch, engine.launch, Requests.check):
        assert inspect.signature(f).parameters['grid_refine'].default is None
    assert 'grid_refine' in Requests.KEYWORDS and Requests.DEFAULTS['grid_refine'] is None
    assert inspect.signature(engine.new_result).parameters['grid_refine_levels'].default == 0
    # the functions that were there keep their signatures
    assert list(inspect.signature(pkg.ltsva_grid).parameters) == LTSVA_ARGS + ['slowness_grid', 'alpha', 'rij', 'grid_map']
    assert list(inspect.signature(pkg.ltsva_seeded).parameters) == LTSVA_ARGS + ['slowness_grid', 'halfwidth', 'alpha', 'rij', 'grid_map']
    assert list(inspect.signature(pkg.ltsva_steered).parameters) == LTSVA_ARGS + ['alpha', 'rij', 'taps', 'slowness_grid', 'grid_map',
                                                                                  'subsample', 'kept', 'min_pairs']
    assert list(inspect.signature(pkg.narrow_band_least_squares_grid).parameters) == ref_args + ['slowness_grid', 'grid_map']
    assert list(inspect.signature(pkg.narrow_band_least_squares_steered).parameters) == ref_args + ['taps', 'slowness_grid', 'grid_map',
                                                                                                  'subsample']
    assert list(inspect.signature(pkg.ltsva).parameters) == LTSVA_ARGS + ['alpha', 'plot_array_coordinates', 'rij']
    for f in (pkg.ltsva, pkg.ltsva_grid, pkg.ltsva_steered, pkg.ltsva_batch, pkg.narrow_band_least_squares, pkg.narrow_band_least_squares_grid):
        assert 'levels' not in inspect.signature(f).parameters
    pkg.install_as_reference_modules()
    import lts_array
    import narrow_band_least_squares as nbls_mod
    assert lts_array.ltsva_grid_refined is pkg.ltsva_grid_refined and lts_array.ltsva_grid_refined_batch is pkg.ltsva_grid_refined_batch
    assert nbls_mod.narrow_band_least_squares_grid_refined is pkg.narrow_band_least_squares_grid_refined


def test_check_grid_refinement():
    from narrow_band_least_squares_amd import planner
    levels, step = planner.check_grid_refinement(4, None, GRID, 8, False)
    assert levels == 4 and type(levels) is int and step.dtype == np.float64 and step.tolist() == [1.0, 0.5]
    levels, step = planner.check_grid_refinement(np.int32(12), (0.25, 2.0), GRID, 4)
    assert levels == 12 and step.tolist() == [0.25, 2.0]
    assert planner.check_grid_refinement(1, [0.1, 0.1], GRID[:1], 6)[0] == 1       # a given step needs no lattice
    for bad in (0, 13, -1, 2.5, True, False, None, '4', [4]):
        with pytest.raises(ValueError, match='levels'):
            planner.check_grid_refinement(bad, None, GRID, 8)
    for bad in ((0.0, 1.0), (1.0, -1.0), (np.nan, 1.0), (1.0, np.inf), (1.0,), (1.0, 1.0, 1.0), 1.0, 'ab', [[1.0, 1.0]]):
        with pytest.raises(ValueError, match='step'):
            planner.check_grid_refinement(4, bad, GRID, 8)
    with pytest.raises(ValueError, match='steering'):
        planner.check_grid_refinement(4, None, GRID, 0)                            # no taps: F is piecewise constant
    with pytest.raises(ValueError):
        planner.check_grid_refinement(4, None, GRID, 5)
    with pytest.raises(ValueError, match='seed'):
        planner.check_grid_refinement(4, None, GRID, 8, True)
    with pytest.raises(ValueError, match='slowness_grid'):
        planner.check_grid_refinement(4, None, None, 8)
    with pytest.raises(ValueError, match='single value on axis 1'):                # an axis with one value has no lattice step
        planner.check_grid_refinement(4, None, GRID[1::3], 8)
    with pytest.raises(ValueError, match='single value on axis 0'):
        planner.check_grid_refinement(4, None, GRID[3:6], 8)


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
    bad_kw = [dict(levels=0), dict(levels=13), dict(levels=2.5), dict(levels=True), dict(step=(0.0, 1.0)), dict(step=(np.nan, 1.0)),
              dict(step=1.0), dict(taps=0), dict(taps=5), dict(grid_map=1), dict(slowness_grid=np.zeros((3, 3))),
              dict(slowness_grid=GRID[3:6]), dict(alpha=0.3)]
    for kw in bad_kw:
        kw = dict(dict(slowness_grid=GRID), **kw)
        with pytest.raises(ValueError):
            pkg.ltsva_grid_refined(_stream(4), None, None, 10.0, 0.5, rij=rij, **kw)
        with pytest.raises(ValueError):
            pkg.ltsva_grid_refined_batch([_stream(4), _stream(4)], None, None, 10.0, 0.5, rij=rij, **kw)
    with pytest.raises(ValueError):
        pkg.ltsva_grid_refined(_stream(2), None, None, 10.0, 0.5, GRID, rij=rij[:, :2])
    assert pkg.ltsva_grid_refined_batch([], None, None, 10.0, 0.5, GRID) == []
    rows = list(np.zeros((4, 600)))
    for kw in (dict(grid_refine=4), dict(grid_refine=4, slowness_grid=GRID), dict(grid_refine=(4, None, 1), slowness_grid=GRID, beam_taps=8),
               dict(grid_refine=(), slowness_grid=GRID, beam_taps=8), dict(grid_refine=4, slowness_grid=GRID, beam_taps=8, seed_halfwidths=3),
               dict(grid_refine=(4, (1.0, 0.0)), slowness_grid=GRID, beam_taps=8)):
        with pytest.raises(ValueError):
            engine.process(rows, 20.0, 0.0, rij, [(None, None)], [10.0], 0.5, 1.0, prefiltered=True, **kw)
        with pytest.raises(ValueError):
            engine.process_batch([rows] * 2, 20.0, [0.0, 0.0], rij, [(None, None)], [10.0], 0.5, 1.0, prefiltered=True, **kw)
    fr = np.logspace(-1, 0.5, 16)
    args = ([10.0, 10.0], 0.5, 1.0, _stream(4), None, None, 2, np.zeros(16), np.zeros(16), np.array([0.5, 1.0, 2.0]), 'log', fr,
            'butter', 2, 0.01)
    for kw in (dict(levels=0), dict(levels=13), dict(step=(1.0, -1.0)), dict(taps=0), dict(grid_map=1), dict(slowness_grid=GRID[1::3])):
        with pytest.raises(ValueError):
            pkg.narrow_band_least_squares_grid_refined(*args, rij=rij, **dict(dict(slowness_grid=GRID), **kw))
    with pytest.raises(TypeError):                                 # the extensions are keywords
        pkg.narrow_band_least_squares_grid_refined(*args, rij, GRID)


def test_header_declares_and_binding_knows_the_symbols():
    from narrow_band_least_squares_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'nbls.h'), encoding='utf-8').read()
    assert re.search(r'^int nbls_set_beam_grid_refinement\(nbls_handle\* h, int32_t levels /\* 0 = off \*/, const double\* step', header, re.M)
    assert re.search(r'^int nbls_fetch_beam_grid_refined\(nbls_handle\* h, double\* slowness, double\* fstat, double\* power, int32_t\* path, '
                     r'double\* stencil\);', header, re.M)
    assert re.search(r'^int nbls_beam_grid_refine_lds_bytes\(int32_t nelem, int32_t W, int32_t halo\);', header, re.M)
    assert re.search(r'^#define NBLS_BEAM_GRID_REFINE_MAX_LEVELS 12$', header, re.M) and _hip.GRID_REFINE_MAX_LEVELS == 12
    for s in SYMBOLS:
        assert s in _hip.EXPORTS
    # the defining lines of the header are those of the definition the truth restates
    for phrase in ('e = (ldexp(h0, -l), ldexp(h1, -l))', 'a = j / 3 - 1,  b = j % 3 - 1', 'j = 4 is the centre and is not evaluated again',
                   'the centre before any other', 'A NaN F is no candidate', 'taken before the move', 'j* = 4 leaves all three unchanged',
                   'H_r = grid_halo + ceil(fs max_i(|xij[i][0]| h0 + |xij[i][1]| h1)) + 1', 'width of the main lobe'):
        assert phrase in header, phrase


def test_library_exports_and_prototypes():
    import ctypes as C
    from narrow_band_least_squares_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('library not built')
    lib = _hip.load_library()
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    assert lib.nbls_set_beam_grid_refinement.argtypes == [C.c_void_p, C.c_int32, dp]
    assert lib.nbls_fetch_beam_grid_refined.argtypes == [C.c_void_p, dp, dp, dp, ip, dp]
    assert lib.nbls_beam_grid_refine_lds_bytes.argtypes == [C.c_int32, C.c_int32, C.c_int32]
    assert lib.nbls_set_beam_grid_refinement(None, 4, None) == _hip.NBLS_ERR_ARG
    assert lib.nbls_fetch_beam_grid_refined(None, None, None, None, None, None) == _hip.NBLS_ERR_ARG


def test_lds_formula_at_its_cap():
    """nelem (W + 2 halo) 8 bytes up to the grid kernel's 156 KiB, 0 beyond: the global form."""
    from narrow_band_least_squares_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        pytest.skip('library not built')
    lib = _hip.load_library()
    cap = 156 * 1024
    for nelem, W in ((3, 16), (4, 257), (8, 400), (8, 1200), (32, 513)):
        fits = (cap // (8 * nelem) - W) // 2                                       # the largest halo that is staged
        assert fits >= 0 and nelem * (W + 2 * fits) * 8 <= cap < nelem * (W + 2 * (fits + 1)) * 8
        assert lib.nbls_beam_grid_refine_lds_bytes(nelem, W, fits) == nelem * (W + 2 * fits) * 8
        assert lib.nbls_beam_grid_refine_lds_bytes(nelem, W, fits + 1) == 0
        assert lib.nbls_beam_grid_refine_lds_bytes(nelem, W, 0) == nelem * W * 8
        assert lib.nbls_beam_grid_refine_lds_bytes(nelem, W, fits) == lib.nbls_beam_grid_lds_bytes(nelem, W, fits)
    assert lib.nbls_beam_grid_refine_lds_bytes(8, 2496, 0) == cap and lib.nbls_beam_grid_refine_lds_bytes(8, 2497, 0) == 0
    for bad in ((0, 16, 0), (3, 0, 0), (3, 16, -1)):
        assert lib.nbls_beam_grid_refine_lds_bytes(*bad) == _hip.NBLS_ERR_ARG
    assert lib.nbls_beam_grid_refine_lds_bytes(3, 16, 2 ** 30) == 0


class Refused(RuntimeError):
    pass


class StandIn:
    """Logs every call as (name, args, kwargs); ``refuse``: the first call of that method raises ``Refused``."""

    def __init__(self, refuse=None):
        self.refuse, self.log = refuse, []

    def __getattr__(self, name):
        if name.startswith('_'):
            raise AttributeError(name)

        def call(*args, **kw):
            self.log.append((name, args, kw))
            if name == self.refuse:
                raise Refused(name)
        return call

    def calls(self, name):
        return [(a, kw) for n, a, kw in self.log if n == name]


def _record(**more):
    from narrow_band_least_squares_amd.call_requests import Requests
    rij = np.array([[0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 1.0, 1.0]])
    return Requests.check(4, 2, 20.0, [200, 100], rij=rij, **dict(dict(slowness_grid=GRID, beam_taps=8), **more))


def test_the_request_goes_onto_the_handle_and_comes_off_it():
    from narrow_band_least_squares_amd import planner
    from narrow_band_least_squares_amd.call_requests import STEPS
    xij = planner.co_array(np.array([[0.0, 1.0, 0.0, 1.0], [0.0, 0.0, 1.0, 1.0]]))[0]
    req = _record(grid_refine=(5, (0.5, 0.25)))
    assert req.grid_refine[0] == 5 and req.grid_refine[1].tolist() == [0.5, 0.25] and req.on('grid_refine')
    assert _record(grid_refine=3).grid_refine[1].tolist() == [1.0, 0.5]           # the grid's lattice step
    assert [s.method for s in STEPS].count('set_beam_grid_refinement') == 1
    h = StandIn()
    with req.applied(h, xij):
        h.plan()
    names = [n for n, _, _ in h.log]
    sets = h.calls('set_beam_grid_refinement')
    assert len(sets) == 2 and sets[0][0][0] == 5 and sets[0][0][1].tolist() == [0.5, 0.25] and sets[1] == ((0, None), {})
    at = names.index('plan')
    assert names.index('set_beam_grid') < names.index('set_beam_interpolation') < names.index('set_beam_grid_refinement') < at
    assert names[at + 1:].count('set_beam_grid_refinement') == 1
    # unset on every way out: a plan that refuses, a later setter that refuses, the refinement's own setter refusing
    h = StandIn(refuse='plan')
    with pytest.raises(Refused):
        with req.applied(h, xij):
            h.plan()
    assert h.calls('set_beam_grid_refinement')[-1] == ((0, None), {})
    h = StandIn(refuse='set_beam_grid_refinement')
    with pytest.raises(Refused):
        with req.applied(h, xij):
            h.plan()
    assert len(h.calls('set_beam_grid_refinement')) == 1 and not h.calls('plan')   # what was not set is not unset
    assert h.calls('set_beam_grid')[-1] == ((None,), {}) and h.calls('set_beam_interpolation')[-1] == ((0,), {})
    # untouched when off
    off = _record()
    assert off.grid_refine is None and not off.on('grid_refine')
    h = StandIn()
    with off.applied(h, xij):
        h.plan()
    assert not h.calls('set_beam_grid_refinement') and h.calls('set_beam_grid')


def test_for_bands_and_the_result_keywords():
    req = _record(grid_refine=(5, (0.5, 0.25)))
    cut = req.for_bands(slice(1, 2))
    assert cut.grid_refine is req.grid_refine and cut.beam_grid is req.beam_grid
    assert req.result_keywords(100)['grid_refine_levels'] == 5 and req.wants().grid_refine_levels == 5
    assert _record().result_keywords(100)['grid_refine_levels'] == 0
    # the time-segmented path refuses what the request needs — the steering, then the grid — and so the request
    with pytest.raises(ValueError, match='fractional-sample steering is not available'):
        req.segmented_refusal(4, 10 ** 6)
    with pytest.raises(ValueError, match='slowness-grid search is not available'):
        req.replace(beam_taps=0).segmented_refusal(4, 10 ** 6)


def test_the_result_group_allocates_and_scatters():
    from narrow_band_least_squares_amd import engine
    from narrow_band_least_squares_amd.call_requests import RESULT_GROUPS
    rows = [g for g in RESULT_GROUPS if g.method == 'fetch_beam_grid_refined']
    assert len(rows) == 1 and not rows[0].est and not rows[0].per_row
    assert tuple((n, t, d) for n, t, d in rows[0].calls[0][1]) == FIELDS
    req = _record(grid_refine=(5, (0.5, 0.25)))
    VL, nb = 7, 2
    args = (4, 1.0, 20.0, np.array([200, 100]), np.array([100, 50]), np.array([5, 7]), VL)
    res = engine.new_result(*args, **req.result_keywords(1000))
    for name, trailing, dtype in FIELDS:
        a = getattr(res, name)
        assert a.shape == (nb, VL) + tuple(5 if t == 'R' else t for t in trailing) and a.dtype == dtype and not a.any()
    off = engine.new_result(*args, **_record().result_keywords(1000))
    assert off.grid_index is not None and not any(hasattr(off, name) for name, _, _ in FIELDS)

    class Fetcher(StandIn):
        def fetch_beam_grid(self):
            return np.full((nb, VL), 2, dtype=np.int32), np.full((nb, VL), 3.0), np.full((nb, VL), 4.0)

        def fetch_beam_grid_refined(self):
            self.log.append(('fetch_beam_grid_refined', (), {}))
            return tuple(np.full((nb, VL) + tuple(5 if t == 'R' else t for t in trailing), 10 + k, dtype=dtype)
                         for k, (_, trailing, dtype) in enumerate(FIELDS))
    h = Fetcher()
    engine.fetch_groups(h, req, [res], 0, nb)
    assert len(h.calls('fetch_beam_grid_refined')) == 1
    for k, (name, _, _) in enumerate(FIELDS):
        assert np.all(getattr(res, name) == 10 + k)
    # two recordings of one pass: row b * 2 + s is band b of recording s
    pair = [engine.new_result(*args, **req.result_keywords(1000)) for _ in range(2)]

    class Interleaved(Fetcher):
        def fetch_beam_grid(self):
            return tuple(np.repeat(a, 2, axis=0) for a in Fetcher.fetch_beam_grid(self))

        def fetch_beam_grid_refined(self):
            out = []
            for k, (_, trailing, dtype) in enumerate(FIELDS):
                a = np.empty((2 * nb, VL) + tuple(5 if t == 'R' else t for t in trailing), dtype=dtype)
                a[...] = (np.arange(2 * nb) % 2 * 100 + k).reshape((-1,) + (1,) * (a.ndim - 1))
                out.append(a)
            return tuple(out)
    engine.fetch_groups(Interleaved(), req, pair, 0, nb)
    for s, r in enumerate(pair):
        for k, (name, _, _) in enumerate(FIELDS):
            assert np.all(getattr(r, name) == 100 * s + k), (s, name)


def test_new_kernel_uses_no_scratch_and_spills_no_vector_register(tmp_path):
    """The compiler's resource report of beam_grid_refine.hip: six instances of grid_refine_kernel (staged and global, 4, 6
    and 8 taps), none with a private segment or a spilled vector register; the staged form's taps are single ds_read_b64;
    no atomics; a translation unit of its own, built without contraction."""
    hipcc = '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    out = tmp_path / 'beam_grid_refine.s'
    subprocess.run([hipcc, '-O3', '-std=c++17', '--offload-arch=gfx950', '-I' + LIBDIR, '-S', '--cuda-device-only',
                    os.path.join(LIBDIR, 'beam_grid_refine.hip'), '-o', str(out), '-ffp-contract=off'], check=True,
                   stderr=subprocess.DEVNULL, timeout=900)
    text = out.read_text()
    found = re.findall(r'\.amdhsa_kernel (\S*grid_refine_kernel\S*)(.*?)\.end_amdhsa_kernel', text, re.S)
    assert len(found) == 6, [n for n, _ in found]
    assert sorted(re.search(r'ILb([01])ELi(\d)E', n).groups() for n, _ in found) == [(f, t) for f in '01' for t in '468']
    for name, body in found:
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0, name
        assert int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1)) == 128, name      # the eight (F, P) pairs
    for key in ('vgpr_spill_count', 'private_segment_fixed_size'):
        vals = re.findall(r'\.%s:\s+(\d+)' % key, text)
        assert len(vals) == 6 and all(int(v) == 0 for v in vals), (key, vals)
    assert 'ds_read_b64' in text and 'ds_read2' not in text
    assert not re.search(r'\b(global|flat|ds|buffer)_atomic', text)
    mk = open(os.path.join(LIBDIR, 'Makefile'), encoding='utf-8').read()
    assert 'beam_grid_refine.o' in re.search(r'^OBJS = (.*)$', mk, re.M).group(1).split()
    assert 'beam_grid_refine.hip' in re.search(r'^DEVSRC = (.*)$', mk, re.M).group(1).split()
    assert re.search(r'^beam_grid_refine\.o:.* steer\.h .*\n\t\$\(HIPCC\) \$\(CXXFLAGS\) \$\(NOFMA\) -c', mk, re.M)
    src = open(os.path.join(LIBDIR, 'beam_grid.hip'), encoding='utf-8').read()
    assert 'grid_refine_kernel' not in src                                        # the grid's own file holds no new kernel
