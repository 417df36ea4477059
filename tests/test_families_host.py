"""Host side of the family labelling (``nbls_set_families`` / ``nbls_label_families``): names, signatures
and defaults of everything new, every earlier signature as it was, the header's declarations and their bindings, every
``ValueError`` before any GPU call, the Makefile's lines, the compiler's resource report, ``planner.family_table`` on
hand-made families and the split of a batch's labelling.  CPU only."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import families_cases as fc
import families_truth as ft
import narrow_band_least_squares_amd as pkg
from narrow_band_least_squares_amd import _hip, engine, planner, synthetic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, 'narrow_band_least_squares_amd', 'csrc')
SYMBOLS = ['nbls_set_families', 'nbls_fetch_families', 'nbls_label_families']
FS = 20.0
REQUEST = ['mdccm_min', 'baz_tol', 'vel_tol', 'vel_min', 'vel_max', 'sigma_tau_max', 'band_reach', 'time_reach', 'min_pixels']
LTSVA_ARGS = ['st', 'lat_list', 'lon_list', 'window_length', 'window_overlap', 'alpha', 'rij']
GOOD = dict(mdccm_min=0.5, baz_tol=5.0, vel_tol=0.03, vel_min=0.2, vel_max=0.6)


def _defaults(f):
    return {k: p.default for k, p in inspect.signature(f).parameters.items() if p.default is not inspect.Parameter.empty}


def test_public_names_signatures_and_defaults():
    for name in ('narrow_band_least_squares_families', 'narrow_band_least_squares_families_batch', 'ltsva_families',
                 'ltsva_families_batch', 'label_families'):
        assert name in pkg.__all__ and callable(getattr(pkg, name))
    ref_args = list(inspect.signature(pkg.narrow_band_least_squares).parameters)
    for f, head in ((pkg.narrow_band_least_squares_families, ref_args),
                    (pkg.narrow_band_least_squares_families_batch, ref_args[:3] + ['streams'] + ref_args[4:]),
                    (pkg.ltsva_families, LTSVA_ARGS), (pkg.ltsva_families_batch, ['streams'] + LTSVA_ARGS[1:])):
        sig = inspect.signature(f)
        assert list(sig.parameters) == head + REQUEST, f.__name__
        for k in REQUEST:
            assert sig.parameters[k].kind is inspect.Parameter.KEYWORD_ONLY, k
        for k in REQUEST[:5]:
            assert sig.parameters[k].default is inspect.Parameter.empty, k
        assert [sig.parameters[k].default for k in REQUEST[5:]] == [None, 1, 1, 4]
    assert list(inspect.signature(pkg.label_families).parameters) == ['vel', 'baz', 'mdccm', 'sigma_tau', 'nwin', 'winlens', 'incs', 'nseg',
                                                                      'device', 'params']
    assert list(inspect.signature(planner.check_families).parameters) == REQUEST[:1] + ['baz_tol', 'vel_tol', 'vel_min', 'vel_max'] + \
        REQUEST[5:] + ['window_slice', 'estimators', 'comm']
    assert _defaults(planner.check_families) == dict(sigma_tau_max=None, band_reach=1, time_reach=1, min_pixels=1, window_slice=None,
                                                     estimators=None, comm=False)
    assert list(inspect.signature(planner.family_table).parameters) == ['family', 'table', 'vel', 'baz', 'mdccm', 'sigma_tau', 'band_edges',
                                                                        'winlens', 'incs', 'fs', 'starttime']
    assert list(inspect.signature(_hip.Handle.set_families).parameters) == ['self', 'params']
    assert list(inspect.signature(_hip.Handle.fetch_families).parameters) == ['self', 'capacity']
    assert list(inspect.signature(_hip.Handle.label_families).parameters) == ['self', 'params', 'nseg', 'winlen', 'wininc', 'nwin', 'vel',
                                                                              'baz', 'mdccm', 'sigma_tau', 'capacity']
    assert list(inspect.signature(synthetic.transient_waves).parameters) == ['rij', 'npts', 'fs', 'sources', 'snr_db', 'seed', 'ramp_s']
    for f in (engine.launch, engine.process, engine.process_batch):
        p = inspect.signature(f).parameters
        assert 'families' in p and p['families'].default is None, f.__name__
    assert _hip.FAMILY_FIELDS == planner.FAMILY_FIELDS == ft.FIELDS and len(ft.FIELDS) == _hip.FAMILY_COLUMNS == 8


def test_install_as_reference_modules_exports_the_new_functions():
    pkg.install_as_reference_modules()
    import lts_array as la
    import narrow_band_least_squares as nb
    assert la.ltsva_families is pkg.ltsva_families and la.ltsva_families_batch is pkg.ltsva_families_batch
    assert nb.narrow_band_least_squares_families is pkg.narrow_band_least_squares_families
    assert nb.label_families is pkg.label_families


def test_earlier_signatures_and_pinned_tails_are_unchanged():
    assert list(inspect.signature(engine.launch).parameters)[-4:] == ['element_delays', 'element_delays_kept', 'beam_trace', 'beam_taps']
    assert list(inspect.signature(engine.process).parameters)[-4:] == ['element_max_shift', 'element_delays_kept', 'want_beam_trace',
                                                                       'beam_taps']
    assert list(inspect.signature(engine.process_batch).parameters)[-4:] == ['element_max_shift', 'element_delays_kept',
                                                                             'want_beam_trace', 'beam_taps']
    assert list(inspect.signature(engine.new_result).parameters)[-4:] == ['want_music', 'want_music_maps', 'want_music_vectors',
                                                                          'want_music_peaks']
    assert list(inspect.signature(_hip.Handle.set_beam_trace).parameters) == ['self', 'window', 'mdccm_min', 'kept']


def test_header_binding_and_library_agree():
    header = open(os.path.join(ROOT, 'include', 'nbls.h'), encoding='utf-8').read()
    assert re.search(r'^int nbls_set_families\(nbls_handle\* h, const nbls_family_params\* params /\* NULL = off \*/\);', header, re.M)
    assert re.search(r'^int nbls_fetch_families\(nbls_handle\* h, int32_t\* family, int32_t\* nfamilies, int64_t\* table, int64_t capacity\);',
                     header, re.M)
    assert re.search(r'^int nbls_label_families\(nbls_handle\* h, const nbls_family_params\* params, int32_t nbands, int32_t nseg, '
                     r'int32_t vector_len,$', header, re.M)
    assert re.search(r'^    double mdccm_min, vel_min, vel_max, sigma_tau_max, baz_tol, vel_tol;\n    int32_t band_reach, time_reach, '
                     r'min_pixels, flags;\n\} nbls_family_params;', header, re.M)
    assert [n for n, _ in _hip.FamilyParams._fields_] == ['mdccm_min', 'vel_min', 'vel_max', 'sigma_tau_max', 'baz_tol', 'vel_tol',
                                                          'band_reach', 'time_reach', 'min_pixels', 'flags']
    assert C.sizeof(_hip.FamilyParams) == 6 * 8 + 4 * 4
    assert re.search(r'^#define NBLS_FAMILY_COLUMNS %d$' % _hip.FAMILY_COLUMNS, header, re.M)
    assert re.search(r'^#define NBLS_FAMILY_MAX_REACH %d$' % _hip.FAMILY_MAX_REACH, header, re.M)
    assert planner.FAMILY_MAX_REACH == _hip.FAMILY_MAX_REACH
    for phrase in ('c2 = 2 * s0 + W_b', '|c2 - c2\'| <= 2 * time_reach * max(inc_b, inc_b\')', 'd = 360.0 - d if d > 180.0',
                   'ascending order of their smallest cell', '-2 for an eligible cell whose component is too small',
                   'count | first_cell (the smallest cell) | peak_cell', 'sample_first (min s0) | sample_end (max s0 + W_b)',
                   'a NaN fails the gate'):
        assert phrase in header, phrase
    for s in SYMBOLS:
        assert s in _hip.EXPORTS
    lib = _hip.load_library()
    dp, ip, lp = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int64)
    fp = C.POINTER(_hip.FamilyParams)
    assert lib.nbls_set_families.argtypes == [C.c_void_p, fp]
    assert lib.nbls_fetch_families.argtypes == [C.c_void_p, ip, ip, lp, C.c_int64]
    assert lib.nbls_label_families.argtypes == [C.c_void_p, fp, C.c_int32, C.c_int32, C.c_int32, ip, ip, ip, dp, dp, dp, dp, ip, ip, lp,
                                                C.c_int64]
    out = subprocess.run(['nm', '-D', '--defined-only', _hip.LIB_PATH], capture_output=True, text=True).stdout
    assert set(SYMBOLS) <= set(re.findall(r'\b(nbls_[a-z0-9_]+)', out))
    # without a handle: argument errors, not crashes
    assert lib.nbls_set_families(None, None) == _hip.NBLS_ERR_ARG
    assert lib.nbls_fetch_families(None, None, None, None, 0) == _hip.NBLS_ERR_ARG
    assert lib.nbls_label_families(None, None, 0, 0, 0, None, None, None, None, None, None, None, None, None, None, 0) == _hip.NBLS_ERR_ARG
    p = _hip.family_params(0.5, 0.2, 0.6, None, 5.0, 0.03, 1, 2, 3)
    assert (p.mdccm_min, p.vel_min, p.vel_max, p.baz_tol, p.vel_tol, p.band_reach, p.time_reach, p.min_pixels, p.flags) == \
        (0.5, 0.2, 0.6, 5.0, 0.03, 1, 2, 3, 0) and np.isnan(p.sigma_tau_max)
    assert _hip.family_params(0.5, 0.2, 0.6, 0.25, 5.0, 0.03, 1, 2, 3).sigma_tau_max == 0.25


BAD = [dict(mdccm_min=np.nan), dict(mdccm_min=np.inf), dict(mdccm_min='x'), dict(mdccm_min=None), dict(mdccm_min=True),
       dict(vel_min=0.7), dict(vel_min=np.nan), dict(vel_max=np.inf), dict(vel_max=None), dict(sigma_tau_max=np.inf),
       dict(sigma_tau_max=-np.inf), dict(sigma_tau_max='x'), dict(baz_tol=-0.5), dict(baz_tol=180.5), dict(baz_tol=np.nan),
       dict(baz_tol=None), dict(vel_tol=-0.01), dict(vel_tol=np.nan), dict(vel_tol=np.inf), dict(band_reach=-1), dict(band_reach=9),
       dict(band_reach=1.0), dict(band_reach=True), dict(time_reach=0), dict(time_reach=9), dict(time_reach=1.5), dict(time_reach=None),
       dict(min_pixels=0), dict(min_pixels=-3), dict(min_pixels=2.0), dict(min_pixels=2 ** 31), dict(window_slice=(0, 2)),
       dict(estimators=[(1.0, (0,))]), dict(comm=True)]


@pytest.mark.parametrize('bad', BAD, ids=[','.join(b) + str(i) for i, b in enumerate(BAD)])
def test_check_families_refuses(bad):
    with pytest.raises(ValueError):
        planner.check_families(**dict(GOOD, **bad))


def test_check_families_returns():
    want = dict(GOOD, sigma_tau_max=None, band_reach=1, time_reach=1, min_pixels=1)
    assert planner.check_families(**GOOD) == want
    assert planner.check_families(0.5, 5.0, 0.03, 0.2, 0.6) == want
    assert planner.check_families(**dict(GOOD, sigma_tau_max=np.nan)) == want                    # NaN: no gate, as in the C ABI
    got = planner.check_families(np.float32(0.5), 0, np.int64(0), 0.3, 0.3, 0.25, np.int32(8), 8, np.int64(7))
    assert got == dict(mdccm_min=0.5, baz_tol=0.0, vel_tol=0.0, vel_min=0.3, vel_max=0.3, sigma_tau_max=0.25, band_reach=8, time_reach=8,
                       min_pixels=7)
    assert planner.check_families(**dict(GOOD, baz_tol=180, mdccm_min=-1))['baz_tol'] == 180.0
    _hip.family_params(**got)                                                                   # the dict is the binding's keywords


def test_check_family_lattice():
    z = np.zeros((6, 5))
    ok = planner.check_family_lattice(2, [40, 60, 80], [20, 30, 40], [5] * 6, z, z, z, None, False)
    assert ok[0] == 2 and ok[1].dtype == ok[2].dtype == ok[3].dtype == np.int32 and ok[4].flags.c_contiguous and ok[7] is None
    for bad in (dict(nseg=0), dict(nseg=4), dict(winlens=[40, 60]), dict(winlens=[40, 0, 80]), dict(incs=[20, -1, 40]),
                dict(incs=[20.0, 30.0, 40.0]), dict(nwin=[5] * 5), dict(nwin=[6] + [5] * 5), dict(nwin=[-1] + [5] * 5), dict(vel=z[:5]),
                dict(baz=z[:, :4]), dict(mdccm=z.reshape(-1)), dict(sigma_tau=z), dict(gate=True), dict(sigma_tau=z[:, :4], gate=True)):
        kw = dict(dict(nseg=2, winlens=[40, 60, 80], incs=[20, 30, 40], nwin=[5] * 6, vel=z, baz=z, mdccm=z, sigma_tau=None, gate=False), **bad)
        with pytest.raises(ValueError):
            planner.check_family_lattice(**kw)
    assert planner.check_family_lattice(2, [40, 60, 80], [20, 30, 40], [5] * 6, z, z, z, z, True)[7] is not None


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
    call = lambda **kw: engine.process(data, FS, 0.0, rij, [(None, None)], [65.5 / FS], 0.5, 1.0, prefiltered=True, **kw)
    bads = [dict(GOOD, **b) for b in BAD if not set(b) & {'window_slice', 'estimators', 'comm'}]
    for bad in bads + [dict(GOOD, nope=1), {k: v for k, v in GOOD.items() if k != 'baz_tol'}, (0.5, 5.0), 'x', 3]:
        with pytest.raises(ValueError):
            call(families=bad)
        with pytest.raises(ValueError):
            engine.process_batch([list(data), list(data)], FS, [0.0, 1.0], rij, [(None, None)], [65.5 / FS], 0.5, 1.0, prefiltered=True,
                                 families=bad)
    with pytest.raises(ValueError, match='window_slice'):
        call(families=GOOD, window_slice=(0, 2))
    args = (st, None, None, 65.5 / FS, 0.5)
    for bad in bads:
        with pytest.raises(ValueError):
            pkg.ltsva_families(*args, rij=rij, **bad)
        with pytest.raises(ValueError):
            pkg.ltsva_families_batch([st, st], *args[1:], rij=rij, **bad)
        with pytest.raises(ValueError):
            pkg.ltsva_families_batch([], *args[1:], rij=rij, **bad)
    with pytest.raises(TypeError):                                   # the request's first five are required keywords
        pkg.ltsva_families(*args, rij=rij, mdccm_min=0.5)
    with pytest.raises(ValueError):                                  # too few elements
        pkg.ltsva_families(synthetic.make_stream(data[:2], FS), None, None, 65.5 / FS, 0.5, rij=rij[:, :2], **GOOD)
    fr = np.logspace(-1, 0.5, 16)
    nargs = ([10.0, 10.0], 0.5, 1.0, st, None, None, 2, np.zeros(16), np.zeros(16), np.array([0.5, 1.0, 2.0]), 'log', fr, 'butter', 2, 0.01)
    with pytest.raises(TypeError):
        pkg.narrow_band_least_squares_families(*nargs, rij=rij)
    for bad in bads[::3]:
        with pytest.raises(ValueError):
            pkg.narrow_band_least_squares_families(*nargs, rij=rij, **bad)
        with pytest.raises(ValueError):
            pkg.narrow_band_least_squares_families_batch(*nargs[:3], [st, st], *nargs[4:], rij=rij, **bad)
    z = np.zeros((2, 5))
    lat = dict(vel=z, baz=z, mdccm=z, sigma_tau=None, nwin=[5, 5], winlens=[40, 60], incs=[20, 30])
    for bad in (dict(nwin=[6, 5]), dict(winlens=[40]), dict(incs=[0, 30]), dict(sigma_tau=z), dict(vel=z[:1]), dict(nseg=2)):
        with pytest.raises(ValueError):
            pkg.label_families(**dict(lat, **bad), **GOOD)
    for bad in (dict(sigma_tau_max=0.5), dict(time_reach=0), dict(nope=1)):
        with pytest.raises(ValueError):
            pkg.label_families(**lat, **dict(GOOD, **bad))
    with pytest.raises(ValueError):
        pkg.label_families(**lat, **{k: v for k, v in GOOD.items() if k != 'vel_min'})


def test_makefile_and_resource_report(tmp_path):
    """csrc/families.hip is built without contraction like the other opt-ins and listed for both libraries; none of its eight
    kernels has a private segment or spills a register, only the three scan kernels hold LDS (256 counters), and the
    union kernel stays within 64 VGPRs (DESIGN.md section 26.2 records the counts)."""
    mk = open(os.path.join(LIBDIR, 'Makefile'), encoding='utf-8').read()
    assert 'families.o' in re.search(r'^OBJS = (.*)$', mk, re.M).group(1).split()
    assert 'families.hip' in re.search(r'^DEVSRC = (.*)$', mk, re.M).group(1).split()
    rule = re.search(r'^families\.o: (.*)\n\t(.*)$', mk, re.M)
    trace = re.search(r'^kept\.o: (.*)\n\t(.*)$', mk, re.M)
    assert rule and '$(NOFMA)' in rule.group(2) and rule.group(2).replace(' $(NOFMA)', '') == trace.group(2)
    for dep in ('families.hip', 'nbls_internal.h', 'dev_buf.h', '../../include/nbls.h'):
        assert dep in rule.group(1).split(), dep
    hipcc = '/opt/rocm/bin/hipcc'                                        # (the compiler the Makefile names: no skip without it)
    out = tmp_path / 'families.s'
    subprocess.run([hipcc, '-O3', '-std=c++17', '--offload-arch=gfx950', '-I' + LIBDIR, '-S', '--cuda-device-only',
                    os.path.join(LIBDIR, 'families.hip'), '-o', str(out), '-ffp-contract=off'], check=True,
                   stderr=subprocess.DEVNULL, timeout=900)
    text = out.read_text()
    found = dict(re.findall(r'\.amdhsa_kernel (\S*family_\w+_kernel\S*)(.*?)\.end_amdhsa_kernel', text, re.S))
    names = sorted(re.search(r'family_(\w+)_kernel', n).group(1) for n in found)
    assert names == ['flatten', 'ids', 'init', 'label', 'peak', 'scan', 'sums', 'union']
    for name, body in found.items():
        kind = re.search(r'family_(\w+)_kernel', name).group(1)
        assert int(re.search(r'\.amdhsa_private_segment_fixed_size (\d+)', body).group(1)) == 0, name
        assert int(re.search(r'\.amdhsa_next_free_vgpr (\d+)', body).group(1)) <= 64, name
        lds = int(re.search(r'\.amdhsa_group_segment_fixed_size (\d+)', body).group(1))
        assert lds == (1024 if kind in ('sums', 'scan', 'ids') else 0), name
    for key in ('vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size'):
        vals = re.findall(r'\.%s:\s+(\d+)' % key, text)
        assert len(vals) == 8 and all(int(v) == 0 for v in vals), (key, vals)
    assert '.uses_dynamic_stack: true' not in text and 'scratch_' not in text
    # every access to the parent array in the union kernel is an atomic: its only plain loads are those of the inputs
    body = text[text.index('family_union_kernel'):]
    body = body[:body.index('s_endpgm')]
    assert len(re.findall(r'global_atomic_cmpswap', body)) >= 2 and len(re.findall(r'global_load_dword v\d+, .* sc1', body)) >= 3


# ---- planner.family_table on hand-made families ----

def _table(rows):
    return np.array(rows, dtype=np.int64).reshape(-1, 8)


def test_family_table_circular_mean_across_north():
    family = np.array([[0, 0, -1, -2]], dtype=np.int32)
    baz = np.array([[359.0, 1.0, 90.0, 90.0]])
    vel = np.array([[0.3, 0.4, 9.0, 9.0]])
    md = np.array([[0.6, 0.8, 0.9, 0.9]])
    sig = np.array([[0.01, 0.03, 9.0, 9.0]])
    t = planner.family_table(family, _table([2, 0, 1, 0, 0, 0, 0, 60]), vel, baz, md, sig, [(0.5, 1.0)], [40], [20], FS, 100.0)
    assert len(t['count']) == 1 and t['count'][0] == 2
    assert min(t['baz_mean'][0], 360.0 - t['baz_mean'][0]) < 1e-9            # 0 degrees, not 180
    R = np.cos(np.deg2rad(1.0))
    assert abs(t['baz_std'][0] - np.rad2deg(np.sqrt(-2.0 * np.log(R)))) < 1e-9
    assert abs(t['vel_mean'][0] - 0.35) < 1e-15 and abs(t['vel_std'][0] - 0.05) < 1e-15
    assert t['mdccm_median'][0] == 0.7 and t['mdccm_peak'][0] == 0.8 and t['sigma_tau_median'][0] == 0.02
    assert (t['peak_band'][0], t['peak_window'][0], t['peak_baz'][0], t['peak_vel'][0]) == (0, 1, 1.0, 0.4)
    assert (t['t_start'][0], t['t_end'][0], t['f_lo'][0], t['f_hi'][0]) == (0.0, 3.0, 0.5, 1.0)
    assert t['t_start_datenum'][0] == 100.0 and t['t_end_datenum'][0] == 100.0 + 3.0 / 86400.0


def test_family_table_single_cell_family_peak_tie_and_segments():
    # 2 bands x 2 recordings (rows b * 2 + s), 3 windows; family 0 a single cell of recording 1, family 1 three cells of
    # recording 0 over both bands with a tie of the peak MdCCM
    family = np.array([[-1, 1, 1], [0, -1, -1], [-1, -1, 1], [-1, -1, -1]], dtype=np.int32)
    vel = np.full((4, 3), 0.34)
    baz = np.array([[0, 10.0, 20.0], [77.0, 0, 0], [0, 0, 30.0], [0, 0, 0]])
    md = np.array([[0, 0.9, 0.7], [0.6, 0, 0], [0, 0, 0.9], [0, 0, 0]])
    table = _table([[1, 3, 3, 0, 0, 1, 0, 40], [3, 1, 1, 0, 1, 0, 20, 140]])
    t = planner.family_table(family, table, vel, baz, md, None, [(0.5, 1.0), (1.0, 2.0)], [40, 60], [20, 40], FS, [100.0, 200.0])
    assert t['count'].tolist() == [1, 3] and t['segment'].tolist() == [1, 0]
    assert t['baz_mean'][0] == pytest.approx(77.0, abs=1e-12) and t['baz_std'][0] == 0.0 and t['vel_std'][0] == 0.0
    assert t['mdccm_median'][0] == t['mdccm_peak'][0] == 0.6 and np.isnan(t['sigma_tau_median']).all()
    assert t['baz_mean'][1] == pytest.approx(20.0, abs=1e-9) and t['mdccm_median'][1] == 0.9
    assert (t['peak_band'][1], t['peak_window'][1], t['peak_baz'][1]) == (0, 1, 10.0)      # the tie goes to the table's (smallest) cell
    assert t['f_lo'].tolist() == [0.5, 0.5] and t['f_hi'].tolist() == [1.0, 2.0]
    assert t['t_start_datenum'].tolist() == [200.0, 100.0 + 1.0 / 86400.0]
    assert t['t_end'].tolist() == [2.0, 7.0]
    empty = planner.family_table(np.full((4, 3), -1, dtype=np.int32), _table([]), vel, baz, md, None, [(0.5, 1.0), (1.0, 2.0)], [40, 60],
                                 [20, 40], FS, 100.0)
    assert all(len(v) == 0 for v in empty.values())
    with pytest.raises(ValueError):
        planner.family_table(family, table[:1], vel, baz, md, None, [(0.5, 1.0), (1.0, 2.0)], [40, 60], [20, 40], FS, 100.0)


def test_family_table_on_a_truth_labelling():
    c = fc.random_grids()[2]
    fam, n, tab = ft.label(*fc.args_of(c))
    t = planner.family_table(fam, tab, c['vel'], c['baz'], c['mdccm'], c['sigma_tau'], [(0.1 * k, 0.1 * k + 0.1) for k in range(1, 7)],
                             c['winlen'], c['wininc'], FS, 0.0)
    for k in range(n):
        m = fam == k
        assert t['count'][k] == m.sum() and t['mdccm_peak'][k] == c['mdccm'][m].max()
        assert t['mdccm_median'][k] == np.median(c['mdccm'][m]) and t['sigma_tau_median'][k] == np.median(c['sigma_tau'][m])
        assert abs(t['vel_mean'][k] - c['vel'][m].mean()) < 1e-12 and abs(t['vel_std'][k] - c['vel'][m].std()) < 1e-12
        z = np.exp(1j * np.deg2rad(c['baz'][m])).mean()
        assert abs((t['baz_mean'][k] - np.rad2deg(np.angle(z)) + 180.0) % 360.0 - 180.0) < 1e-9


def test_split_of_a_batch_labelling():
    """A pass over k recordings numbers its families across all of them: ``engine.split_families`` gives every recording the
    labelling of a pass of its own."""
    c = fc.segments()
    rng = np.random.default_rng(12)
    c['mdccm'] = np.where(rng.random(c['mdccm'].shape) < 0.2, 0.25, c['mdccm'])        # (recordings that differ)
    fam, n, tab = ft.label(*fc.args_of(c))
    nb, k, vl = 3, 3, fam.shape[1]
    parts = engine.split_families(fam, tab, nb, k, vl)
    assert len(parts) == 3
    for j, (f, t) in enumerate(parts):
        rows = np.arange(nb) * k + j
        own = ft.label(c['par'], 1, c['winlen'], c['wininc'], c['nwin'][rows], c['vel'][rows], c['baz'][rows], c['mdccm'][rows])
        assert f.dtype == np.int32 and t.dtype == np.int64
        assert np.array_equal(f, own[0]) and np.array_equal(t, own[2]), j


def test_transient_waves_are_confined_in_time_and_frequency():
    rij = synthetic.array_geometry(4, 1.0)
    npts, fs = 4000, 20.0
    src = [(50.0, 0.34, 1.0, 40.0, 120.0, 0.5, 1.0)]
    quiet = synthetic.transient_waves(rij, npts, fs, [], snr_db=40.0, seed=5)
    x = synthetic.transient_waves(rij, npts, fs, src, snr_db=40.0, seed=5)
    assert x.shape == quiet.shape == (4, npts) and quiet.std() == pytest.approx(0.01, rel=0.05)
    t = np.arange(npts) / fs
    delay = np.abs(rij).sum(axis=0).max() / 0.34                         # no element sees the gate open earlier or later than this
    outside = (t < 40.0 - delay) | (t > 120.0 + delay)
    assert np.abs(x[:, outside]).max() < 0.06 and x[:, (t > 60.0) & (t < 100.0)].std() > 0.5
    f = np.fft.rfftfreq(npts, 1.0 / fs)
    p = (np.abs(np.fft.rfft(x, axis=1)) ** 2).sum(axis=0)
    assert p[(f >= 0.4) & (f <= 1.1)].sum() > 0.98 * p.sum()
    assert np.array_equal(x, synthetic.transient_waves(rij, npts, fs, src, snr_db=40.0, seed=5))
    two = synthetic.transient_waves(rij, npts, fs, src + [(200.0, 0.3, 0.5, 100.0, 180.0, 2.0, 3.0)], snr_db=40.0, seed=5)
    late = (t > 130.0) & (t < 170.0)
    assert two[:, late].std() == pytest.approx(0.5, rel=0.2) and x[:, late].std() < 0.02
