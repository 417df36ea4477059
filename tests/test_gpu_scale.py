"""Every result of the GPU path follows the amplitude of its input exactly: each case runs a plan once
on the trace as it is and once per transformation of tests/scale_cases.py — T1 every sample times 2^k, T2 channel i times
2^(k_i), T3 every sample negated — and holds every field the plan returns to the table there: the same bits, the exact
factor 2^(e k), or the sign.  No comparison has a tolerance; a difference is a bug.  k = -30 and +24 are the physical
scales (m/s against Pa, digitiser counts) and the contract; +-100 lies far outside the float range with every fourth-order
product of samples still inside 2^+-450 (tests/test_scale_cases.py checks the inputs, and that the float64 references obey
the relation on them).  The relation carries no truth of its own: one case goes through the oracle away from unit scale.
Each case prints the fields and cells it compared."""
import numpy as np
import pytest

import band_batch_cases as bb
import scale_cases as sc
from scale_cases import T1, T2
from test_gpu_capon import _against_reference as capon_check
from test_gpu_parity import _compare_ltsva
from narrow_band_least_squares_amd import engine, ltsva
from narrow_band_least_squares_amd.stream import Stream, Trace, Stats

pytestmark = pytest.mark.gpu

T0 = sc.T0
LAGS = dict(want_lag=True, want_cmax=True, want_z=True, want_uncert=True)


def _run(c, data, alpha, **kw):
    """One prefiltered call on ``data`` with the geometry and window of the set ``c``."""
    return engine.process(data, c['fs'], T0, c['rij'], [(None, None)], [c['winlen']], 0.5, alpha, prefiltered=True, **kw)


def _screen_summary(h):
    """Of every candidate record of the pass just run (``Handle.screen_records``: unit, sliding channel, partner) the two
    words that are functions of the int8 images alone, whatever the order the waves ran in: the screening maximum and the
    candidate threshold theta (f32 bits) -> (units, N, N, 2) int32.  The quantiser scales a channel window by QMAX over its
    own max |x| and theta is formed from quantised-domain sums, so a power of two on the window changes neither.  The
    candidate lists themselves are not compared: only the picked lags are the contract."""
    return np.ascontiguousarray(h.screen_records()[..., 4:6])


def _metamorphic(label, c, alpha, cases, seeded=False, impl=None, **kw):
    """The plan on the set's trace, then once per case on the transformed trace: every field by the table; through the
    screening correlator (``impl=3``) also the screening maxima and thresholds under every T1."""
    h = engine.get_handle()
    h.set_profiling(True)
    try:
        ref = _run(c, c['data'], alpha, **kw)
        if impl is not None:
            assert h.timings()['xcorr_impl'] == impl, h.timings()
        screen = _screen_summary(h) if impl == 3 else None
        assert screen is None or (screen.shape[0] == int(ref.nwin[0]) and screen.any())
        for name, T, k in cases:
            got = _run(c, sc.transform(c['data'], T, k), alpha, **kw)
            if impl is not None:
                assert h.timings()['xcorr_impl'] == impl, (name, h.timings())
            if screen is not None and T == T1:
                now = _screen_summary(h)
                bad = np.argwhere(now != screen)
                assert not len(bad), ('%s, %s: the screening maximum or theta of %d records differs, first (unit, i, j, word) %s: '
                                      '%s against %s' % (label, name, len(bad), bad[0].tolist(), now[tuple(bad[0])], screen[tuple(bad[0])]))
            nf, nc = sc.compare(ref, got, T, k, seeded=seeded, label='%s, %s:' % (label, name))
            assert nf >= 5 and nc > 0, (label, name, nf, nc)
            print('%s, %s: %d fields, %d cells%s' % (label, name, nf, nc, '; %d screening records' % (screen.size // 2)
                                                      if screen is not None and T == T1 else ''))
    finally:
        h.set_profiling(False)
    assert int(ref.nwin[0]) >= 3 and np.isfinite(ref.vel[0, :int(ref.nwin[0])]).all()
    return ref


# ---- the correlators -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alpha', [1.0, 0.5])
def test_screening_route(alpha):
    """6 elements, W = 600: the int8 screening correlator, its candidate records and the DMA verifier, under OLS and LTS,
    at all four k, per-channel gains and negation."""
    ref = _metamorphic('screening alpha=%g' % alpha, sc.prefiltered('screen'), alpha, sc.cases(), impl=3, **LAGS)
    assert ref.lag is not None and ref.cmax is not None and ref.z is not None and ref.vel_uncert is not None
    assert np.ptp(ref.lag[0, :int(ref.nwin[0])]) > 0


@pytest.mark.parametrize('name', ['long', 'groups'])
def test_slab_quantiser_and_partner_groups(name):
    """4 elements at W = 5000 (the slab quantiser) and 8 elements at W = 6000 (two partner groups)."""
    _metamorphic(name, sc.prefiltered(name), 1.0, sc.cases(ks=(-30, 100), t2=False), impl=3, **LAGS)


@pytest.mark.parametrize('impl', [1, 2])
def test_general_correlators(impl):
    """The VALU and the f64-MFMA correlator forced, 4 elements, W = 257."""
    _metamorphic('xcorr_impl=%d' % impl, sc.prefiltered('general'), 1.0, sc.cases(), impl=impl, xcorr_impl=impl, **LAGS)


@pytest.mark.parametrize('plan', ['bounded', 'seeded', 'refined'])
def test_bounded_seeded_and_refined_plans(plan):
    """8 elements, W = 257: the bounded-lag correlator, the seeded one behind its grid search, and the sub-sample refinement.
    ``lag_frac`` is the same bits under T1 and T2.  A lag seed is a beam maximum, which per-channel gains move: there T2
    compares nothing that follows from the lags (``seeded=True``)."""
    c = sc.prefiltered('plans')
    kw = dict(LAGS, want_subsample=True, want_consistency=True)
    if plan == 'bounded':
        kw.update(min_velocity=0.25)
    elif plan == 'seeded':
        kw.update(slowness_grid=bb.SEED_GRID, seed_halfwidths=[6])
    ref = _metamorphic(plan, c, 0.5, sc.cases(), seeded=plan == 'seeded', **kw)
    n = int(ref.nwin[0])
    assert ref.lag_frac is not None and np.any(ref.lag_frac[0, :n] != 0.0)
    assert sc.behaviour('lag_frac', T1) == sc.SAME and sc.behaviour('lag_frac', T2) == sc.SAME


# ---- the filter ----------------------------------------------------------------------------------------------------------
def test_raw_trace_through_the_filter():
    """Two zero-phase bands of different window length, tapered, the narrowest band of the filter tests among them: the
    fetched filtered samples are the unscaled ones times 2^k, or negated, exactly, and so every result behind them."""
    c = sc.raw()

    def call(data):
        res = engine.process(data, c['fs'], T0, c['rij'], sc.RAW_EDGES, sc.RAW_WINLENS, 0.5, 1.0, *sc.RAW_FILTER, want_beam=True,
                             **LAGS)
        return res, [res.handle.fetch_filtered(b) for b in range(len(sc.RAW_EDGES))]

    ref, filt = call(c['data'])
    assert [int(w) for w in ref.W] == [1200, 600] and all(np.abs(f).max() > 0 for f in filt)
    for name, T, k in sc.cases():
        got, gfilt = call(sc.transform(c['data'], T, k))
        nc = sum(sc.check_field('filtered', filt[b], gfilt[b], T, k, label='raw, %s, band %d:' % (name, b)) for b in range(2))
        assert nc == 2 * c['data'].size
        nf, cells = sc.compare(ref, got, T, k, label='raw, %s:' % name)
        print('raw, %s: filtered samples %d cells; %d fields, %d cells' % (name, nc, nf, cells))


# ---- the opt-in results ----------------------------------------------------------------------------------------------------
FAMILIES = dict(mdccm_min=0.2, vel_min=0.05, vel_max=50.0, baz_tol=180.0, vel_tol=50.0, min_pixels=1)


def _spectra(c):
    return dict(capon_grid=c['grid'], capon_freqs=[c['freq']], capon_snapshots=sc.EXTRAS_SHAPE[1:], want_capon_maps=True,
                want_capon_csdm=True, capon_peaks=3, capon_peak_floor=0.0, capon_cells=c['cells'], capon_music=(2, 0.05, True, True, True, 0.0),
                capon_clean=(6, 0.5, 0.02, True))


@pytest.mark.parametrize('taps', [0, 4])
def test_every_opt_in_result_in_one_plan(taps):
    """8 elements, W = 65, Ls 16, Hs 8, 129 grid points, LTS: beam and F, the grid search with its map, the closures, Capon
    and Bartlett with maps, matrix and 3 peaks, MUSIC with map, vectors and peaks, CLEAN-SC with its matrix, the kept
    elements (the beam, the element delays and the beam trace over them), the families — everything coexists in one plan
    (tests/test_gpu_refusals.py); once with whole-sample steering and once with 4 taps."""
    c = sc.extras(8)
    kw = dict(LAGS, want_beam=True, slowness_grid=c['grid'], want_grid_map=True, want_consistency=True, kept=(None, True, False),
              element_max_shift=4, element_delays_kept=True, want_beam_trace=dict(window='hann', kept=True), families=FAMILIES,
              beam_taps=taps, **_spectra(c))
    ref = _metamorphic('extras taps=%d' % taps, c, 0.5, sc.cases(ks=(-30, 24, 100), t2=True), **kw)
    names, _ = sc.batch_fields()
    absent = [f for f in names if f not in sc.CONFIG + ('lag_frac', 'weights') and getattr(ref, f, None) is None]
    assert not absent, 'the plan returned no %s' % absent
    n = int(ref.nwin[0])
    assert np.any(ref.beam_trace) and np.all(ref.capon_power[0, :n] > 0) and np.all(ref.music_eigenvalues[0, :n, 0] > 0)
    assert np.all(ref.clean_count[0, :n] > 0) and ref.family is not None and ref.family_table is not None
    for f in ('capon_csdm', 'clean_csdm'):                       # the sign the mirrored triangle carries: R = R^H, a real diagonal
        R = getattr(ref, f)[0, :n]
        assert np.array_equal(R, np.conj(np.swapaxes(R, 1, 2))) and not np.any(np.diagonal(R, axis1=1, axis2=2).imag), f


def test_spectra_of_32_elements():
    """The Capon, MUSIC and CLEAN-SC plan once more at the largest array (the wide-matrix paths of the kernels)."""
    c = sc.extras(32)
    _metamorphic('spectra N=32', c, 1.0, sc.cases(ks=(-30, 24, 100), t2=False), **_spectra(c))


def test_spectra_against_the_truth_at_seismic_scale():
    """The Capon plan of the 8-element set at k = -30 through the checker of tests/test_gpu_capon.py as it stands: the matrix
    against the long-double truth within its derived bound, which is built from the samples and scales with them, Hermitian
    bit for bit, and both spectra from that matrix.  With the oracle comparison below, the scaled side of the relation
    rests on a truth of its own."""
    c = sc.extras(8)
    x = sc.transform(c['data'], T1, -30)
    kw = _spectra(c)
    del kw['capon_music'], kw['capon_clean']
    res = _run(c, x, 1.0, **kw)
    worst = capon_check(res, x, c['grid'], sc.EXTRAS_SHAPE[1], sc.EXTRAS_SHAPE[2], 0.01, label='k=-30', freq=c['freq'])
    assert max(worst.values()) <= 1.0 and float(np.abs(res.capon_csdm).max()) < 2.0 ** -50


# ---- several traces, several scales ----------------------------------------------------------------------------------------
def test_recordings_of_different_scales_in_one_batch():
    """Three recordings of one array at 2^-30, 1 and 2^24 in one pass, two raw bands, everything of the batch on: each
    result is the single unscaled call of its recording, transformed by its own k.  Nothing leaks between recordings."""
    recs, rij, t0s = bb.recordings()
    ks = (-30, 0, 24)
    batch = engine.process_batch([list(sc.transform(recs[s], T1, ks[s])) for s in range(bb.S)], bb.FS, t0s, rij, bb.EDGES, bb.WINLENS,
                                 bb.OVERLAP, bb.ALPHA, *bb.FILTER, **bb.ALL_ON)
    for s in range(bb.S):
        single = engine.process(recs[s], bb.FS, t0s[s], rij, bb.EDGES, bb.WINLENS, bb.OVERLAP, bb.ALPHA, *bb.FILTER, **bb.ALL_ON)
        nf = nc = 0
        for f in bb.FIELDS:
            assert getattr(single, f) is not None and getattr(batch[s], f) is not None, f
            n = sc.check_field(f, getattr(single, f), getattr(batch[s], f), T1, ks[s], label='batch, recording %d (k=%+d):' % (s, ks[s]))
            nf, nc = nf + (n > 0), nc + n
        assert nf == len(bb.FIELDS)
        print('batch, recording %d (k=%+d): %d fields, %d cells' % (s, ks[s], nf, nc))


def _window_rows(res, idx):
    """The per-window fields of a one-band ``BandBatch`` at the windows ``idx`` -> dict."""
    vl = res.vel.shape[1]
    out = {}
    for f in sc.fields_of(res):
        v = getattr(res, f)
        if f not in sc.CONFIG and f != 'grids' and isinstance(v, np.ndarray) and v.shape[:2] == (1, vl):
            out[f] = v[0, idx]
    return out


@pytest.mark.parametrize('alpha', [1.0, 0.5])
def test_gain_step_inside_one_trace(oracle, alpha):
    """The second half of the screening trace times 2^40: a window's scale must not depend on its neighbour's.  Every window
    wholly inside one half equals the window of the unscaled call under the table (k = 0 before the step, 40 behind it);
    the whole stepped trace, the straddling windows among it, goes through the oracle with lags and maxima exact.  The
    screening maxima and thresholds of the windows inside a half are those of the unscaled call too: the verifier would
    repair the lags of a window quantised with its neighbour's scale, these words show it (tests/test_scale_cases.py holds the
    trace to a window behind the step whose neighbour's largest sample lies before it)."""
    c = sc.prefiltered('screen')
    data, half = sc.gain_step()
    before, after, across = sc.window_sides(data.shape[1], c['fs'], c['winlen'], 0.5, half)
    assert len(before) >= 2 and len(after) >= 2 and len(across) >= 1
    kw = dict(LAGS, want_beam=True)
    ref = _run(c, c['data'], alpha, **kw)
    screen_ref = _screen_summary(engine.get_handle())
    got = _run(c, data, alpha, **kw)
    screen_got = _screen_summary(engine.get_handle())
    assert screen_ref.shape == screen_got.shape == (int(ref.nwin[0]), c['N'], c['N'], 2)
    for name, idx, k in (('before', before, 0), ('behind', after, sc.GAIN_STEP)):
        nf, nc = sc.compare(_window_rows(ref, idx), _window_rows(got, idx), T1, k, label='gain step, windows %s the step:' % name)
        assert nf >= 10
        # the int8 image of a window is scaled by the window's own max |x|: the neighbour across the step does not enter
        assert np.array_equal(screen_ref[idx], screen_got[idx]), 'gain step: the screening records of windows %s %s the step differ' % (
            np.flatnonzero((screen_ref[idx] != screen_got[idx]).any(axis=(1, 2, 3))).tolist(), name)
        print('gain step alpha=%g, %d windows %s the step: %d fields, %d cells, %d screening records' % (
            alpha, len(idx), name, nf, nc, screen_ref[idx].size // 2))
    st = oracle.make_stream(np.array(data), c['fs'], starttime=T0)
    h = engine.get_handle()
    h.set_profiling(True)
    try:
        _compare_ltsva(oracle, c, st, c['winlen'], alpha)
        assert h.timings()['xcorr_impl'] == 3
    finally:
        h.set_profiling(False)
    print('gain step alpha=%g: %d windows across the step against the oracle' % (alpha, len(across)))


def _typed_stream(x, fs):
    st = Stream()
    for row in x:
        st.append(Trace(row, Stats(sampling_rate=fs, npts=x.shape[1], starttime=T0, latitude=None, longitude=None)))
    return st


@pytest.mark.parametrize('kind', ['int32', 'float32', 'fortran'])
def test_input_types(kind):
    """Digitiser counts as int32, float32 samples and a Fortran-ordered float64 array, through ``engine.process`` and through
    ``ltsva`` on a stream: the same bits as the call on the C-contiguous float64 copy."""
    c = sc.prefiltered('screen')
    x = {'int32': sc.counts_int32, 'float32': lambda: c['data'].astype(np.float32),
         'fortran': lambda: np.asfortranarray(c['data'])}[kind]()
    assert x.dtype != np.float64 or not x.flags.c_contiguous
    plain = np.ascontiguousarray(x, dtype=np.float64)
    ref, got = _run(c, plain, 0.5, **LAGS), _run(c, x, 0.5, **LAGS)
    nf, nc = sc.compare(ref, got, T1, 0, label='%s through process:' % kind)
    a = ltsva(_typed_stream(plain, c['fs']), None, None, c['winlen'], 0.5, 0.5, rij=c['rij'])
    b = ltsva(_typed_stream(x, c['fs']), None, None, c['winlen'], 0.5, 0.5, rij=c['rij'])
    assert len(a) == len(b) == 8 and len(a[0]) == int(ref.nwin[0])
    for i in (0, 1, 2, 3, 5, 6, 7):
        assert sc.same_bits(a[i], b[i]), (kind, i)
    assert a[4].keys() == b[4].keys() and all(np.array_equal(a[4][key], b[4][key]) for key in a[4])
    print('%s: %d fields, %d cells through process; the 8 returns of ltsva' % (kind, nf, nc))


# ---- one truth away from unit scale ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('alpha', [1.0, 0.5])
def test_oracle_comparison_at_seismic_scale(oracle, alpha):
    """The screening case at k = -30 against the oracle, with the tolerances of the parity tests as they stand (every
    absolute one there sits on a quantity that carries no amplitude: a correlation maximum, a slowness, a lag)."""
    c = sc.prefiltered('screen')
    st = oracle.make_stream(sc.transform(c['data'], T1, -30), c['fs'], starttime=T0)
    h = engine.get_handle()
    h.set_profiling(True)
    try:
        _compare_ltsva(oracle, c, st, c['winlen'], alpha)
        assert h.timings()['xcorr_impl'] == 3
    finally:
        h.set_profiling(False)
