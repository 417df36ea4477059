"""The band-pass stage (csrc/filter.hip) sample by sample against the long-double DF2T truth of tests/filter_truth.py,
at every trace length and plan shape where its scan changes: the 512-sample chunk, the 16-sample LDS tile, the
16-chunk column tile of the matrix-core state kernel, the 64-chunk carry group (= one apply workgroup: beyond it the
group step M^len, a non-zero group-in state and the unmasked fast path of the apply kernel are in use), multi-band plans
whose 16-row weight tiles are partial or straddle bands, channel subsets, the option forms, the time-segmented path,
NaN samples at the seams — and the narrow bands of the baseline configurations, where SciPy's float64 sosfilt is no
reference any more and the bound is its own error times a margin measured on the CPU (filter_truth.NARROW_K).

Every truth is computed once per (filter, longest length) and kept at module scope.
"""
import functools

import numpy as np
import pytest

import filter_truth as ft
from narrow_band_least_squares_amd import engine, planner
from narrow_band_least_squares_amd._hip import Handle

pytestmark = pytest.mark.gpu

C, T, G = ft.constants()
LENGTHS = ft.boundary_lengths(C, T, G)
MB_LENGTHS = ft.multiband_lengths(C, T, G)
NOISE_ROWS = 2               # rows 0, 1: noise + in-band sinusoid; row 2: the crafted input of the case's length


@pytest.fixture(scope='module')
def handle():
    h = Handle(engine.default_device())
    yield h
    h.close()


def run_filter(h, x, sos, zero_phase, fs, options=(), row_step=0):
    """x (nchans, npts) through a filter-only plan of sos (B, S, 6) -> list of B arrays (nchans, npts)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    before = x.copy()
    nchans, npts = x.shape
    nb = sos.shape[0]
    tl, tr = planner.taper_ramps(npts)
    try:
        for key in options:
            h.set_option(key, 1)
        h.set_option('filter_row_step', row_step)
        h.set_trace(x, fs)
        h.plan(sos, zero_phase, tl, tr, [2] * nb, [max(1, npts)] * nb, 1)
        h.execute(stages=1)
        h.sync()
        out = [h.fetch_filtered(b) for b in range(nb)]
    finally:
        for key in options:
            h.set_option(key, 0)
        h.set_option('filter_row_step', 0)
    np.testing.assert_array_equal(x, before)               # the input rows are untouched
    for y in out:
        assert y.shape == (nchans, npts)                    # exactly npts samples per row (the padded tail is not returned)
    return out


def assert_close(y, truth, tol, what):
    scale = float(np.max(np.abs(truth)))
    err = float(np.max(np.abs(y.astype(np.longdouble) - truth)))
    assert np.isfinite(err), what
    assert err <= tol * scale, '%s: max |gpu - truth| = %.3e = %.3e of max |truth|' % (what, err, err / scale if scale else np.inf)


# ---- 1. one band, every boundary length, every kind of filter, the option forms ----
@functools.lru_cache(maxsize=None)
def _boundary_case(name):
    """-> (sos, zero_phase, {n: input (3, n)}, {n: truth (3, n)})"""
    ftype, lo, hi, order, zero_phase = ft.FILTERS[name]
    sos = ft.design(ftype, lo, hi, order, ft.FS)
    nmax = max(LENGTHS)
    x = np.zeros((NOISE_ROWS + len(LENGTHS), nmax))
    x[:NOISE_ROWS] = ft.noise_with_tone(sum(map(ord, name)), NOISE_ROWS, nmax, ft.FS, lo, hi)
    for i, n in enumerate(LENGTHS):
        x[NOISE_ROWS + i, :n] = ft.crafted(n, C, G)        # (zeros behind its end: they do not reach the prefix)
    rows = {n: list(range(NOISE_ROWS)) + [NOISE_ROWS + i] for i, n in enumerate(LENGTHS)}
    truth = ft.truth_of_prefixes(sos, x, zero_phase, LENGTHS, rows_of=rows.__getitem__)
    return sos, zero_phase, {n: np.ascontiguousarray(x[rows[n], :n]) for n in LENGTHS}, truth


@pytest.mark.parametrize('npts', LENGTHS)
@pytest.mark.parametrize('name', list(ft.FILTERS))
def test_filter_at_every_boundary_length(handle, name, npts):
    """No length of the list is refused by the API (a one-sample trace is a plan of one chunk and no window)."""
    sos, zero_phase, inputs, truth = _boundary_case(name)
    x, want = inputs[npts], truth[npts]
    assert want.shape == (NOISE_ROWS + 1, npts)
    y = run_filter(handle, x, sos[None], zero_phase, ft.FS)[0]
    assert_close(y, want, ft.TOL, '%s npts=%d' % (name, npts))
    if name in ft.TWO_SECTION:
        scale = float(np.max(np.abs(want)))
        for form, keys in ft.FORMS.items():
            z = run_filter(handle, x, sos[None], zero_phase, ft.FS, options=keys)[0]
            assert_close(z, want, ft.TOL, '%s npts=%d %s' % (name, npts, form))
            assert np.max(np.abs(z - y)) <= ft.TOL_FORMS * scale, (name, npts, form)


# ---- 2. several bands in one plan, channel subsets ----
@functools.lru_cache(maxsize=None)
def _multiband_case(k):
    """Nine bands x eight channels -> (sos (9, S, 6), zero_phase, input (8, nmax), {n: truth (9, 8, n)})"""
    ftype, order, zero_phase = ft.MULTIBAND_FILTERS[k]
    sos = np.stack([ft.design(ftype, lo, hi, order, ft.FS) for lo, hi in ft.MULTIBAND_EDGES])
    assert sos.shape == (9, order, 6)
    nch, nmax = max(ft.MULTIBAND_NCHANS), max(MB_LENGTHS)
    x = ft.noise_with_tone(500 + k, nch, nmax, ft.FS, 1.0, 2.0)
    x[2] += np.pad(ft.crafted(G * C + 1, C, G), (0, nmax - (G * C + 1)))
    per_series = np.repeat(sos, nch, axis=0)                 # series (band, channel), band-major
    truth = ft.truth_of_prefixes(per_series, np.tile(x, (9, 1)), zero_phase, MB_LENGTHS)
    return sos, zero_phase, x, {n: t.reshape(9, nch, n) for n, t in truth.items()}


@pytest.mark.parametrize('npts', MB_LENGTHS)
@pytest.mark.parametrize('nchans', ft.MULTIBAND_NCHANS)
@pytest.mark.parametrize('nbands', ft.MULTIBAND_NBANDS)
@pytest.mark.parametrize('k', range(len(ft.MULTIBAND_FILTERS)), ids=['%s%d' % f[:2] for f in ft.MULTIBAND_FILTERS])
def test_filter_multi_band_plans(handle, k, nbands, nchans, npts):
    """B * 2S weight rows in tiles of 16: 2 to 72 rows — tiles that are partial, that end on a band and that straddle
    bands.  Every band against its own truth; then the same plan filtered channel by channel (filter_row_step 1:
    launches with ch0 > 0), which changes nothing (every series is independent)."""
    sos, zero_phase, x, truth = _multiband_case(k)
    xin = np.ascontiguousarray(x[:nchans, :npts])
    out = run_filter(handle, xin, np.ascontiguousarray(sos[:nbands]), zero_phase, ft.FS)
    assert len(out) == nbands
    for b in range(nbands):
        assert_close(out[b], truth[npts][b, :nchans], ft.TOL, 'band %d of %d' % (b, nbands))
    by_row = run_filter(handle, xin, np.ascontiguousarray(sos[:nbands]), zero_phase, ft.FS, row_step=1)
    for b in range(nbands):
        assert_close(by_row[b], truth[npts][b, :nchans], ft.TOL, 'band %d of %d, channel by channel' % (b, nbands))
        np.testing.assert_array_equal(by_row[b], out[b])


# ---- 3. NaN samples at the seams ----
def test_nan_at_chunk_and_group_seams_matches_sosfilt(handle):
    """A NaN at C-1, at C and at G*C (a channel each) of a causal filter: NaN from there on and nowhere else, exactly
    as sosfilt propagates it; the finite samples inside the tolerance."""
    name = 'cheby1_2s_causal'
    ftype, lo, hi, order, zero_phase = ft.FILTERS[name]
    sos = ft.design(ftype, lo, hi, order, ft.FS)
    npts = (G + 1) * C + 1
    x = ft.noise_with_tone(77, 3, npts, ft.FS, lo, hi)
    at = (C - 1, C, G * C)
    for ch, p in enumerate(at):
        x[ch, p] = np.nan
    y = run_filter(handle, x.copy(), sos[None], zero_phase, ft.FS)[0]
    ref = ft.scipy_float64(sos, x, zero_phase)
    truth = ft.df2t_truth(sos, x, zero_phase)
    for ch, p in enumerate(at):
        finite = np.isfinite(ref[ch])
        assert finite[:p].all() and not finite[p:].any()
        np.testing.assert_array_equal(np.isfinite(y[ch]), finite)
        np.testing.assert_array_equal(np.isnan(y[ch]), np.isnan(ref[ch]))
        np.testing.assert_array_equal(np.isfinite(truth[ch]), finite)
        assert_close(y[ch, :p], truth[ch, :p], ft.TOL, 'NaN at %d' % p)


# ---- 4. the time-segmented path ----
@pytest.mark.parametrize('nseg', [2, 3])
@pytest.mark.parametrize('name', ['cheby1_2s_causal', 'butter_2s_zero_phase'])
def test_filter_in_time_segments(handle, name, nseg):
    """nbls_filter_segment: the trace in two and in three segments cut at whole chunks, the state handed on."""
    ftype, lo, hi, order, zero_phase = ft.FILTERS[name]
    sos = ft.design(ftype, lo, hi, order, ft.FS)
    npts = (G + 6) * C + 37
    seg = {2: (G // 2 + 8) * C, 3: (G // 2 - 2) * C}[nseg]
    assert (npts + seg - 1) // seg == nseg
    x = ft.noise_with_tone(88 + nseg, 3, npts, ft.FS, lo, hi)
    x[2] = ft.crafted(npts, C, G)
    before = x.copy()
    y = engine.filter_band_segmented(handle, [np.ascontiguousarray(r) for r in x], ft.FS, sos, zero_phase, seg)
    np.testing.assert_array_equal(x, before)
    assert y.shape == x.shape
    assert_close(y, ft.df2t_truth(sos, x, zero_phase, taper=False), ft.TOL, '%s in %d segments' % (name, nseg))


@pytest.mark.parametrize('nseg', [2, 3])
@pytest.mark.parametrize('zero_phase', [False, True], ids=['causal', 'zero_phase'])
def test_narrow_band_in_time_segments(handle, zero_phase, nseg):
    """The same with cfg-5's first band (0.1-0.1031 Hz at 20 Hz).  At the wide bands above M = A^512 is zero to
    rounding, so a wrong power of M in the state that leaves a segment (M^len of a group shorter than 64 chunks) cannot
    show; here the spectral radius of M is 0.84 and it does.  Bound: that of the narrow-band cases (the segments are
    the same scan, cut at chunk seams)."""
    i = 5
    ftype, lo, hi, order, fs = ft.NARROW_BANDS[i]
    assert (ftype, lo, hi, fs) == ('butter', 0.1, 0.1031, 20.0)
    sos = ft.design(ftype, lo, hi, order, fs)
    npts = (G + 6) * C + 37
    seg = {2: (G // 2 + 8) * C, 3: (G // 2 - 2) * C}[nseg]
    assert (npts + seg - 1) // seg == nseg
    x = ft.noise_with_tone(188 + nseg, 3, npts, fs, lo, hi)
    truth = ft.df2t_truth(sos, x, zero_phase, taper=False)
    e_ref = ft.rel_err(ft.scipy_float64(sos, x, zero_phase, taper=False), truth)
    y = engine.filter_band_segmented(handle, [np.ascontiguousarray(r) for r in x], fs, sos, zero_phase, seg)
    e_gpu = ft.rel_err(y, truth)
    print('\nNARROW-SEGMENTS %d %-10s e_ref %.2e  e_gpu %.2e  bound %.2e' % (
        nseg, 'zero-phase' if zero_phase else 'causal', e_ref, e_gpu, ft.narrow_bound(e_ref)))
    assert np.isfinite(e_gpu)
    assert e_gpu <= ft.narrow_bound(e_ref)


# ---- 5. narrow bands ----
@functools.lru_cache(maxsize=None)
def _narrow_forward(i):
    ftype, lo, hi, order, fs = ft.NARROW_BANDS[i]
    sos = ft.design(ftype, lo, hi, order, fs)
    x = ft.narrow_input(i)
    return sos, x, ft.df2t_forward(sos, x)


@functools.lru_cache(maxsize=None)
def _narrow_truth(i, zero_phase):
    sos, x, fwd = _narrow_forward(i)
    return ft.truth_of_prefixes(sos, x, zero_phase, ft.NARROW_LENGTHS, forward=fwd)


@pytest.mark.parametrize('npts', ft.NARROW_LENGTHS)
@pytest.mark.parametrize('i,zero_phase', ft.narrow_cases(),
                         ids=['%s_%g-%g_fs%g_%s' % (ft.NARROW_BANDS[i][0], ft.NARROW_BANDS[i][1], ft.NARROW_BANDS[i][2],
                                                    ft.NARROW_BANDS[i][4], 'zero_phase' if zp else 'causal')
                              for i, zp in ft.narrow_cases()])
def test_narrow_bands_against_the_truth(handle, i, zero_phase, npts):
    """e_gpu <= K e_ref + 64 eps, all three errors against the long-double truth as fractions of max |truth|: e_ref =
    SciPy's float64 sosfilt (the oracle's filter_data), e_emu = the float64 restatement of the chunked scan (printed:
    it tells an algorithmic limit from a kernel bug), e_gpu = the kernels.  K = filter_truth.NARROW_K comes from the
    CPU (tests/test_filter_truth.py), never from e_gpu."""
    sos, x, _ = _narrow_forward(i)
    fs = ft.NARROW_BANDS[i][4]
    truth = _narrow_truth(i, zero_phase)[npts]
    xin = np.ascontiguousarray(x[:, :npts])
    e_ref = ft.rel_err(ft.scipy_float64(sos, xin, zero_phase), truth)
    e_emu = ft.rel_err(ft.chunked_float64(sos, xin, zero_phase), truth)
    y = run_filter(handle, xin, sos[None], zero_phase, fs)[0]
    e_gpu = ft.rel_err(y, truth)
    print('\nNARROW %-7s %g-%g Hz order %d fs %g %-10s npts %6d  e_ref %.2e  e_emu %.2e  e_gpu %.2e  bound %.2e' % (
        ft.NARROW_BANDS[i][0], ft.NARROW_BANDS[i][1], ft.NARROW_BANDS[i][2], ft.NARROW_BANDS[i][3], fs,
        'zero-phase' if zero_phase else 'causal', npts, e_ref, e_emu, e_gpu, ft.narrow_bound(e_ref)))
    assert np.isfinite(e_gpu)
    assert e_gpu <= ft.narrow_bound(e_ref)
