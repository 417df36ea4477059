"""Each element's delay against the beam of the others (``nbls_set_element_delays``, csrc/element_delay.hip; DESIGN.md section
23) against tests/element_delay_truth.py: the results within the derived long-double bounds at the GPU's own solved
slowness, at every shape where the kernel's loops change, and bit-equality between the forms of a pass."""
import os
import subprocess
import sys

import numpy as np
import pytest

import element_delay_cases as cases
import element_delay_truth as edt
import test_element_delay_truth as demo_cpu
from narrow_band_least_squares_amd import (engine, planner, synthetic, _hip, ltsva, ltsva_element_delays,
                                           ltsva_element_delays_batch, narrow_band_least_squares,
                                           narrow_band_least_squares_element_delays, get_freqlist, get_winlenlist)

pytestmark = pytest.mark.gpu

FS, T0 = cases.FS, cases.T0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ('element_delay', 'element_cc', 'element_shift')
PLAIN = ('vel', 'baz', 'mdccm', 'sigma_tau', 'mask')


def _same(a, b, keys, label=''):
    for k in keys:
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and x.dtype == y.dtype, (label, k)
        assert x.tobytes() == y.tobytes() or np.array_equal(x, y, equal_nan=True), (label, k)


class _options:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        for k, v in self.kw.items():
            engine.get_handle().set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            engine.get_handle().set_option(k, 192 if k == 'screen_batch_mb' else 0)


def _process(data, rij, W, K, alpha=1.0, overlap=0.0, **kw):
    kw = dict(dict(want_z=True), **kw)
    res = engine.process(data, FS, T0, rij, [(None, None)], [(W + 0.5) / FS], overlap, alpha, prefiltered=True, element_max_shift=K,
                         **kw)
    assert int(res.W[0]) == W
    return res


def _against_truth(res, filt, K, label='', band=0, kept=False):
    """The three grids of a band against (b) at the GPU's own z (and dropped masks); prints the worst fraction of a bound."""
    n, W, inc = int(res.nwin[band]), int(res.W[band]), int(res.inc[band])
    refs = edt.row_reference(filt, FS, res.xij, res.z[band], W, inc, n, K, res.dropped_mask[band] if kept else None)
    got = [getattr(res, k)[band, :n] for k in FIELDS]
    vals, ties, worst = edt.check_units(refs, *got)
    print('%s N=%d W=%d K=%d: %d windows, %d values, %d through a near-tie; worst fraction of a bound %.3g'
          % (label, filt.shape[0], W, K, n, vals, ties, worst))
    for k in FIELDS:
        assert not getattr(res, k)[band, n:].any()                           # cells beyond nwin are zeros
    return refs


# ---- the shapes ----

@pytest.mark.parametrize('kind', ['noise', 'wave'])
@pytest.mark.parametrize('shape', cases.SHAPES, ids=lambda s: 'N%d-W%d-K%d' % s)
def test_shapes_against_the_truth(shape, kind):
    N, W, K = shape
    data, rij = cases.trace(N, W, kind)
    res = _process(data, rij, W, K)
    assert int(res.nwin[0]) >= 19
    _against_truth(res, data, K, kind)
    if kind == 'wave':                                                       # the pick means something: a coherent wave
        n = int(res.nwin[0])
        assert np.median(res.element_cc[0, :n]) > 0.5


@pytest.mark.parametrize('kind', ['noise', 'wave'])
@pytest.mark.parametrize('pair', [cases.BOUNDARY[0:2], cases.BOUNDARY[2:4], cases.BOUNDARY[4:6]], ids=['W-K256', 'W-K100', 'K-W200'])
def test_both_sides_of_the_staged_global_boundary(pair, kind):
    lib = _hip.load_library()
    (N, W0, K0), (_, W1, K1) = pair
    assert lib.nbls_element_delay_lds_bytes(N, W0, K0) == (N * (W0 + 2 * K0) + W0) * 8 > 0
    assert lib.nbls_element_delay_lds_bytes(N, W1, K1) == 0 and (N * (W1 + 2 * K1) + W1) * 8 > 156 * 1024
    for N, W, K in pair:
        data, rij = cases.trace(N, W, kind)
        res = _process(data, rij, W, K)
        _against_truth(res, data, K, kind + (' staged' if lib.nbls_element_delay_lds_bytes(N, W, K) else ' global'))


@pytest.mark.parametrize('shape', [(4, 65, 2), (8, 257, 8), (9, 513, 7), (32, 65, 7), (8, 1025, 1)], ids=lambda s: 'N%d-W%d-K%d' % s)
def test_staged_and_global_forms_give_the_same_bits(shape):
    N, W, K = shape
    for kind in ('noise', 'wave'):
        data, rij = cases.trace(N, W, kind)
        with _options(element_delay_form=1):
            staged = _process(data, rij, W, K)
        with _options(element_delay_form=2):
            glob = _process(data, rij, W, K)
        auto = _process(data, rij, W, K)
        _same(staged, glob, FIELDS + PLAIN, 'forms')
        _same(staged, auto, FIELDS + PLAIN, 'automatic')
        n = int(staged.nwin[0])
        assert np.any(staged.element_delay[0, :n] != 0) and np.isfinite(staged.element_cc[0, :n]).any()
        if kind == 'noise':
            assert np.any(staged.element_shift != 0)


@pytest.mark.parametrize('shape', [(4, 65, 2), (8, 257, 7), (8, 257, 8), (9, 513, 0), (32, 65, 1), (32, 109, 256)], ids=lambda s: 'N%d-W%d-K%d' % s)
def test_one_and_four_shifts_per_item_give_the_same_bits(shape):
    """Option ``element_delay_chunk``: a wave takes one shift or four consecutive ones of an element together (2K + 1 = 1, 3,
    5, 15, 17, 513: whole chunks, a last chunk of one, two and three shifts); either way, in either form, the same bits."""
    N, W, K = shape
    staged_fits = _hip.load_library().nbls_element_delay_lds_bytes(N, W, K) > 0
    for kind in ('noise', 'wave'):
        data, rij = cases.trace(N, W, kind)
        four = _process(data, rij, W, K)
        for form in ((1, 2) if staged_fits else (2,)):
            with _options(element_delay_chunk=1, element_delay_form=form):
                one = _process(data, rij, W, K)
            _same(one, four, FIELDS + PLAIN, 'chunk 1, form %d' % form)
        with _options(element_delay_chunk=4, element_delay_form=2):
            _same(_process(data, rij, W, K), four, FIELDS + PLAIN, 'chunk 4, global')
    with pytest.raises(ValueError):
        engine.get_handle().set_option('element_delay_chunk', 2)


def test_forced_staged_form_is_refused_where_it_does_not_fit():
    N, W, K = cases.BOUNDARY[1]
    data, rij = cases.trace(N, W, 'noise')
    with _options(element_delay_form=1):
        with pytest.raises(ValueError, match='element_delay_form') as err:
            _process(data, rij, W, K)
        assert err.value.code == _hip.NBLS_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        engine.get_handle().set_option('element_delay_form', 3)


# ---- edges of the trace, NaN, dead channels ----

def test_windows_that_read_off_both_ends_of_the_trace():
    """K = 40 beside windows of 64 at the first and the last sample, and delays of several samples (an array of 2 km)."""
    N, W, K = 5, 64, 40
    rij = synthetic.array_geometry(N, 1.0)
    data = np.ascontiguousarray(synthetic.plane_wave(rij, 20 * W + 1, FS, 0.5, 4.0, baz_deg=60.0, snr_db=6.0, seed=31))
    res = _process(data, rij - rij.mean(axis=1, keepdims=True), W, K)
    refs = _against_truth(res, data, K, 'ends')
    n = int(res.nwin[0])
    assert (refs[0]['d'] - K).min() < 0 and n * W + refs[n - 1]['d'].max() + K > data.shape[1]


def test_nan_samples_nan_slowness_and_a_zero_channel():
    N, W, K = 4, 65, 3
    data, rij = cases.trace(N, W, 'wave')
    n = planner.window_plan(data.shape[1], FS, (W + 0.5) / FS, 0.0)[2]
    # a zero channel: NaN / NaN / 0 for itself in every window, the others finite
    dead = data.copy()
    dead[2] = 0.0
    res = _process(dead, rij, W, K)
    _against_truth(res, dead, K, 'zero channel')
    assert np.isnan(res.element_delay[0, :n, 2]).all() and np.isnan(res.element_cc[0, :n, 2]).all() and not res.element_shift[0, :n, 2].any()
    assert np.isfinite(np.delete(res.element_cc[0, :n], 2, axis=1)).all()
    # window 3 constant in every channel: every lag is 0, MAD(tau) = 0, and under LTS z is NaN — the bad unit: NaN / NaN / 0
    # for every element (an OLS plan solves z = 0 there, which is finite: the window is an ordinary one, all-zero shifts aside)
    for M in (N, 9):
        wave, geo = (data, rij) if M == N else cases.trace(M, W, 'wave')
        flat = wave.copy()
        flat[:, 3 * W:4 * W] = 1.0
        res = _process(flat, geo, W, K, alpha=0.5)
        assert np.isnan(res.z[0, 3]).all() and np.isfinite(res.z[0, 2]).all() and np.isfinite(res.z[0, 4]).all()
        assert res.element_delay.shape[2] == M
        assert np.isnan(res.element_delay[0, 3]).all() and np.isnan(res.element_cc[0, 3]).all() and not res.element_shift[0, 3].any()
        assert np.isfinite(res.element_cc[0, 2]).all() and np.isfinite(res.element_cc[0, 4]).all()
        _against_truth(res, flat, K, 'flat window, LTS')
    flat = data.copy()
    flat[:, 3 * W:4 * W] = 1.0
    res = _process(flat, rij, W, K)
    assert np.isfinite(res.z[0, 3]).all()
    _against_truth(res, flat, K, 'flat window, OLS')
    # a NaN sample: the windows that read it inside are NaN (their z is NaN already or their sums are), the neighbours
    # that read it in a halo alone lose the shifts that touch it
    nan = data.copy()
    nan[1, 5 * W + 1] = np.nan
    res = _process(nan, rij, W, K)
    _against_truth(res, nan, K, 'NaN sample')
    assert np.isnan(res.element_cc[0, 5]).all() and np.isfinite(res.element_cc[0, 6]).all()


# ---- the elements LTS kept ----

def _mistimed(N, npts, bad, seed=900):
    rij = synthetic.array_geometry(N, 1.0)
    data = synthetic.plane_wave(rij, npts, FS, 0.5, 4.0, baz_deg=60.0, snr_db=10.0, seed=seed, timing_error_s=0.25,
                                bad_element=bad)
    return np.ascontiguousarray(data), rij - rij.mean(axis=1, keepdims=True)


@pytest.mark.parametrize('bad', [0, 3, 7])
def test_kept_beam_with_the_first_a_middle_and_the_last_element_dropped(bad):
    N, W, K = 8, 257, 8
    data, rij = _mistimed(N, 20 * W + 1, bad)
    res = _process(data, rij, W, K, alpha=0.5, kept=(N - 1, False, False), element_delays_kept=True)
    n = int(res.nwin[0])
    named = res.dropped_mask[0, :n] == 1 << bad
    assert named.sum() >= n // 2, res.dropped_mask[0, :n]
    _against_truth(res, data, K, 'kept, element %d late' % bad, kept=True)
    if bad != 0:        # (element 0 is the time base: its own lateness is everybody else's earliness)
        assert abs(np.median(res.element_delay[0, :n][named, bad]) - 0.25) <= 1.0 / FS
    # the same pass without the flag: the full array's beam, other bits where an element is dropped
    full = _process(data, rij, W, K, alpha=0.5, kept=(N - 1, False, False))
    _against_truth(full, data, K, 'full beam on the same plan')
    assert np.any(full.element_cc[0, :n][named] != res.element_cc[0, :n][named])
    _same(full, res, PLAIN + ('dropped_mask', 'kept_count'), 'kept flag')


def test_kept_beam_falls_back_to_the_whole_array():
    """N = 4, q = 1: whatever LTS drops, fewer than 3 elements remain wherever a pair lost its weight: S is the array."""
    N, W, K = 4, 65, 3
    data, rij = _mistimed(N, 20 * W + 1, 3)
    res = _process(data, rij, W, K, alpha=0.5, kept=(1, False, False), element_delays_kept=True)
    n = int(res.nwin[0])
    assert np.any(res.dropped_mask[0, :n] != 0) and np.all(res.kept_count[0, :n][res.dropped_mask[0, :n] != 0] == N)
    _against_truth(res, data, K, 'fallback', kept=True)
    plain = _process(data, rij, W, K, alpha=0.5)
    _same(res, plain, FIELDS + PLAIN, 'fallback is the plain beam')


# ---- the forms of a pass ----

EDGES, WINLENS, FILTER = [(0.5, 2.0), (1.0, 4.0)], [257.5 / FS, 65.5 / FS], ('butter', 2, 0.01)
SHIFTS = [9, 4]
FORM_KW = dict(kept=(7, False, False), element_max_shift=SHIFTS, element_delays_kept=True)


def _recordings(npts=4801, S=3):
    rij = synthetic.array_geometry(8, 1.0)
    data = [np.ascontiguousarray(synthetic.plane_wave(rij, npts, FS, 0.5, 4.0, baz_deg=20.0 + 67.0 * i, snr_db=10.0, timing_error_s=0.25,
                                                      bad_element=(7, 0, 2)[i], seed=520 + i)) for i in range(S)]
    return data, rij - rij.mean(axis=1, keepdims=True), [T0 + 0.0173 * i for i in range(S)]


def _two_bands(data, rij, t0=T0, **kw):
    return engine.process(data, FS, t0, rij, EDGES, WINLENS, 0.5, 0.5, *FILTER, **dict(FORM_KW, **kw))


def test_batch_of_three_recordings_equals_three_single_calls():
    recs, rij, t0s = _recordings()
    batch = engine.process_batch([list(d) for d in recs], FS, t0s, rij, EDGES, WINLENS, 0.5, 0.5, *FILTER, **FORM_KW)
    for s in range(3):
        single = _two_bands(recs[s], rij, t0s[s])
        assert [int(w) for w in single.W] == [257, 65] and np.any(single.element_shift != 0)
        assert np.abs(single.element_shift[0]).max() <= 9 and np.abs(single.element_shift[1]).max() <= 4
        _same(batch[s], single, FIELDS + PLAIN, 'recording %d' % s)


@pytest.mark.parametrize('overlap', [1, -1])
def test_streamed_in_several_batches_equals_the_unstreamed_pass(monkeypatch, overlap):
    recs, rij, _ = _recordings(48001, 1)
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    whole = _two_bands(recs[0], rij)
    h = engine.get_handle()
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '1')
    try:
        h.set_option('screen_batch_mb', 1)
        h.set_option('solve_min_units', 1)
        h.set_option('overlap', overlap)
        streamed = _two_bands(recs[0], rij)
        nbatches = h.result_batches()
    finally:
        h.set_option('screen_batch_mb', 192)
        h.set_option('solve_min_units', 0)
        h.set_option('overlap', 0)
    assert nbatches >= 3, nbatches
    _same(streamed, whole, FIELDS + PLAIN, 'streamed')


def test_window_slices_add_up_to_the_full_call():
    recs, rij, _ = _recordings(2401, 1)
    full = _two_bands(recs[0], rij)
    parts = [_two_bands(recs[0], rij, window_slice=(k, 3)) for k in range(3)]
    for k in FIELDS:
        total = np.zeros_like(getattr(full, k))
        for p in parts:
            a = getattr(p, k)
            filled = (a != 0) | np.isnan(a) if a.dtype.kind == 'f' else a != 0
            assert not np.any(filled & (total != 0)), k                      # rows outside a slice stay zero
            total = total + np.nan_to_num(a) if a.dtype.kind == 'f' else total + a
        np.testing.assert_array_equal(total, np.nan_to_num(getattr(full, k)) if total.dtype.kind == 'f' else getattr(full, k), err_msg=k)


def test_two_band_rounds_equal_one(monkeypatch):
    recs, rij, _ = _recordings(2401, 1)
    one = _two_bands(recs[0], rij)
    per_band = 8.0 * 8 * (2401 + 64)
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', repr(1.5 * per_band / 2.0 ** 30))      # one band per round
    assert engine.max_bands_per_pass(8, 2401) == 1
    two = _two_bands(recs[0], rij)
    _same(two, one, FIELDS + PLAIN, 'band rounds')


def test_unchanged_beside_the_other_extras():
    """Beam, grid, Capon, closure, refinement and 8-tap interpolation in the same plan: the refinement moves z and with it
    the delays, so it is compared with a refined plan; everything else leaves the three grids bit for bit."""
    N, W, K = 8, 257, 8
    data, rij = cases.trace(N, W, 'wave')
    alone = _process(data, rij, W, K)
    grid = planner.slowness_grid(3.5, 11)
    many = _process(data, rij, W, K, want_beam=True, slowness_grid=grid, want_consistency=True, beam_taps=8, capon_grid=grid,
                    capon_freqs=[2.0], capon_snapshots=([64], [16]), want_beam_trace=True)
    _same(many, alone, FIELDS + PLAIN, 'extras')
    refined = _process(data, rij, W, K, want_subsample=True)
    both = _process(data, rij, W, K, want_subsample=True, want_beam=True, beam_taps=8)
    _same(both, refined, FIELDS + PLAIN, 'refined')
    _against_truth(refined, data, K, 'refined')


@pytest.mark.parametrize('picks', ['seeded', 'bounded'])
def test_seeded_and_bounded_picks(picks):
    N, W, K = 8, 257, 8
    data, rij = _mistimed(N, W * 8 + 1, 7)
    kw = dict(slowness_grid=planner.slowness_grid(3.5, 11), seed_halfwidths=6) if picks == 'seeded' else dict(min_velocity=0.3)
    res = _process(data, rij, W, K, alpha=0.5, kept=(N - 1, False, False), element_delays_kept=True, **kw)
    _against_truth(res, data, K, picks, kept=True)


# ---- on and off, refusals ----

def test_off_after_on_and_the_refusals_of_the_library():
    N, W, K = 5, 65, 3
    data, rij = cases.trace(N, W, 'wave')
    never = engine.process(data, FS, T0, rij, [(None, None)], [(W + 0.5) / FS], 0.0, 1.0, prefiltered=True)
    on = _process(data, rij, W, K)
    h = on.handle
    off = engine.process(data, FS, T0, rij, [(None, None)], [(W + 0.5) / FS], 0.0, 1.0, prefiltered=True)
    _same(off, never, PLAIN, 'off after on')
    _same(on, never, PLAIN, 'on')
    with pytest.raises(_hip.NblsError) as err:                       # the plan did not ask
        h.fetch_element_delays()
    assert err.value.code == _hip.NBLS_ERR_STATE
    ip = lambda *v: np.array(v, dtype=np.int32).ctypes.data_as(h.lib.nbls_set_element_delays.argtypes[1])
    for table, nb, flags in ((ip(3), 0, 0), (ip(-1), 1, 0), (ip(257), 1, 0), (ip(3), 1, 2), (ip(3), -1, 0)):
        assert h.lib.nbls_set_element_delays(h._h, table, nb, flags) == _hip.NBLS_ERR_ARG
    VL = on.grids.shape[2]
    plan = lambda: h.plan(None, False, None, None, [W], [W], VL)
    plan()
    with pytest.raises(_hip.NblsError):                              # the refused calls left the handle unchanged
        h.fetch_element_delays()
    try:
        h.set_element_delays([3, 3])                                 # two entries for a plan of one band
        with pytest.raises(ValueError) as err:
            plan()
        assert err.value.code == _hip.NBLS_ERR_ARG
        h.set_element_delays([3], kept=True)                         # KEPT without the kept elements
        with pytest.raises(_hip.NblsError, match='nbls_set_kept_elements') as err:
            plan()
        assert err.value.code == _hip.NBLS_ERR_STATE
        h.set_element_delays([3])
        plan()
        assert not any(a.any() for a in h.fetch_element_delays())    # zeros until a pass has run the solve stage
        h.execute(stages=3)
        assert not any(a.any() for a in h.fetch_element_delays())
        h.execute()
        got = h.fetch_element_delays()
        for a, k in zip(got, FIELDS):
            assert a.tobytes() == getattr(on, k).tobytes() or np.array_equal(a, getattr(on, k), equal_nan=True), k
        sub = [0, 1, 2, 3]                                           # further estimators are out of scope
        xs, ps, xp = planner.co_array(rij[:, sub])
        h.set_estimators([dict(kept=sub, xij=xs, pair_idx=ps, xpinv=xp, lts=None, eig6=None)])
        with pytest.raises(ValueError, match='nbls_set_estimators') as err:
            plan()
        assert err.value.code == _hip.NBLS_ERR_UNSUPPORTED
    finally:
        h.set_estimators(())
        h.set_element_delays(None)
    plan()
    with pytest.raises(_hip.NblsError):                              # switched off again
        h.fetch_element_delays()
    fresh = _hip.Handle(0)
    try:
        xij, pair_idx, xpinv = planner.co_array(rij)
        fresh.set_trace(data, FS)
        fresh.set_element_delays([3])
        with pytest.raises(_hip.NblsError) as err:                   # no geometry
            fresh.plan(None, False, None, None, [W], [W], VL)
        assert err.value.code == _hip.NBLS_ERR_STATE
        perm = np.arange(len(xij))
        perm[[0, 1]] = [1, 0]                                        # rows 0..N-2 are not the pairs (0, m)
        fresh.set_geometry(xij[perm], np.asarray(pair_idx)[perm], xpinv[:, perm])
        with pytest.raises(_hip.NblsError) as err:
            fresh.plan(None, False, None, None, [W], [W], VL)
        assert err.value.code == _hip.NBLS_ERR_STATE
    finally:
        fresh.set_element_delays(None)
        fresh.close()


def test_rccl_communicator_refuses_the_element_delays():
    """A communicator lives as long as its process: a child process over the tests' loopback transport."""
    src = os.path.join(ROOT, 'tests', 'c_caller', 'loopback_rccl.cpp')
    lib = os.path.join(ROOT, 'tests', 'c_caller', 'libloopback_rccl.so')
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.run(['/opt/rocm/bin/hipcc', '-O2', '-shared', '-fPIC', '--offload-arch=gfx950', src, '-o', lib], check=True,
                       timeout=300)
    env = dict(os.environ, NBLS_TEST_TRANSPORT=lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_element_delay_comm_worker.py')], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and 'ELEMENT_DELAY_COMM_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the demonstration and the public entry points ----

@pytest.fixture(scope='module')
def demo():
    rij = synthetic.array_geometry(8, 1.0)
    bad = demo_cpu._band(synthetic.plane_wave(rij, demo_cpu.NPTS, FS, 0.1, 5.0, snr_db=10.0, timing_error_s=0.25, bad_element=7))
    clean = demo_cpu._band(synthetic.plane_wave(rij, demo_cpu.NPTS, FS, 0.1, 5.0, snr_db=10.0))
    return dict(rij=rij, bad=np.ascontiguousarray(bad), clean=np.ascontiguousarray(clean))


def test_demonstration_statements_hold_on_the_gpu(demo):
    """The case of DESIGN.md section 20.4 through ``ltsva_element_delays``: the statements the CPU truth asserts, on the GPU's
    results; this window length takes the global form."""
    K = int(planner.element_shifts([0.55], FS)[0])
    assert _hip.load_library().nbls_element_delay_lds_bytes(8, demo_cpu.W, K) == 0
    args = (None, None, demo_cpu.W / FS, 0.5)
    kept = ltsva_element_delays(synthetic.make_stream(demo['bad'], FS), *args, alpha=0.5, rij=demo['rij'], max_shift=K, kept=True)
    full = ltsva_element_delays(synthetic.make_stream(demo['bad'], FS), *args, alpha=0.5, rij=demo['rij'], max_shift=K)
    clean = ltsva_element_delays(synthetic.make_stream(demo['clean'], FS), *args, alpha=0.5, rij=demo['rij'], max_shift=K, kept=True)
    assert len(kept) == 13 and len(full) == 11 and kept[8].shape == (demo_cpu.NWIN, 8) and kept[10].dtype == np.int32
    assert np.count_nonzero(kept[11] == 1 << 7) >= 18
    mk, mf, mc = demo_cpu.demonstration_medians(kept[8], full[8], clean[8])
    np.set_printoptions(precision=4, suppress=True)
    print('kept beam medians %s\nfull beam medians %s\nclean medians %s' % (mk, mf, mc))
    edt.demonstration_statements(mk, mf, mc, 7, 0.25, FS)
    plain = ltsva(synthetic.make_stream(demo['bad'], FS), *args, alpha=0.5, rij=demo['rij'])
    for a, b in zip(plain[:4], kept[:4]):
        np.testing.assert_array_equal(a, b)


def test_public_entry_points():
    N, W, K = 6, 257, 6
    rij = synthetic.array_geometry(N, 1.0)
    recs = [np.ascontiguousarray(synthetic.plane_wave(rij, 8 * W + 1, FS, 0.5, 4.0, baz_deg=40.0 + 90 * i, snr_db=10.0, seed=70 + i,
                                                      timing_error_s=0.25, bad_element=N - 1)) for i in range(2)]
    streams = [synthetic.make_stream(r, FS) for r in recs]
    args = (None, None, (W + 0.5) / FS, 0.5)
    singles = [ltsva_element_delays(s, *args, alpha=0.5, rij=rij, max_shift=K, kept=True) for s in streams]
    batch = ltsva_element_delays_batch(streams, *args, alpha=0.5, rij=rij, max_shift=K, kept=True)
    for one, two in zip(singles, batch):
        assert len(one) == len(two) == 13
        for a, b in zip(one[8:], two[8:]):
            assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)
    res = engine.process(recs[0], FS, T0, rij, [(None, None)], [(W + 0.5) / FS], 0.5, 0.5, prefiltered=True, want_z=True,
                         kept=(N - 1, False, False), element_max_shift=K, element_delays_kept=True)
    n = int(res.nwin[0])
    assert np.array_equal(singles[0][8], res.element_delay[0, :n], equal_nan=True)
    _against_truth(res, recs[0], K, 'ltsva_element_delays', kept=True)
    ols = ltsva_element_delays(streams[0], *args, rij=rij, max_shift=K)
    assert len(ols) == 11 and ols[8].shape == (n, N)
    # the narrow-band driver: the default range is half a period of every band's upper edge
    fmin, fmax, nb = 0.5, 4.0, 3
    freqlist, nbands, _ = get_freqlist(fmin, fmax, 'linear', nb)
    winlens = get_winlenlist('constant', nbands, 12.0, 12.0, 12.0)
    fr = np.logspace(-1, 0.5, 16)
    w, h = np.zeros(16), np.zeros(16)
    nargs = (winlens, 0.5, 0.5, streams[0], None, None, nbands, w, h, freqlist, 'linear', fr, 'butter', 2, 0.01)
    out = narrow_band_least_squares_element_delays(*nargs, rij=rij, kept=True)
    ref = narrow_band_least_squares(*nargs, rij=rij)
    assert len(out) == len(ref) + 1
    for a, b in zip(ref[:4], out[:4]):
        np.testing.assert_array_equal(a, b)
    d = out[-1]
    assert set(d) == {'element_delay', 'element_cc', 'element_shift', 'dropped_mask', 'kept_count'}
    shifts = planner.element_shifts([freqlist[i + 1] for i in range(nbands)], FS)
    for b in range(nbands):
        assert d['element_delay'].shape[0] == nbands and np.abs(d['element_shift'][b]).max() <= shifts[b]
        assert np.any(d['element_shift'][b] != 0) or shifts[b] == 0
