"""The beam trace at the windows' solved slowness (``nbls_set_beam_trace``, csrc/beam_trace.hip: beam_trace_kernel; DESIGN.md
section 21) on the GPU, against tests/beam_trace_truth.py on the GPU's own fetched filtered band, slowness, MdCCM and dropped
mask: bit for bit against the float64 restatement (a) everywhere, within the derived rounding bound of the long-double
reference (b) on general data, exactly the source signal on small-integer traces with designed whole-sample delays.  The
forms of a pass (streamed, batched, HBM rounds, the second solve stream, seeded and refined plans) bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

import beam_trace_cases as cases
import beam_trace_truth as bt
import solve_truth as st
from narrow_band_least_squares_amd import (engine, planner, synthetic, _hip, ltsva, ltsva_beam_trace, ltsva_beam_trace_batch,
                                           narrow_band_least_squares, narrow_band_least_squares_beam_trace)

pytestmark = pytest.mark.gpu

FS = cases.FS
T0 = 17884.0729166667
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = ('vel', 'baz', 'mdccm', 'sigma_tau', 'mask')


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _process(data, rij, W, alpha, trace=True, overlap=0.5, **kw):
    res = engine.process(data, FS, T0, rij, [(None, None)], [(W + 0.5) / FS], overlap, alpha, prefiltered=True, want_z=True,
                         want_beam_trace=trace, **kw)
    assert int(res.W[0]) == W
    return res


def _truth_args(res, filt, band=0):
    mask = None if res.dropped_mask is None else res.dropped_mask[band]
    return (filt, res.z[band], res.mdccm[band], int(res.nwin[band]), mask, res.xij, FS, int(res.W[band]), int(res.inc[band]))


def _restated(res, filt, g, gate=None, band=0, kept=False):
    args = list(_truth_args(res, filt, band))
    if not kept:
        args[4] = None
    return bt.restate(*args, g, gate)


def _wave(N, npts, mistimed=False, seed=900, snr_db=6.0):
    rij = synthetic.array_geometry(N, 1.0)
    data = synthetic.plane_wave(rij, npts, FS, 0.5, 4.0, baz_deg=60.0, snr_db=snr_db, timing_error_s=0.25 if mistimed else 0.0,
                                bad_element=N - 1 if mistimed else None, seed=seed)
    return np.ascontiguousarray(data), rij - rij.mean(axis=1, keepdims=True)


# ---- exact cases ----

def _exact(N, W, overlap, npts, scale, label):
    """Integer traces, boxcar: bit-equal to (a); equal to s wherever every window over the sample has the designed delays and
    reads inside the trace."""
    data, rij, s, D = cases.exact_trace(N, npts, scale)
    res = _process(data, rij, W, 1.0, 'boxcar', overlap)
    n, inc = int(res.nwin[0]), int(res.inc[0])
    got = res.beam_trace[0]
    assert res.beam_trace.shape == (1, npts)
    exp = _restated(res, data, np.ones(W))
    assert _bits(got, exp), (label, int(np.count_nonzero(got != exp)))
    designed = np.array([np.array_equal(bt.window_delays(res.xij, FS, res.z[0, w], N), D) for w in range(n)])
    cover, good = np.zeros(npts, dtype=int), np.zeros(npts, dtype=int)
    for w in range(n):
        cover[w * inc:w * inc + W] += 1
        good[w * inc:w * inc + W] += int(designed[w])
    idx = np.arange(npts)
    sure = (cover > 0) & (good == cover) & (idx + D.min() >= 0) & (idx + D.max() < npts)
    assert np.array_equal(got[sure], s[sure]), label
    assert np.all(got[cover == 0] == 0.0), label
    print('%s: N=%d W=%d inc=%d npts=%d, %d windows (%d with the designed delays), %d samples equal to s, %d uncovered'
          % (label, N, W, inc, npts, n, int(designed.sum()), int(sure.sum()), int(np.sum(cover == 0))))
    return res, designed, sure, cover, D


@pytest.mark.parametrize('N', cases.EXACT_N)
def test_exact_traces(N):
    res, designed, sure, cover, D = _exact(N, 200, 0.5, 2 * cases.TILE + 9, 1, 'exact')
    assert designed.all() and sure.sum() >= 2 * cases.TILE - 200       # the input does what it was made for


@pytest.mark.parametrize('case', cases.SEAMS, ids=[c[0].split(' (')[0] for c in cases.SEAMS])
def test_seams(case):
    label, N, W, overlap, npts, scale = case
    res, designed, sure, cover, D = _exact(N, W, overlap, npts, scale, label)
    n, inc = int(res.nwin[0]), int(res.inc[0])
    if W >= 64:
        assert designed.sum() >= n - 2 and sure.sum() >= (npts - 2 * W) // 2, label
    assert cover.max() == -(-W // inc)
    if 'tail' in label:
        assert np.sum(cover == 0) >= 16 and np.all(res.beam_trace[0][cover == 0] == 0.0)
    if 'both ends' in label:
        assert D.min() < 0 and (n - 1) * inc + W - 1 + D.max() >= npts and designed[0] and designed[-1]


@pytest.mark.parametrize('order', [(257, 65), (65, 257)])
def test_two_bands_with_different_window_lengths(order):
    """Filtered on the GPU, two bands of different W in either order: each band's trace on its own synthesis window, against
    both truths on the filtered, tapered samples the kernel read."""
    data, rij = _wave(4, 2401)
    res = engine.process(data, FS, T0, rij, [(0.5, 1.5), (1.5, 4.0)], [(order[0] + 0.5) / FS, (order[1] + 0.5) / FS], 0.5, 1.0,
                         'butter', 2, 0.01, want_z=True, want_beam_trace=True)
    assert [int(w) for w in res.W] == list(order) and res.beam_trace.shape == (2, 2401)
    for b in range(2):
        _against_both(res, res.handle.fetch_filtered(b), planner.beam_trace_window(order[b]), band=b, label='band %d' % b)


# ---- general data ----

def _against_both(res, filt, g, gate=None, band=0, kept=False, label=''):
    got = res.beam_trace[band]
    args = list(_truth_args(res, filt, band))
    if not kept:
        args[4] = None
    a = bt.restate(*args, g, gate)
    b, bound, cover = bt.reference(*args, g, gate)
    err = np.abs(got.astype(np.longdouble) - b).astype(np.float64)
    pos = bound > 0                                                  # (a sample whose every term is 0.0 has bound 0 and error 0)
    worst = float(np.max(err[pos] / bound[pos])) if np.any(pos) else 0.0
    print('%s: %d samples, %d covered, worst |gpu - b| / bound = %.3f, bit-equal to (a): %s'
          % (label, len(got), int(np.sum(cover > 0)), worst, _bits(got, a)))
    assert np.all(err <= bound), (label, worst)
    assert _bits(got, a), (label, int(np.count_nonzero(got != a)))
    assert np.all(got[cover == 0] == 0.0)
    return cover


@pytest.mark.parametrize('N,alpha,W,overlap', [(3, 1.0, 65, 0.5), (4, 0.5, 257, 0.75), (9, 0.5, 1200, 0.75), (8, 0.5, 200, 0.9)])
def test_general_data_against_both_truths(N, alpha, W, overlap):
    npts = {65: 1201, 257: 2401, 1200: 6001, 200: 2401}[W]
    data, rij = _wave(N, npts, mistimed=alpha < 1.0)
    res = _process(data, rij, W, alpha, 'hann', overlap)
    cover = _against_both(res, data, planner.beam_trace_window(W), label='N=%d W=%d' % (N, W))
    assert cover.max() == -(-W // int(res.inc[0])) and np.all(res.beam_trace[0][cover > 0] != 0.0)


# ---- the gate ----

def test_gate():
    """A wave in the first half of the trace, noise in the second: a threshold between the two MdCCM populations leaves the
    noise windows out; samples only they cover are exactly 0.0.  NaN switches the gate off."""
    N, W, npts = 6, 200, 4001
    data, rij = _wave(N, npts, snr_db=20.0)
    noise = np.random.default_rng(8).standard_normal((N, npts))
    data[:, npts // 2:] = noise[:, npts // 2:]
    plain = _process(data, rij, W, 1.0, 'hann')
    n, inc = int(plain.nwin[0]), int(plain.inc[0])
    md = plain.mdccm[0, :n]
    first, second = md[:n // 2 - 1], md[n // 2 + 1:]
    assert first.min() > second.max(), (first.min(), second.max())
    gate = 0.5 * (first.min() + second.max())
    res = _process(data, rij, W, 1.0, dict(window='hann', mdccm_min=gate))
    g = planner.beam_trace_window(W)
    cover = _against_both(res, data, g, gate=gate, label='gated')
    assert np.any(cover == 0) and np.all(res.beam_trace[0][(n // 2 + 2) * inc:] == 0.0)
    used = md >= gate
    assert used[:n // 2 - 1].all() and not used[n // 2 + 1:].any()
    assert _bits(res.beam_trace[0][:(n // 2 - 2) * inc], plain.beam_trace[0][:(n // 2 - 2) * inc])
    nan = _process(data, rij, W, 1.0, dict(window='hann', mdccm_min=float('nan')))
    assert _bits(nan.beam_trace, plain.beam_trace)
    everyone = _process(data, rij, W, 1.0, dict(window='hann', mdccm_min=-1.0))
    assert _bits(everyone.beam_trace, plain.beam_trace)


# ---- the elements LTS kept ----

def _designed(N):
    """Windows of unit pulses on a plane-wave pattern with one or two elements' pulses displaced (tests/test_gpu_kept.py)."""
    q = st.grid_units(N)
    s = st.SLOWNESS[0]
    p = st.CENTRE - (q[:, 0] * s[0] + q[:, 1] * s[1])
    rows = [('exact', p.copy(), ())]
    for e in (0, N // 2, N - 1):
        pk = p.copy()
        pk[e] += 7
        rows.append(('element %d' % e, pk, (e,)))
    pk = p.copy()
    pk[N - 1] += 7
    pk[0] -= 5
    rows.append(('elements 0 and %d' % (N - 1), pk, (0, N - 1)))
    want = [tuple(e for e in bad if st.within_breakdown(N, len(bad))) for _, _, bad in rows]
    return [(name, [[(int(v), 1.0)] for v in pk]) for name, pk, _ in rows], want, int(p[0])


@pytest.mark.parametrize('N', [8, 9])
def test_kept_elements_on_designed_weights(N):
    """Element 0, a middle one and the last dropped at N = 8, two at once at N = 8 and 9: each window summed over the elements
    its mask leaves, at the delays against element 0 — a dropped element 0 does not move the window.  Where nothing is
    dropped the bits are the flag-off plan's."""
    tabs, want, p0 = _designed(N)                                    # p0: where element 0's pulse is on the plane wave
    rij = st.grid_geometry(N)
    x = st.pulse_trace(tabs)
    n = len(tabs)
    kw = dict(prefiltered=True, vector_len=n + 3, want_z=True, kept=(N - 1, False, False))
    call = lambda flag: engine.process(x, st.FS, T0, rij, [(None, None)], [st.W / st.FS], 0.0, 0.5,
                                       want_beam_trace=dict(window='boxcar', kept=flag), **kw)
    on, off = call(True), call(False)
    assert int(on.nwin[0]) == n and _bits(on.dropped_mask, off.dropped_mask)
    intended = [sum(1 << e for e in w) for w in want]
    assert on.dropped_mask[0, :n].tolist() == intended and any(m & 1 for m in intended) and sum(bool(m) for m in intended) >= 4
    g = np.ones(st.W)
    for res, kept in ((on, True), (off, False)):
        args = list(_truth_args(res, x))
        if not kept:
            args[4] = None
        assert _bits(res.beam_trace[0], bt.restate(*args, g)), kept
    W = st.W
    for w in range(n):
        a, b = on.beam_trace[0][w * W:(w + 1) * W], off.beam_trace[0][w * W:(w + 1) * W]
        if intended[w] == 0:
            assert _bits(a, b), tabs[w][0]                            # nothing dropped: the flag-off plan's bits
        else:
            # the kept elements' pulses line up on element 0's time base: one pulse of height 1 where element 0's pulse
            # would be on the plane wave, whether or not element 0 itself is kept
            assert a[p0] == 1.0 and np.count_nonzero(a) == 1, (tabs[w][0], np.flatnonzero(a))
            assert b[p0] < 1.0 and np.count_nonzero(b) >= 2, tabs[w][0]


def test_kept_flag_on_a_noisy_wave_against_both_truths():
    N, W = 8, 257
    data, rij = _wave(N, W * 6 + 1, mistimed=True, snr_db=10.0)
    kw = dict(kept=(N - 1, False, False))
    on = _process(data, rij, W, 0.5, dict(window='hann', kept=True), **kw)
    n = int(on.nwin[0])
    assert np.count_nonzero(on.dropped_mask[0, :n] == 1 << (N - 1)) >= n // 2
    _against_both(on, data, planner.beam_trace_window(W), kept=True, label='kept')
    off = _process(data, rij, W, 0.5, dict(window='hann', kept=False), **kw)
    assert not _bits(on.beam_trace, off.beam_trace) and all(_bits(getattr(on, k), getattr(off, k)) for k in PLAIN)


# ---- the forms of a pass ----

EDGES = [(0.5, 1.5), (1.5, 4.0)]
WINLENS = [257.5 / FS, 65.5 / FS]
FILTER = ('butter', 2, 0.01)
NF = 6
FORM_KW = dict(want_beam=True, kept=(NF - 1, True, False), want_beam_trace=dict(window='hann', mdccm_min=0.3, kept=True))


def _recordings(npts=2401, S=3):
    rij = synthetic.array_geometry(NF, 1.0)
    data = [np.ascontiguousarray(synthetic.plane_wave(rij, npts, FS, 0.5, 4.0, baz_deg=20.0 + 67.0 * i, snr_db=10.0, timing_error_s=0.25,
                                                      bad_element=(NF - 1, 0, 2)[i], seed=520 + i)) for i in range(S)]
    return data, rij - rij.mean(axis=1, keepdims=True), [T0 + 0.0173 * i for i in range(S)]


def _two_bands(data, rij, t0=T0, **kw):
    return engine.process(data, FS, t0, rij, EDGES, WINLENS, 0.5, 0.5, *FILTER, **dict(FORM_KW, **kw))


def test_batch_of_three_recordings_equals_three_single_calls():
    recs, rij, t0s = _recordings()
    batch = engine.process_batch([list(d) for d in recs], FS, t0s, rij, EDGES, WINLENS, 0.5, 0.5, *FILTER, **FORM_KW)
    assert len(batch) == 3
    for s in range(3):
        single = _two_bands(recs[s], rij, t0s[s])
        assert single.beam_trace.shape == (2, 2401) and single.beam_trace.any(axis=1).all()
        assert _bits(batch[s].beam_trace, single.beam_trace), s
        for k in PLAIN + ('dropped_mask', 'beam_power'):
            assert _bits(getattr(batch[s], k), getattr(single, k)), (s, k)
    assert not _bits(batch[0].beam_trace, batch[1].beam_trace)


def test_streamed_and_overlapped_passes_equal_the_unstreamed_pass(monkeypatch):
    recs, rij, _ = _recordings(48001, 1)
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    whole = _two_bands(recs[0], rij)
    assert whole.beam_trace.any(axis=1).all()
    h = engine.get_handle()
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '1')
    try:
        h.set_option('screen_batch_mb', 1)
        h.set_option('solve_min_units', 1)
        streamed = _two_bands(recs[0], rij)
        nbatches = h.result_batches()
        h.set_option('overlap', 1)                                # the per-batch solves on the second stream: the trace joins through an event
        overlapped = _two_bands(recs[0], rij)
        h.set_option('overlap', -1)
        serial = _two_bands(recs[0], rij)
    finally:
        h.set_option('overlap', 0)
        h.set_option('screen_batch_mb', 192)
        h.set_option('solve_min_units', 0)
    assert nbatches >= 3, nbatches
    for name, got in (('streamed', streamed), ('overlap on', overlapped), ('overlap off', serial)):
        assert _bits(got.beam_trace, whole.beam_trace), name
        for k in PLAIN:
            assert _bits(getattr(got, k), getattr(whole, k)), (name, k)


def test_two_hbm_rounds_equal_one(monkeypatch):
    recs, rij, _ = _recordings(2401, 1)
    whole = _two_bands(recs[0], rij)
    # room for one band with its trace row, not for two: NF filtered rows and one trace row per band
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', repr(1.5 * 8.0 * (NF + 1) * (2401 + 64) / 2.0 ** 30))
    assert engine.max_bands_per_pass(NF, 2401, 1) == 1
    rounds = _two_bands(recs[0], rij)
    assert _bits(rounds.beam_trace, whole.beam_trace)
    for k in PLAIN:
        assert _bits(getattr(rounds, k), getattr(whole, k)), k


@pytest.mark.parametrize('plan', ['seeded', 'refined'])
def test_seeded_and_refined_plans(plan):
    """The trace follows whatever slowness the plan solves; the delays are the whole-sample ones of z in every case."""
    N, W = 8, 257
    data, rij = _wave(N, W * 4 + 1, mistimed=True, snr_db=10.0)
    kw = dict(slowness_grid=planner.slowness_grid(3.5, 11), seed_halfwidths=6) if plan == 'seeded' else dict(want_subsample=True)
    res = _process(data, rij, W, 0.5, 'hann', **kw)
    assert _bits(res.beam_trace[0], _restated(res, data, planner.beam_trace_window(W))), plan
    full = _process(data, rij, W, 0.5, 'hann')
    assert not _bits(res.z, full.z) or plan == 'seeded'


# ---- off ----

def test_a_plan_without_the_feature():
    N, W = 5, 65
    data, rij = _wave(N, 1201)
    off = _process(data, rij, W, 1.0, None, want_beam=True)
    assert off.beam_trace is None
    with pytest.raises(_hip.NblsError) as err:
        off.handle.fetch_beam_trace(0)
    assert err.value.code == _hip.NBLS_ERR_STATE
    on = _process(data, rij, W, 1.0, True, want_beam=True)
    for k in PLAIN + ('z', 'beam_power', 'fstat'):
        assert _bits(getattr(on, k), getattr(off, k)), k
    assert on.beam_trace.any()


# ---- refusals ----

def test_refusals_of_the_library():
    N = 5
    data, rij = _wave(N, 1201)
    res = engine.process(data, FS, T0, rij, [(None, None)], [65.5 / FS], 0.5, 1.0, prefiltered=True)
    h = res.handle
    plan = lambda W=(65,): h.plan(None, False, None, None, list(W), [32] * len(W), 40)
    g = planner.beam_trace_window(65)
    dp = g.ctypes.data_as(_hip.C.POINTER(_hip.C.c_double))
    for bad in ((dp, -1, 0.5, 0), (dp, 65, 0.5, 2), (dp, 65, 0.5, -1)):        # a negative count, unknown flags: the handle is unchanged
        assert h.lib.nbls_set_beam_trace(h._h, *bad) == _hip.NBLS_ERR_ARG, bad[1:]
    plan()
    with pytest.raises(_hip.NblsError) as err:
        h.fetch_beam_trace(0)
    assert err.value.code == _hip.NBLS_ERR_STATE
    try:
        for table in (g[:64], np.r_[g, 1.0], np.zeros(65), np.r_[g[:64], -1.0], np.r_[g[:64], np.nan], np.r_[g[:64], np.inf]):
            h.set_beam_trace(table)
            with pytest.raises(ValueError, match='nbls_set_beam_trace') as err:
                plan()
            assert err.value.code == _hip.NBLS_ERR_ARG
        h.set_beam_trace(np.r_[g, np.zeros(65)])                     # the second band's table all zero
        with pytest.raises(ValueError, match='band 1') as err:
            plan((65, 65))
        assert err.value.code == _hip.NBLS_ERR_ARG
        h.set_beam_trace(g, kept=True)                               # the flag without the kept feature
        with pytest.raises(_hip.NblsError, match='nbls_set_kept_elements') as err:
            plan()
        assert err.value.code == _hip.NBLS_ERR_STATE
        h.set_beam_trace(g)
        h.set_window_ranges(np.array([1]), np.array([5]))
        with pytest.raises(ValueError, match='nbls_set_window_ranges') as err:
            plan()
        assert err.value.code == _hip.NBLS_ERR_UNSUPPORTED
        h.set_window_ranges(None)
        sub = [0, 1, 2, 3]
        xs, ps, xp = planner.co_array(rij[:, sub])
        h.set_estimators([dict(kept=sub, xij=xs, pair_idx=ps, xpinv=xp, lts=None, eig6=None)])
        with pytest.raises(ValueError, match='nbls_set_estimators') as err:
            plan()
        assert err.value.code == _hip.NBLS_ERR_UNSUPPORTED
        h.set_estimators(())
        plan()                                                       # accepted
        n = int(res.nwin[0])
        assert not h.fetch_beam_trace(0).any()                       # zeros until a pass has run the solve stage
        h.execute(stages=3)
        assert not h.fetch_beam_trace(0).any()
        h.execute()
        first = h.fetch_beam_trace(0)
        assert first.shape == (1201,) and first[:32 * n].all()
        h.execute(stages=3)                                          # a pass without the solve stage leaves it as it is
        assert _bits(h.fetch_beam_trace(0), first)
        for row in (-1, 1):
            with pytest.raises(ValueError) as err:
                h.fetch_beam_trace(row)
            assert err.value.code == _hip.NBLS_ERR_ARG
    finally:
        h.set_window_ranges(None)
        h.set_estimators(())
        h.set_beam_trace(None)
    plan()
    with pytest.raises(_hip.NblsError):                              # switched off again
        h.fetch_beam_trace(0)


def test_rccl_communicator_refuses_the_request_at_plan_time():
    """A communicator lives as long as its process: a child process over the tests' loopback transport."""
    src = os.path.join(ROOT, 'tests', 'c_caller', 'loopback_rccl.cpp')
    lib = os.path.join(ROOT, 'tests', 'c_caller', 'libloopback_rccl.so')
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.run(['/opt/rocm/bin/hipcc', '-O2', '-shared', '-fPIC', '--offload-arch=gfx950', src, '-o', lib], check=True,
                       timeout=300)
    env = dict(os.environ, NBLS_TEST_TRANSPORT=lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_beam_trace_comm_worker.py')], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and 'BEAM_TRACE_COMM_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the public calls ----

def test_public_calls_on_the_demonstration_trace():
    d = cases.DEMO
    noisy, clean, rij = cases.demo_traces()
    st8 = synthetic.make_stream(noisy, FS)
    got = ltsva_beam_trace(st8, None, None, d['W'] / FS, 0.5, alpha=0.5, rij=rij)
    plain = ltsva(st8, None, None, d['W'] / FS, 0.5, alpha=0.5, rij=rij)
    assert len(got) == 9 and len(plain) == 8
    for i in (0, 1, 2, 3, 5, 6, 7):
        np.testing.assert_array_equal(got[i], plain[i])
    trace = got[8]
    assert trace.shape == (d['npts'],) and trace.dtype == np.float64
    ratio = cases.residual_ratio(trace, noisy[0], clean[0])
    print('ltsva_beam_trace on the demonstration trace: residual ratio %.3f (1 / N = %.3f)' % (ratio, 1.0 / d['N']))
    assert ratio <= 2.0 / d['N']
    gated = ltsva_beam_trace(st8, None, None, d['W'] / FS, 0.5, alpha=0.5, rij=rij, mdccm_min=d['mdccm_min'])
    assert _bits(gated[8], trace)                                     # every window of the wave passes the demonstration's gate
    quiet = ltsva_beam_trace(synthetic.make_stream(cases.demo_noise(), FS), None, None, d['W'] / FS, 0.5, alpha=0.5, rij=rij,
                             mdccm_min=d['mdccm_min'])
    assert not quiet[8].any()                                         # ... and no window of noise alone
    kept = ltsva_beam_trace(st8, None, None, d['W'] / FS, 0.5, alpha=0.5, rij=rij, kept=True, window='boxcar', mdccm_min=0.0)
    assert kept[8].shape == (d['npts'],) and cases.residual_ratio(kept[8], noisy[0], clean[0]) <= 2.0 / d['N']
    quiet8 = synthetic.make_stream(cases.demo_noise(), FS)
    batch = ltsva_beam_trace_batch([st8, quiet8, st8], None, None, d['W'] / FS, 0.5, alpha=0.5, rij=rij, mdccm_min=d['mdccm_min'])
    assert len(batch) == 3 and all(len(b) == 9 for b in batch)
    assert _bits(batch[0][8], trace) and _bits(batch[2][8], trace) and not batch[1][8].any()
    for i in (0, 1, 2, 3, 5, 6, 7):
        np.testing.assert_array_equal(batch[0][i], got[i])
    one = ltsva_beam_trace_batch([st8], None, None, d['W'] / FS, 0.5, alpha=0.5, rij=rij)
    assert len(one) == 1 and _bits(one[0][8], trace)
    kb = ltsva_beam_trace_batch([st8, st8], None, None, d['W'] / FS, 0.5, alpha=0.5, rij=rij, kept=True, window='boxcar',
                                mdccm_min=0.0)
    assert all(len(b) == 9 and _bits(b[8], kept[8]) for b in kb)


def test_narrow_band_call_on_the_demonstration_trace():
    """The raw traces through the library's own filter: the band's trace against the noise-free wave through the same
    call's filter (the beam trace of the noise-free record, whose elements line up exactly, is its element 0)."""
    d = cases.DEMO
    rij = synthetic.array_geometry(d['N'], 1.0)
    raw = lambda snr: synthetic.make_stream(synthetic.plane_wave(rij, d['npts'], FS, 0.1, 5.0, baz_deg=d['baz'], vel_kms=d['vel'],
                                                                 snr_db=snr), FS)
    fr = np.logspace(-1, 0.5, 16)
    args = lambda s: ([d['W'] / FS, d['W'] / FS], 0.5, 0.5, s, None, None, 2, np.zeros(16), np.zeros(16),
                      np.array([0.8, 1.2, 1.8]), 'linear', fr, 'butter', 2, 0.01)
    out = narrow_band_least_squares_beam_trace(*args(raw(d['snr_db'])), rij=rij)
    ref = narrow_band_least_squares(*args(raw(d['snr_db'])), rij=rij)
    assert len(out) == 10 and len(ref) == 9
    for i in (0, 1, 2, 3, 5, 6):
        np.testing.assert_array_equal(out[i], ref[i])
    assert out[9].shape == (2, d['npts'])
    h = engine.get_handle()
    noisy0 = h.fetch_filtered(0)[0]
    narrow_band_least_squares(*args(raw(400.0)), rij=rij)
    clean0 = engine.get_handle().fetch_filtered(0)[0]
    ratio = cases.residual_ratio(out[9][0], noisy0, clean0)
    print('narrow_band_least_squares_beam_trace, band 0.8 - 1.2 Hz: residual ratio %.3f (1 / N = %.3f)' % (ratio, 1.0 / d['N']))
    assert ratio <= 2.0 / d['N']
