"""The candidate records of the int8 screening correlator (csrc/xcorr_screen.hip) where they overflow, and what the FP64
verifier makes of them, on integer traces whose every correlation value FP64 holds exactly (tests/tie_cases.py; their
premises are asserted without a GPU in tests/test_tie_cases.py).

Every case is a pre-filtered pass of two windows.  FIRST the records (``Handle.screen_records``): for every ordered pair
the true np.correlate index is listed, or inside a flagged interval, or the record carries flag 2; for the designed
cases the count, the flags and the list are the designed ones (``tie_cases.designed_record``).  A failure there is a
``SCREEN finding``.  THEN the result: the lag is the exact reference's, cmax agrees to rtol 1e-12, and both are what the
VALU correlator (xcorr_impl=1) returns on the same bytes — a ``VERIFY finding``.  The findings of a test are collected and
reported together, each with N, W, the route and the case.

list, lane and truth run on every verifier (persistent DMA, LDS, global memory); end and stale on every screening
instance; both, drop and noise on the default route; both again and regroup on the global-memory verifier, the only one
with the run form and, at its window length, more lag groups than waves."""
import numpy as np
import pytest

import tie_cases as tc
from narrow_band_least_squares_amd import engine, planner, synthetic

pytestmark = pytest.mark.gpu

RTOL = 1e-12             # cmax against the reference: the tolerance of tests/test_gpu_routes.py


def _geometry(N):
    rij = synthetic.array_geometry(N, 1.0, seed=N)
    return rij - rij.mean(axis=1, keepdims=True)


def _run(x, W, N, impl):
    return engine.process(x, 1.0, 0.0, _geometry(N), [(None, None)], [float(W)], 0.0, 1.0, prefiltered=True, want_lag=True,
                          want_cmax=True, xcorr_impl=impl)


def _dump(rec):
    n = int(rec[0])
    return 'count %d flags %d interval [%d, %d] max %g theta %g list %s' % (
        n, rec[1], rec[2], rec[3], rec[4:5].view(np.float32)[0], rec[5:6].view(np.float32)[0], sorted(int(k) for k in rec[tc.CHDR:tc.CHDR + n]))


def _check_records(recs, x, g, case, kk_r, pairs, where):
    """-> the SCREEN findings of the records (units, N, N, 32) of the two windows of ``x``."""
    found = []
    N, W = g.N, g.W
    for w in range(2):
        model = tc.model_records(x[:, w * W:(w + 1) * W], g) if case.seed is None else None
        for p, (i, j) in enumerate(pairs):
            kk = int(kk_r[w, p])
            for a, b in ((i, j), (j, i)):
                rec = recs[w, a, b]
                tag = 'SCREEN finding: %s window %d record (%d over %d)' % (where, w, a, b)
                if ((kk >= W - 1) if a < b else (kk <= W - 1)) and not tc.covers(rec, kk):
                    found.append('%s: the true index %d is neither listed, nor in a flagged interval, nor under flag 2: %s' % (
                        tag, kk, _dump(rec)))
                if model is None:
                    continue
                m = model[a, b]
                d = tc.designed_record(m)
                if d['count'] is not None and (int(rec[0]), int(rec[1])) != (d['count'], d['flags']):
                    found.append('%s: designed count %d flags %d (ties at %s): %s' % (tag, d['count'], d['flags'], sorted(m.kk), _dump(rec)))
                if d['listed'] is not None and set(int(k) for k in rec[tc.CHDR:tc.CHDR + int(rec[0])]) != d['listed']:
                    found.append('%s: designed list %s: %s' % (tag, sorted(d['listed']), _dump(rec)))
                if d.get('interval') and not rec[1] & 1:
                    found.append('%s: more than %d ties in one lane and no interval: %s' % (tag, tc.NSLOT, _dump(rec)))
                if not rec[1] & 2 and not all(tc.covers(rec, k) for k in m.kk):
                    found.append('%s: ties %s not covered: %s' % (tag, sorted(k for k in m.kk if not tc.covers(rec, k)), _dump(rec)))
                if rec[4:5].view(np.float32)[0] != m.v.max():
                    found.append('%s: screening maximum %g, the model\'s %g' % (tag, rec[4:5].view(np.float32)[0], m.v.max()))
    return found


def _check_result(lag, cmax, ref, valu, where):
    found = []
    lag_r, cmax_r, _ = ref
    for name, got, want in (('lag', lag, lag_r), ('lag of xcorr_impl=1', valu[0], lag_r), ('lag against xcorr_impl=1', lag, valu[0])):
        if not np.array_equal(got, want):
            bad = np.argwhere(np.asarray(got) != np.asarray(want))
            found.append('VERIFY finding: %s: %s differs at (window, pair) %s: %s, expected %s' % (
                where, name, bad[:6].tolist(), [int(got[tuple(b)]) for b in bad[:6]], [int(want[tuple(b)]) for b in bad[:6]]))
    for name, got, want in (('cmax', cmax, cmax_r), ('cmax of xcorr_impl=1', valu[1], cmax_r)):
        if not np.allclose(got, want, rtol=RTOL, atol=0.0):
            found.append('VERIFY finding: %s: %s off by %g relative' % (where, name, np.max(np.abs(got / want - 1.0))))
    if not np.array_equal(cmax, valu[1]):
        found.append('VERIFY finding: %s: cmax differs from xcorr_impl=1 by %g relative' % (where, np.max(np.abs(cmax / valu[1] - 1.0))))
    return found


def _run_cases(route, families):
    h = engine.get_handle()
    opts = tc.ROUTES[route]['opts']
    found = []
    try:
        for o in opts:
            h.set_option(o, 1)
        for family in families:
            for g, case in tc.cases_for(route, family):
                where = 'N=%d W=%d route=%s %s case=%r' % (g.N, g.W, route, {k: g.route[k] for k in (
                    'G', 'S', 'nsl', 'ncopy', 'screen_inst', 'verifier')}, case)
                x = tc.traces(case, g.W, g.N)
                pairs = [tuple(p) for p in planner.pair_table(g.N)]
                ref = tc.reference(x, g.W, pairs)
                xf = x.astype(np.float64)
                h.set_profiling(True)
                try:
                    res = _run(xf, g.W, g.N, 0)
                    assert h.timings()['xcorr_impl'] == 3, where
                finally:
                    h.set_profiling(False)
                recs = h.screen_records()
                assert recs.shape == (2, g.N, g.N, 32), where
                found += _check_records(recs, x, g, case, ref[2], pairs, where)
                valu = _run(xf, g.W, g.N, 1)
                found += _check_result(res.lag[0, :2], res.cmax[0, :2], ref, (valu.lag[0, :2], valu.cmax[0, :2]), where)
    finally:
        for o in opts:
            h.set_option(o, 0)
    assert not found, '%d findings\n' % len(found) + '\n'.join(found[:40])


@pytest.mark.parametrize('route', ('dma', 'lds', 'glob'))
@pytest.mark.parametrize('family', ('list', 'lane', 'truth'))
def test_list_length_lane_slots_and_true_maximum_on_every_verifier(route, family):
    """m = 1..64 exact ties spread over the lanes (the list up to 26, flag 2 from 27), 6..16 ties in one lane (six slots,
    then the interval), and one pulse of 2^20 +- 1 among 2^20 wherever the records can put it."""
    _run_cases(route, (family,))


@pytest.mark.parametrize('route', ('dma', 'nc4', 'tb8'))
@pytest.mark.parametrize('family', ('end', 'stale'))
def test_window_end_and_stale_slots_on_every_screen_instance(route, family):
    """Candidates at d = +-(W - 1), +-(W - 2) with W mod (TBV step) in {0, 1, step - 1, step, step + 1}; stairs below seven
    ties in one lane, rising and falling, and stairs in one lag group with the ties in the next."""
    _run_cases(route, (family,))


@pytest.mark.parametrize('family', ('both', 'drop', 'noise'))
def test_both_directions_direction_drop_and_noise_on_the_default_route(family):
    """Ties in both records of a pair (d = 0 is in both), runs of consecutive lags, the direction the verifier drops or
    keeps, and the designs over integer noise (soundness of the records and the result only)."""
    _run_cases('dma', (family,))


@pytest.mark.parametrize('family', ('both', 'regroup'))
def test_run_form_and_slot_reuse_on_the_global_memory_verifier(family):
    """The run form (sorted list, runs of up to four lags, a lag listed by both directions) on runs of 2..9 lags, two runs
    one lag apart and runs across d = 0; and six pulses per lag group at rising / falling levels in thirteen groups on
    eight waves: a wave's second group finds its lane's six slots taken by the first."""
    _run_cases('glob', (family,))


@pytest.mark.parametrize('route', ('nsl1', 'static', 'npg'))
def test_one_sliding_channel_static_dealing_pretest_and_partner_groups(route):
    _run_cases(route, dict(tc.PLAN)[route])


def test_batch_of_three_recordings_through_the_dma_verifier():
    """Three recordings in one pass (``set_segments(3)``): six units' records, recording s at units 2 s, 2 s + 1."""
    route = 'seg'
    g = tc.route_geometry(route)
    cases = [c for _, c in tc.cases_for(route, 'lane')]
    S = tc.ROUTES[route]['nseg']
    assert len(cases) == S and g.route['verifier'] == 1
    xs = [tc.traces(c, g.W, g.N) for c in cases]
    pairs = [tuple(p) for p in planner.pair_table(g.N)]
    npts = tc.npts_of(g.W)
    prep = engine.prepare(g.N, npts, 1.0, _geometry(g.N), [(None, None)], [float(g.W)], 0.0, 1.0, prefiltered=True)
    h = engine.get_handle()
    got = {}
    try:
        h.set_segments(S)
        h.set_trace_rows([row for x in xs for row in np.ascontiguousarray(x.astype(np.float64))], 1.0)
        h.set_geometry(prep.xij, prep.pair_idx, prep.xpinv)
        for impl in (0, 1):
            h.set_profiling(impl == 0)
            h.plan(None, prep.zero_phase, prep.tl, prep.tr, prep.W, prep.inc, prep.vector_len, lts=None, xcorr_impl=impl)
            h.execute()
            got[impl] = h.fetch(want_lag=True, want_cmax=True)
            if impl == 0:
                assert h.timings()['xcorr_impl'] == 3
                recs = h.screen_records()
    finally:
        h.set_profiling(False)
        h.set_segments(1)
    assert recs.shape == (2 * S, g.N, g.N, 32)
    found = []
    for s, (case, x) in enumerate(zip(cases, xs)):
        where = 'N=%d W=%d route=%s recording %d case=%r' % (g.N, g.W, route, s, case)
        ref = tc.reference(x, g.W, pairs)
        found += _check_records(recs[2 * s:2 * s + 2], x, g, case, ref[2], pairs, where)
        found += _check_result(got[0]['lag'][s, :2], got[0]['cmax'][s, :2], ref, (got[1]['lag'][s, :2], got[1]['cmax'][s, :2]), where)
    assert not found, '%d findings\n' % len(found) + '\n'.join(found[:40])
