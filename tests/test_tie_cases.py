"""Without a GPU: the premises of tests/test_gpu_ties.py (tests/tie_cases.py).  For every case and every shape it is run
at: the traces are integers whose correlations FP64 holds exactly in any order, distinct correlation values keep distinct
quotients, the exact reference is the oracle's; in a NumPy model of the quantiser and of the screening values the designed
ties are exact ties, nothing else lies within 2 theta of a record's maximum (theta: the kernel's own formula — the factor
2 is the margin, so that no design rests on the model's last bit), no direction of any pair is empty, and the designed
lags fall in the lanes the case was built for.  The shapes reach the routes they were chosen for."""
import os
import re

import numpy as np
import pytest

import tie_cases as tc
from narrow_band_least_squares_amd import planner, _hip

ROUTE_FAMILY = [(r, f) for r, fams in tc.PLAN for f in fams]


def test_stated_constants_are_the_sources():
    for name, pattern, value in tc.STATED:
        with open(os.path.join(tc.CSRC, name)) as f:
            found = re.findall(pattern, f.read())
        assert found and all(str(v) == str(value) for v in found), '%s: %s gives %r, tests/tie_cases.py states %r' % (
            name, pattern, found, value)
    with open(os.path.join(tc.CSRC, 'xcorr_screen.hip')) as f:
        src = f.read()
    for line in tc.THETA_SOURCE:
        assert line in src, 'theta_model evaluates a formula the kernel no longer has: %s' % line


def test_shapes_reach_the_routes_they_were_chosen_for():
    for name, r in tc.ROUTES.items():
        g = tc.route_geometry(name)
        for k, v in r['expect'].items():
            assert g.route[k] == v, '%s: %s is %r, chosen for %r (%s)' % (name, k, g.route[k], v, g.route)
    assert {tc.ROUTES[n]['expect'].get('verifier') for n in ('dma', 'lds', 'glob')} == {1, 2, 3}
    assert {tc.ROUTES[n]['expect'].get('screen_inst') for n in ('dma', 'nc4', 'tb8')} == {1, 2, 3}
    # the global-memory verifier at the first window length of three elements (the fewest that screen) that leaves LDS
    g = tc.ROUTES['glob']
    assert g['N'] == 3 and g['N'] * g['W'] * 8 > 158 * 1024 and tc.geometry(3, g['W'] - 2).route['verifier'] == 2
    with pytest.raises(AssertionError):
        tc.geometry(2, 600)
    n = tc.route_geometry('npg')
    assert n.route['G'] < n.N - 1                       # partner groups
    assert tc.route_geometry('lds').step == 32          # the hand-scheduled two-block K loop
    for name in ('dma', 'nc4', 'tb8'):
        g0 = tc.route_geometry(name)
        ws = tc.end_windows(name)
        assert [W % g0.span for W in ws] == [0, 1, g0.step - 1, g0.step, g0.step + 1]
        for W in ws:
            g = tc.route_geometry(name, W)
            assert (g.S, g.TBV, g.route['screen_inst']) == (g0.S, g0.TBV, g0.route['screen_inst'])
            assert planner.window_plan(tc.npts_of(W), 1.0, float(W), 0.0)[1:3] == (W, 2)
    # the families the issue asks of every verifier and of every screening instance
    plan = dict(tc.PLAN)
    assert all({'list', 'lane', 'truth'} <= set(plan[r]) for r in ('dma', 'lds', 'glob'))
    assert all({'end', 'stale'} <= set(plan[r]) for r in ('dma', 'nc4', 'tb8'))
    assert set(tc.FAMILIES) <= set(plan['dma'])


def test_lane_helpers():
    for S, TBV in ((8, 4), (2, 4), (1, 8), (1, 4)):
        step, span = 16 * S, TBV * 16 * S
        lane = tc.one_lane(4 * TBV, 8 * span, S, TBV, p=2, block=3)
        assert len(set(lane)) == 4 * TBV and {tc.lane_of(d, S, TBV) for d in lane} == {(2, 3)}
        assert lane == sorted(lane) and lane[:5] == [2 * span + 12 + r for r in range(4)] + [2 * span + step + 12]
        # every lag of a group belongs to exactly one of its 4 S lanes, sixteen (TBV = 4) or thirty-two lags each
        loads = {}
        for d in range(span, 2 * span):
            loads.setdefault(tc.lane_of(d, S, TBV), []).append(d)
        assert len(loads) == 4 * S and all(len(v) == 4 * TBV for v in loads.values())
        for m in (1, 26, 27, 40):
            lags = tc.spread(m, 4 * span, S, TBV)
            assert len(set(lags)) == m and tc.lane_loads(lags, S, TBV, 4)[1] <= tc.NSLOT
    assert tc.lane_loads([4, 5, 6, 7, 132, 133, 134], 8, 4, 4) == (7, 7)
    assert tc.lane_loads([4, 5, 6, 7, 4 * 512 + 4, 4 * 512 + 5, 4 * 512 + 6], 8, 4, 4) == (4, 7)     # a later group: any wave


def _pairs(N):
    return [tuple(p) for p in planner.pair_table(N)]


@pytest.mark.parametrize('route,family', ROUTE_FAMILY)
def test_premises_of_every_case(oracle, route, family):
    cases = tc.cases_for(route, family)
    assert cases
    for g, case in cases:
        msg = '%s %r N=%d W=%d' % (route, case, g.N, g.W)
        N, W = g.N, g.W
        x = tc.traces(case, W, N)
        assert x.dtype == np.int64 and x.shape == (N, tc.npts_of(W)), msg
        pairs = _pairs(N)
        lag_r, cmax_r, kk_r = tc.reference(x, W, pairs)
        xf = x.astype(np.float64)
        assert np.array_equal(xf.astype(np.int64), x)
        # the reference is the oracle's (float64 samples, np.correlate, division before the arg-max)
        tau_o, _, cmax_o = oracle.correlate_windows(xf.T, W, np.arange(2) * W, pairs, 1.0)
        np.testing.assert_array_equal(lag_r, np.rint(tau_o.T).astype(np.int64), err_msg=msg)
        np.testing.assert_array_equal(cmax_r, cmax_o.T, err_msg=msg)
        for w in range(2):
            seg = x[:, w * W:(w + 1) * W]
            for i, j in pairs:
                a, b = seg[i], seg[j]
                # every partial sum of every lag in any order is bounded by sum |a| * max |b|
                assert float(np.sum(np.abs(a))) * float(np.max(np.abs(b))) < 2.0 ** 53 and np.sum(a * a) < 2 ** 53, msg
                _, _, c, quot = tc.pair_truth(a, b)
                ci = np.correlate(a, b, 'full')
                assert np.array_equal(c, ci), msg
                cf = np.correlate(a.astype(np.float64), b.astype(np.float64), 'full')
                assert np.array_equal(cf, ci.astype(np.float64)) and np.array_equal(cf.astype(np.int64), ci), msg
                # distinct raw values have distinct quotients: the division cannot make a tie the integers do not have
                u, first = np.unique(c, return_index=True)
                assert np.all(np.diff(quot[first]) > 0), msg
            # the quantiser as the issue writes it and as the kernel computes it
            for ch in range(N):
                mx = np.max(np.abs(seg[ch]))
                assert np.array_equal(tc.quantise(seg[ch])[0], np.rint(seg[ch] * 16256.0 / mx).astype(np.int64)), msg
            if case.seed is not None:
                continue
            recs = tc.model_records(seg, g)
            for (i, j), r in recs.items():
                assert r.v.max() > 0, '%s window %d: direction %d over %d is empty' % (msg, w, i, j)
                assert len(r.near) == 0, '%s window %d (%d over %d): lags %s within 2 theta = %g of the maximum %g' % (
                    msg, w, i, j, r.near[:8], 2 * r.theta, r.v.max())
                # the true index of the pair is among the ties of the direction(s) that hold it
                kk = int(kk_r[w, pairs.index((min(i, j), max(i, j)))])
                if (kk >= W - 1) if i < j else (kk <= W - 1):
                    assert kk in r.kk or r.v.max() < recs[j, i].v.max(), msg
            for (i, j), sign in (((0, 1), 1), ((1, 0), -1)):
                r = recs[i, j]
                want = sorted(sign * s for s in case.ties[w] if sign * s >= 0)
                top = max(recs[0, 1].v.max(), recs[1, 0].v.max())
                if want:
                    assert list(r.ties) == want and r.v.max() == top, '%s window %d (%d over %d): ties %s, designed %s' % (
                        msg, w, i, j, r.ties, want)
                else:
                    assert r.v.max() < top - 2 * r.theta, msg
                if case.kind == 'lane' and want:
                    assert len({tc.lane_of(d, g.S, g.TBV) for d in want}) == 1 and r.sure == len(want), msg
                if case.kind == 'spread':
                    assert r.may <= tc.NSLOT, msg
                d = tc.designed_record(r)
                assert d['count'] is not None or d.get('interval') or case.kind is None, msg


def test_every_family_designs_what_it_says():
    g = tc.route_geometry('dma')

    def designed(case, w=0, pair=(0, 1)):
        return tc.designed_record(tc.model_records(tc.traces(case, g.W, g.N)[:, w * g.W:(w + 1) * g.W], g)[pair])

    got = [designed(c) for c in tc.list_length(g.W, g.S, g.TBV)]
    assert [(d['count'], d['flags']) for d in got] == [(1, 0), (2, 0), (6, 0), (7, 0), (25, 0), (26, 0), (26, 2), (26, 2), (26, 2)]
    assert all(len(d['listed']) == d['count'] for d in got[:6]) and all(d['listed'] is None for d in got[6:])
    # the mirrored window: the same design in the record of the sliding index ABOVE its partner
    assert [designed(c, 1, (1, 0))['count'] for c in tc.list_length(g.W, g.S, g.TBV)[:6]] == [1, 2, 6, 7, 25, 26]
    got = [designed(c) for c in tc.lane_slots(g.W, g.S, g.TBV)]
    assert [(d['count'], d['flags']) for d in got] == [(6, 0), (6, 1), (6, 1), (6, 1)]
    up, down, later = tc.stale_slots(g.W, g.S, g.TBV)
    assert designed(up)['flags'] == designed(down)['flags'] == 1
    assert {tc.lane_of(d, g.S, g.TBV)[0] for d in later.ties[0]} == {1} and designed(later)['count'] == 7
    gg = tc.route_geometry('glob')
    for c in tc.stale_across_groups(gg.W, gg.S, gg.TBV, gg.nw):
        d = tc.designed_record(tc.model_records(tc.traces(c, gg.W, gg.N)[:, :gg.W], gg)[0, 1])
        assert (d['count'], d['flags']) == (6, 0) and len(set(c.tables[0].values())) > gg.nw
    # the true maximum: where the special pulse sits decides the reference
    pairs = _pairs(g.N)
    by = {c.name: c for c in tc.true_maximum(g.W, g.S, g.TBV)}
    for name, pick in (('plus_first', min), ('plus_last', max), ('minus_first', lambda t: sorted(t)[1]), ('minus_last', min)):
        c = by[name]
        kk = tc.reference(tc.traces(c, g.W, g.N), g.W, pairs)[2]
        assert kk[0, 0] == g.W - 1 + pick(c.ties[0]), name
    c = by['plus_absorbed']
    assert tc.reference(tc.traces(c, g.W, g.N), g.W, pairs)[2][0, 0] == g.W - 1 + c.ties[0][7]
    c = by['minus_all_but_the_absorbed']
    assert tc.reference(tc.traces(c, g.W, g.N), g.W, pairs)[2][0, 0] == g.W - 1 + c.ties[0][6]
    for c in tc.window_ends(g.W, g.S, g.TBV):
        assert max(c.ties[0]) == g.W - 1 and min(c.ties[1]) == -(g.W - 1)
    # covers(): the soundness test of a record
    rec = np.zeros(32, dtype=np.int32)
    rec[:8] = (2, 0, 0x7fffffff, -1, 0, 0, 700, 650)
    assert tc.covers(rec, 650) and not tc.covers(rec, 651) and not tc.covers(rec, 0)
    rec[1:4] = (1, 640, 660)
    assert tc.covers(rec, 651) and not tc.covers(rec, 661)
    rec[1] = 2
    assert tc.covers(rec, 3)
