"""Host-side premises of tests/test_gpu_unit_counts.py (tests/unit_count_cases.py), without a GPU: the share-out constants
as the sources state them, the listed unit counts against a brute-force restatement of every kernel's index arithmetic,
the properties of the periodic traces, and the routes the correlation shapes are named for."""
import itertools

import numpy as np
import pytest

import unit_count_cases as uc
from narrow_band_least_squares_amd import _hip, planner

CUS = (256, 304, 120, 64)           # MI355X, and other counts: the lists hold for whatever the device reports


def test_the_sources_state_the_share_outs_this_file_assumes():
    got = uc.scrape()
    for name, fn, rx, expected in uc.SOURCE:
        assert got[name] == expected, '%s (%s): the source says %s, the cases assume %s' % (name, fn, got[name], expected)
    assert got['xcd_item'] == (uc.XCDS - 1, 3) and 1 << got['xcd_item'][1] == uc.XCDS
    assert got['screen_unit'][0] == got['screen_grid'][1] == uc.SCREEN_GROUP
    assert got['dma_grid'][0] == got['dma_per_xcd'][1] == uc.XCDS
    assert got['dma_prefetch'] == (2, 3) and got['dma_buffers'] == (1,)          # units k+1 .. k+3 in flight, two LDS buffers
    assert got['quant_reg_waves'] == (uc.QUANT_WAVES_MAX,) and 1 << got['quant_lds_waves'][0] == 64
    assert got['gather_waves'] == (uc.GATHER_WAVES,) and got['gather_cap'] == (uc.GATHER_CAP,)
    assert got['beam_wave_w'] == (uc.BEAM_WAVE_W,)
    assert got['kept_waves'] == (4,) and got['closure_waves'] == (4,) and got['beam_waves'] == (4,)
    for N in range(1, 33):
        a, b, c, d, e = got['kept_lanes']
        assert uc.kept_lanes(N) == (b if N <= a else (d if N <= c else e))


def test_the_issue_s_counts_at_256_compute_units():
    c = uc.per_xcd(256)
    assert c == 32
    assert uc.unit_counts('verify_dma', 256) == sorted({1, 2, 7, 8, 9, 17, 8 * c - 1, 8 * c, 8 * c + 1, 8 * c + 9, 16 * c - 1,
                                                         16 * c + 1, 24 * c + 1, 32 * c - 7})
    assert uc.unit_counts('gather_pairs', 256) == [1, 3, 4, 5, 32 * 256 - 1, 32 * 256, 32 * 256 + 1, 64 * 256 + 1]
    assert uc.unit_counts('kept_elements', N=5) == [7, 8, 9, 31, 32, 33]
    assert uc.unit_counts('kept_elements', N=9) == [3, 4, 5, 15, 16, 17]
    assert uc.unit_counts('kept_elements', N=17) == [1, 2, 3, 7, 8, 9]
    assert uc.unit_counts('solve_lts_wave') == [1, 2, 3, 4, 5, 9]
    assert set(uc.unit_counts('solve_ols')) >= {63, 64, 65, 129}
    assert uc.unit_counts('pack_weights', mask_bytes=1) == [255, 256, 257]
    assert uc.unit_counts('pack_weights', mask_bytes=5) == [51, 52]
    assert uc.unit_counts('closure') == uc.unit_counts('beam_fstat') == [1, 3, 4, 5, 9]
    assert uc.unit_counts('verify_glob') == uc.unit_counts('range_pick') == [1, 2, 3, 5]
    assert uc.unit_counts('xcd_item') == [1, 7, 8, 9, 15, 17]
    assert uc.unit_counts('screen') == [1, 7, 8, 9, 17]


@pytest.mark.parametrize('cus', CUS)
def test_dma_counts_reach_every_walk_of_up_to_four_units(cus):
    """Brute force over every count up to 4 units per workgroup: the patterns a launch can show — a workgroup walking
    0..4 units, an XCD whose workgroups walk k and k - 1 (k = 1..4), a last range short or empty — are all reached by the
    listed counts, and the counts stay within four units per workgroup."""
    c = uc.per_xcd(cus)
    possible = set()
    for nu in range(1, 32 * c + 1):
        possible |= uc.dma_patterns(nu, cus)
    assert possible == {('walk', k) for k in range(5)} | {('ragged', k) for k in range(1, 5)} | {'short', 'empty'}
    counts = uc.unit_counts('verify_dma', cus)
    reached = set()
    for nu in counts:
        assert max(max(row) for row in uc.dma_occupancy(nu, cus)) <= 4
        reached |= uc.dma_patterns(nu, cus)
    assert reached == possible, sorted(map(str, possible - reached))
    # the three-deep prefetch and the two buffers: walks of 1, 2, 3 and 4 units end with 3, 2, 1 and 0 dead prefetches
    assert {max(max(row) for row in uc.dma_occupancy(nu, cus)) for nu in counts} == {1, 2, 3, 4}
    # an XCD range that is one short, and one that is empty
    shares = {nu: (nu + 7) >> 3 for nu in counts}
    assert any(sum(uc.dma_occupancy(nu, cus)[7]) == shares[nu] - 1 for nu in counts)
    assert any(sum(uc.dma_occupancy(nu, cus)[7]) == 0 for nu in counts)


@pytest.mark.parametrize('N,waves', [(1, 1), (3, 1), (3, 2), (3, 3), (3, 4), (9, 4)])
def test_xcd_item_counts_reach_every_workgroup_and_range(N, waves):
    """The streaming kernels (quantisers: ``waves`` per workgroup, N items per unit; verify_lds_kernel: one item per unit):
    every number of live waves a workgroup can have, ranges that are full, short and empty, a share that is no multiple
    of the workgroup."""
    def patterns(nu):
        live, ranges = uc.xcd_occupancy(nu * N, waves)
        share = (nu * N + 7) >> 3
        p = {('live', k) for k in live}
        p |= {'empty' if r == 0 else ('short' if r < share else 'full') for r in ranges}
        if share % waves:
            p.add('ragged share')
        return p
    possible = set()
    for nu in range(1, 200):
        possible |= patterns(nu)
    counts = uc.unit_counts('xcd_item', N=N, waves=waves)
    reached = set()
    for nu in counts:
        reached |= patterns(nu)
    assert reached == possible, sorted(map(str, possible - reached))
    assert {('live', k) for k in range(waves + 1)} <= reached


def test_grouped_counts_reach_full_ragged_and_single_workgroups():
    """Kernels that take consecutive units s at a time: a lone unit, a workgroup short by one, exactly full, one unit in a
    second workgroup, and a third workgroup."""
    for kernel, s, kw in (('screen', 8, {}), ('solve_lts_wave', 4, {}), ('solve_ols', 64, {}), ('uncertainty', 64, {}),
                          ('closure', 4, {}), ('beam_fstat', 4, {})):
        counts = uc.unit_counts(kernel, **kw)
        occ = [tuple(uc.group_occupancy(nu, s)) for nu in counts]
        assert (1,) in occ and (s - 1,) in occ and (s,) in occ and (s, 1) in occ and (s, s, 1) in occ, (kernel, occ)
    # (unit, pair) items of four: 3 pairs per unit
    occ = [tuple(uc.group_occupancy(nu * 3, 4)) for nu in uc.unit_counts('verify_glob')]
    assert {o[-1] for o in occ} == {1, 2, 3} and max(len(o) for o in occ) >= 3
    # 136 pairs per unit (17 elements): whole workgroups, the unit seams inside
    assert all(nu * 136 % 4 == 0 for nu in uc.unit_counts('range_pick'))
    # (unit, mask byte) items of 256
    for MB in (1, 5):
        tails = {uc.group_occupancy(nu * MB, 256)[-1] for nu in uc.unit_counts('pack_weights', mask_bytes=MB)}
        assert 255 in tails and any(t < 8 for t in tails), (MB, tails)
        assert {len(uc.group_occupancy(nu * MB, 256)) for nu in uc.unit_counts('pack_weights', mask_bytes=MB)} == {1, 2}
    # units per wave and per workgroup of the kept elements
    for N in (5, 9, 17):
        upw = 64 // uc.kept_lanes(N)
        counts = uc.unit_counts('kept_elements', N=N)
        assert {upw - 1, upw, upw + 1, 4 * upw - 1, 4 * upw, 4 * upw + 1} - {0} == set(counts)


@pytest.mark.parametrize('cus', CUS)
def test_gather_counts_reach_the_cap_and_the_second_trip(cus):
    counts = uc.unit_counts('gather_pairs', cus)
    occ = {nu: uc.gather_occupancy(nu, cus) for nu in counts}
    cap = uc.GATHER_CAP * cus
    assert [len(occ[nu]) for nu in counts] == [1, 1, 1, 2, cap, cap, cap, cap]
    assert occ[1] == [(1,)] and occ[3] == [(3,)] and occ[4] == [(4,)] and occ[5] == [(4,), (1,)]
    trip = 4 * cap
    assert occ[trip - 1][-1] == (3,) and occ[trip][-1] == (4,)
    assert occ[trip + 1][0] == (4, 1) and occ[trip + 1][1] == (4,)                    # a second trip with three dead waves
    assert occ[2 * trip + 1][0] == (4, 4, 1) and occ[2 * trip + 1][-1] == (4, 4)      # ... and a third


def test_streamed_case_has_three_batches_and_a_ragged_tail():
    b = uc.screen_batches(250, 8, 608, 1)
    assert b == [88, 88, 74] and b[0] % 8 == 0 and b[-1] % 4 != 0


# ---- the traces ----------------------------------------------------------------------------------------------------------
SHAPES = ((3, 64, 16, 7), (3, 64, 16, 9), (3, 64, 17, 14), (8, 600, 100, 7), (4, 16, 4, 7), (5, 16, 4, 9), (9, 300, 50, 7),
          (4, 520, 76, 7), (17, 16, 4, 7))


@pytest.mark.parametrize('N,W,inc,m', SHAPES)
def test_windows_repeat_their_templates_and_the_templates_differ(N, W, inc, m):
    nu = 3 * m + 2
    x = uc.trace(N, W, inc, m, nu)
    assert x.shape == (N, W + (nu - 1) * inc + 1)
    assert planner.window_plan(x.shape[1], uc.FS, uc.winlen(W), uc.overlap(W, inc)) == (W, inc, nu)
    t = uc.templates(N, W, inc, m)
    for w in range(nu):
        assert x[:, w * inc:w * inc + W].tobytes() == t[:, (w % m) * W:(w % m + 1) * W].tobytes()
    for a, b in itertools.combinations(range(m), 2):
        assert not np.array_equal(t[:, a * W:(a + 1) * W], t[:, b * W:(b + 1) * W])
    for rot in (2, 5):
        y = uc.trace(N, W, inc, m, nu, rot=rot)
        for w in range(nu):
            k = (w + rot) % m
            assert y[:, w * inc:w * inc + W].tobytes() == t[:, k * W:(k + 1) * W].tobytes()
    if inc % 2:
        assert m % 2 == 0                      # window and template start on samples of one parity


@pytest.mark.parametrize('N,W,inc,m', SHAPES)
def test_every_template_pair_has_one_best_lag(N, W, inc, m):
    """The best lag of every pair beats the second best by more than GAP |a| |b| (long double, every lag); the reference
    the GPU test uses asserts the same among its candidates."""
    gaps = uc.template_gaps(N, W, inc, m)
    print('N=%d W=%d inc=%d m=%d: smallest gap %.3g' % (N, W, inc, m, gaps.min()))
    assert gaps.min() > uc.GAP
    lag, cmax = uc.template_reference(N, W, inc, m)
    assert lag.shape == (m, N * (N - 1) // 2)
    # the rows a unit is compared by differ between any two templates: every maximum, and the lags of most
    for a, b in itertools.combinations(range(m), 2):
        assert np.all(np.abs(cmax[a] - cmax[b]) > 1e-9), (a, b)
    assert len({lag[k].tobytes() for k in range(m)}) > m // 2


def test_long_window_templates_have_one_best_lag():
    for _, _, W in uc.quantiser_shapes():
        uc.template_reference(3, W, uc.hop_for(W), 7)                 # (asserts the gap among the near-maximal lags)
    s = uc.correlation_shapes()['glob']
    uc.template_reference(s['N'], s['W'], uc.hop_for(s['W']), 7)


@pytest.mark.parametrize('cus', CUS)
def test_m_divides_none_of_a_case_s_distances(cus):
    c = uc.per_xcd(cus)
    cases = [(3, 16, nu) for nu in uc.unit_counts('verify_dma', cus)] + [(3, 17, nu) for nu in (9, 8 * c + 1, 24 * c + 1)]
    cases += [(8, 100, nu) for nu in (1, 9, 8 * c + 1, 250)] + [(3, 16, 3 * uc.ceil_div(8 * c + 1, 3))]
    cases += [(3, 16, nu) for w in (1, 2, 3, 4) for nu in uc.unit_counts('xcd_item', cus, N=3, waves=w)]
    cases += [(9, 50, nu) for nu in uc.unit_counts('xcd_item', cus)]
    cases += [(4, 4, nu) for nu in uc.unit_counts('gather_pairs', cus) + uc.unit_counts('pack_weights', mask_bytes=1)]
    cases += [(5, 4, nu) for nu in uc.unit_counts('solve_ols') + uc.unit_counts('kept_elements', N=5)]
    cases += [(9, 4, nu) for nu in uc.unit_counts('pack_weights', mask_bytes=5) + uc.unit_counts('kept_elements', N=9)]
    used = set()
    for N, inc, nu in cases:
        m = uc.choose_m(nu, N, cus, inc)
        d = uc.distances(nu, N, cus)
        assert {1, 2, 4, 8, 16, 32, 64, 256, c, 8 * c, 8 * cus, 32 * cus, uc.ceil_div(nu, 8), uc.ceil_div(nu * N, 8)} == set(d)
        assert all(k % m for k in d), (N, inc, nu, m)
        assert (m % 2 == 0) == (inc % 2 == 1)
        used.add(m)
    assert 7 in used
    assert uc.choose_m(49 * 8, 1, 256, 16) == 9                        # a share that is a multiple of 7


def test_solve_cases_have_templates_the_sampled_confidence_intervals_can_judge():
    """Every solve case's templates, through the oracle alone: the sampled confidence intervals lie within half their
    tolerance of the closed form (an ellipse that passes the origin closely is a weakness of the sampled reference)."""
    cases = [(4, 16, 4, 0.5, uc.unit_counts('solve_lts_wave') + uc.unit_counts('pack_weights', mask_bytes=1)),
             (8, 16, 4, 0.5, uc.unit_counts('solve_lts_wave')), (5, 16, 4, 1.0, uc.unit_counts('solve_ols')),
             (9, 16, 4, 0.5, uc.unit_counts('pack_weights', mask_bytes=5)), (8, 600, 100, 0.5, [250])]
    for N, W, inc, alpha, counts in cases:
        for m in sorted({uc.choose_m(nu, N, 256, inc) for nu in counts}):
            seed = uc.solve_seed(N, W, inc, m, alpha)
            gap = uc.sampler_gap(N, W, inc, m, alpha, seed)
            print('N=%d W=%d inc=%d m=%d alpha=%g: seed %d, sampled against closed form %.3g of the tolerance' % (N, W, inc, m, alpha, seed, gap))
            assert gap <= 0.5
            assert uc.template_gaps(N, W, inc, m, seed).min() > uc.GAP


# ---- the routes ------------------------------------------------------------------------------------------------------------
def test_correlation_shapes_take_the_routes_they_are_named_for():
    shapes = uc.correlation_shapes()
    for name, (N, W) in (('dma', (3, 600)), ('lds', (9, 300)), ('glob', (3, 6742))):
        assert (shapes[name]['N'], shapes[name]['W']) == (N, W)
    for name, s in shapes.items():
        for npts_pad in (64, 1 << 20):
            r = _hip.route(s['N'], s['W'], npts_pad=npts_pad)
            assert r['correlator'] == _hip.ROUTE_SCREEN, (name, r)
            assert all(r[k] == v for k, v in s['expect'].items()), (name, r)
    short = shapes['dma_short']
    assert short['W'] < 600 and _hip.route(3, short['W'], vrows=3)['verifier'] == 1
    if short['W'] > 64:
        assert _hip.route(3, short['W'] - 1)['verifier'] != 1 or _hip.route(3, short['W'] - 1)['correlator'] != _hip.ROUTE_SCREEN
    for qi, qw, W in uc.quantiser_shapes():
        r = _hip.route(3, W)
        assert (r['quant_inst'], r['quant_waves']) == (qi, qw)
    for N in (4, 5, 8, 9, 17):                                          # W = 16 never screens: the general correlators
        assert _hip.route(N, 16)['correlator'] != _hip.ROUTE_SCREEN
    assert _hip.lag_limit_form(17, 48, 0) == 2 and _hip.lag_seed_form(17, 65, 9, 0) == 2
    assert _hip.route(4, 64)['correlator'] == _hip.ROUTE_SCREEN and _hip.route(4, uc.BEAM_WAVE_W + 8)['correlator'] == _hip.ROUTE_SCREEN
