"""The references of the CLEAN-SC components against each other and against the definition's consequences (tests/clean_truth.py;
DESIGN.md section 24.3), the host helpers ``clean_map`` / ``clean_sources`` on designed component lists, and the
demonstration of section 24.4.  CPU only."""
import functools

import numpy as np
import pytest

import capon_truth as ct
import clean_cases as cc
import clean_truth as clt
import peaks_truth as pt
from narrow_band_least_squares_amd import planner, synthetic, clean_map, clean_sources

FS = cc.FS


@functools.lru_cache(maxsize=None)
def matrices(N, W, Ls, Hs, G):
    """The float64 matrices of an input set's windows (capon_truth's stage A, rounded) and the plan's steering table."""
    data, rij = cc.traces(N, W)
    xij = planner.co_array(rij)[0]
    coef, steer = ct.tables(xij, cc.grid(G), FS, cc.FREQ, Ls, N)
    inc, nwin = cc.windows(W, data.shape[1])
    R, _ = ct.csdm_reference(data, coef, W, inc, nwin, Hs)
    return R.astype(np.complex128), steer


def _walk(R, steer, iterations, gain, floor, label):
    """(a) within (b), step by step along (a)'s own path -> (the reference's dict, worst ratio, waived stop decisions)."""
    ref = clt.clean_reference(R, steer, iterations, gain, floor, history=True)
    worst, waived, eig = 0.0, 0, 0.0
    p0 = tol0 = None
    for i, (R_i, P, g) in enumerate(ref['steps']):
        stopped = i >= ref['count']
        R_n = ref['steps'][i + 1][0] if i + 1 < len(ref['steps']) else ref['R']
        st = clt.check_step('%s i=%d' % (label, i), R_i, steer, gain, floor, i, p0, tol0, stopped, g, gain * P[g] if g >= 0 else np.nan, R_n)
        waived += st['waived']
        if i == 0:
            p0, tol0 = st['p'], st['tol']
        if stopped:
            break
        worst = max(worst, st['worst'])
        eig += 2.0 * float(st['tolR'].sum())
        clt.invariants('%s i=%d' % (label, i), R_i, R_n, st['tolR'], eig)
    return ref, worst, waived


@pytest.mark.parametrize('W,Ls,Hs', cc.SHAPES)
@pytest.mark.parametrize('G', cc.GRID_SIZES)
@pytest.mark.parametrize('N', cc.ELEMENTS)
def test_float64_restatement_within_the_long_double_step(N, G, W, Ls, Hs):
    """Every input set of the GPU tests — every N, G, gain and shape of tests/clean_cases.py —: (a) within (b) at every step,
    no stop decision waived (the condition that licenses the GPU test's 1 %), the trace non-increasing and the smallest
    eigenvalue above the summed bounds."""
    worst = 0.0
    R, steer = matrices(N, W, Ls, Hs, G)
    for gain in cc.GAINS:
        for w in range(len(R)):
            ref, r, waived = _walk(R[w], steer, cc.STEPS, gain, cc.FLOOR, 'N=%d G=%d gain=%g w=%d' % (N, G, gain, w))
            assert waived == 0, 'a condition on the inputs: change the seed'
            assert ref['count'] >= 1 and ref['residual'] <= ref['total']
            worst = max(worst, r)
    print('N=%d G=%d W=%d: worst |dR| / bound of (a) against (b) %.3g' % (N, G, W, worst))


def _rank_one(N, g, power=3.5):
    rij = cc.geometry(N)
    _, steer = ct.tables(planner.co_array(rij)[0], cc.grid(129), FS, cc.FREQ, 16, N)
    a = steer[g]
    return power * np.outer(a, np.conj(a)), steer


@pytest.mark.parametrize('N', cc.ELEMENTS)
def test_one_wave_at_a_grid_point(N):
    R, steer = _rank_one(N, 17)
    ref = clt.clean_reference(R, steer, 8, 1.0, 0.02)
    assert ref['count'] == 1 and ref['index'][0] == 17 and np.all(ref['index'][1:] == -1) and np.all(np.isnan(ref['power'][1:]))
    st = clt.clean_step(R, steer, 1.0)
    assert abs(ref['power'][0] - ref['total']) <= st['tolP'][17] + 4 * N * clt.U * ref['total']
    assert abs(ref['residual']) <= 1e-12 * ref['total']


def test_one_iteration_and_no_floor():
    R, steer = matrices(8, 65, 16, 8, 129)
    one = clt.clean_reference(R[0], steer, 1, 0.5, 0.02)
    many = clt.clean_reference(R[0], steer, 32, 0.5, 0.0)
    assert one['count'] == 1 and many['count'] == 32
    assert one['index'][0] == many['index'][0] and one['power'][0] == many['power'][0]
    assert np.all(np.diff(many['power']) <= 0) and 0 < many['residual'] < one['residual'] < one['total']
    five = clt.clean_reference(R[0], steer, 5, 0.5, 0.0)
    assert np.array_equal(five['index'], many['index'][:5]) and np.array_equal(five['power'], many['power'][:5])
    floored = clt.clean_reference(R[0], steer, 32, 0.5, 0.5)
    c = floored['count']
    assert 1 <= c < 32 and np.array_equal(floored['index'][:c], many['index'][:c])
    assert many['power'][c] < 0.5 * many['power'][0] <= many['power'][c - 1] or c == 1


def test_degenerate_units():
    R, steer = matrices(3, 65, 16, 8, 129)
    for bad in (np.zeros((3, 3), dtype=complex), np.where(np.eye(3, dtype=bool), np.nan, R[0])):
        ref = clt.clean_reference(bad, steer, 4, 0.5, 0.02)
        assert ref['count'] == 0 and np.all(ref['index'] == -1) and np.all(np.isnan(ref['power']))
        assert np.isnan(ref['total']) and np.isnan(ref['residual'])
    nan_off = R[0].copy()
    nan_off[2, 0] = np.nan
    assert clt.clean_reference(nan_off, steer, 4, 0.5, 0.02)['count'] == 0


@pytest.mark.parametrize('dropped,rows', [(1, [1, 2, 3, 4, 5, 6, 7]), (1 << 3, [0, 1, 2, 4, 5, 6, 7]), (1 << 7, [0, 1, 2, 3, 4, 5, 6]),
                                          (0b00111111, list(range(8))), (0, list(range(8)))])
def test_kept_elements(dropped, rows):
    """Element 0, a middle one and the last dropped: (a) on the mask is (a) on the compacted matrix with the kept rows of the
    table, scattered back; fewer than 3 left: the whole array."""
    R, steer = matrices(8, 65, 16, 8, 129)
    assert clt.kept_rows(dropped, 8) == rows
    ref = clt.clean_reference(R[1], steer, 5, 0.5, 0.02, dropped=dropped)
    small = clt.clean_reference(R[1][np.ix_(rows, rows)], steer[:, rows], 5, 0.5, 0.02)
    for k in ('count', 'total', 'residual'):
        assert ref[k] == small[k]
    assert np.array_equal(ref['index'], small['index']) and np.array_equal(ref['power'], small['power'], equal_nan=True)
    gone = [e for e in range(8) if e not in rows]
    assert np.array_equal(ref['R'][np.ix_(rows, rows)], small['R']) and not ref['R'][gone].any() and not ref['R'][:, gone].any()
    _walk(R[1][np.ix_(rows, rows)], steer[:, rows], 5, 0.5, 0.02, 'kept %d' % dropped)


def test_clean_map_and_sources_on_designed_lists():
    ax = np.arange(5) * 0.1
    g0, g1 = np.meshgrid(ax, ax, indexing='ij')
    grid = np.stack([g0.ravel(), g1.ravel()], axis=1)               # 5 x 5, step 0.1; index = 5 i + j
    I = 6
    def lists(comps):
        idx, pw = np.full(I, -1, dtype=np.int32), np.full(I, np.nan)
        idx[:len(comps)], pw[:len(comps)] = [c[0] for c in comps], [c[1] for c in comps]
        return idx, pw, len(comps)
    cases = [lists([(0, 4.0), (24, 3.0), (1, 2.0), (23, 1.0), (0, 0.5)]),         # two clusters
             lists([(6, 2.0), (18, 2.0)]),                                       # a tie in power: the lower rank leads
             lists([(12, 1.0), (11, 3.0), (13, 2.0), (7, 0.5)]),                 # everything within one radius
             lists([(0, 5.0), (4, 4.0), (20, 3.0), (24, 2.0), (12, 1.0)]),       # more clusters than max_sources
             lists([])]                                                          # count 0
    index = np.stack([c[0] for c in cases])
    power = np.stack([c[1] for c in cases])
    count = np.array([c[2] for c in cases])
    m = clean_map(index, power, count, 25)
    assert m.shape == (5, 25) and m[0, 0] == 4.5 and m[0, 24] == 3.0 and m[0, 1] == 2.0 and m[0, 23] == 1.0
    np.testing.assert_allclose(m.sum(axis=1), [10.5, 4.0, 6.5, 15.0, 0.0])
    assert not m[4].any()
    pw, sl, vel, baz = clean_sources(index, power, count, grid, 0.15, 3)
    assert pw.shape == (5, 3) and sl.shape == (5, 3, 2)
    np.testing.assert_allclose(pw[0], [6.5, 4.0, np.nan])
    np.testing.assert_allclose(sl[0, 0], [0.0, 0.1 * 2.0 / 6.5])
    np.testing.assert_allclose(sl[0, 1], [0.4, (0.4 * 3.0 + 0.3 * 1.0) / 4.0])
    np.testing.assert_allclose(pw[1], [2.0, 2.0, np.nan])
    np.testing.assert_allclose(sl[1, :2], [grid[6], grid[18]])
    np.testing.assert_allclose(pw[2], [4.5, 2.0, np.nan])           # led by 11: 12 and 7 are within 0.15 of it, 13 is 0.2 away
    pw2 = clean_sources(index[2], power[2], count[2], grid, 0.25, 3)[0]      # everything within one radius
    np.testing.assert_allclose(pw2, [6.5, np.nan, np.nan])
    np.testing.assert_allclose(pw[3], [5.0, 4.0, 3.0])
    assert np.all(np.isnan(pw[4])) and np.all(np.isnan(sl[4])) and np.all(np.isnan(vel[4])) and np.all(np.isnan(baz[4]))
    np.testing.assert_allclose(vel[1, 0], 1.0 / np.hypot(0.1, 0.1))
    np.testing.assert_allclose(baz[1, 0], 45.0)


# ---- the demonstration ----
RADIUS = 0.45
# sources (baz degrees, velocity km/s, amplitude); ``found``: windows of 19 in which truth (a) with clean_sources finds every
# source within RADIUS s/km on the 81 x 81 grid, as measured
DEMO = [dict(sources=[(50.0, 0.34, 1.0), (70.0, 0.34, 1.0)]),
        dict(sources=[(50.0, 0.34, 1.0), (70.0, 0.34, 0.316)]),
        dict(sources=[(50.0, 0.34, 1.0), (110.0, 0.34, 0.316)]),
        dict(sources=[(50.0, 0.34, 1.0), (110.0, 0.34, 0.7), (200.0, 0.34, 0.5)])]


def source_slowness(sources):
    return np.array([[np.sin(np.radians(b)) / v, np.cos(np.radians(b)) / v] for b, v, _ in sources])


@functools.lru_cache(maxsize=None)
def demo_case(row):
    """Row ``row`` of the table: section 18.4's call (N = 8, 0.45 - 0.55 Hz, seed 4242, 10 dB, 19 windows of 2400 samples) with
    the row's sources -> (centred rij, data, sources, W, inc)."""
    N, W, inc = 8, 2400, 1200
    rij = synthetic.array_geometry(N, 1.0)
    rij = rij - rij.mean(axis=1, keepdims=True)
    sources = DEMO[row]['sources']
    data = synthetic.plane_waves(rij, W + 18 * inc + 1, FS, 0.45, 0.55, sources, snr_db=10.0, seed=4242)
    return rij, data, sources, W, inc


def demo_grid(n=81):
    ax = np.linspace(-4.0, 4.0, n)
    g0, g1 = np.meshgrid(ax, ax, indexing='ij')
    grid = np.ascontiguousarray(np.stack([g0.ravel(), g1.ravel()], axis=1))
    return grid, planner.grid_cells(grid)[0]


def demo_patch():
    """21 x 21 points, step 0.1 s/km, around the slowness of 60 degrees at 0.34 km/s: rows 1 and 2 lie inside."""
    centre = np.array([np.sin(np.radians(60.0)), np.cos(np.radians(60.0))]) / 0.34
    ax = np.arange(-10, 11) * 0.1
    g0, g1 = np.meshgrid(centre[0] + ax, centre[1] + ax, indexing='ij')
    grid = np.ascontiguousarray(np.stack([g0.ravel(), g1.ravel()], axis=1))
    return grid, planner.grid_cells(grid)[0]


def found_every_source(slowness, sources):
    """Every source has one of the slowness vectors (S, 2; NaN rows are none) within RADIUS s/km."""
    s = np.asarray(slowness, dtype=np.float64)
    s = s[~np.isnan(s).any(axis=1)]
    return bool(len(s)) and all(np.hypot(s[:, 0] - t[0], s[:, 1] - t[1]).min() <= RADIUS for t in source_slowness(sources))


def source_powers(index, power, count, grid, sources):
    """One window's components -> (the summed power of the components within RADIUS of each source (S,), the summed power of
    those outside every radius)."""
    c = int(count)
    truth = source_slowness(sources)
    comp = np.asarray(grid)[np.asarray(index)[:c]]
    pw = np.asarray(power)[:c]
    d = np.hypot(comp[:, None, 0] - truth[None, :, 0], comp[:, None, 1] - truth[None, :, 1])
    return np.array([pw[d[:, k] <= RADIUS].sum() for k in range(len(sources))]), float(pw[d.min(axis=1) > RADIUS].sum()) if c else 0.0


STRAY = 0.05          # the median power outside every radius, over the strongest source's: 0 as measured; one component at the
                      # floor f = 0.02 of p_0 with gain 0.5 against a source of about 2 p_0 is 0.005, so 0.05 is ten of them


def peak_lists_find(maps, grid, cells, sources):
    """Windows in which the K strongest local maxima of the map (peaks_truth, floor 0) are the K sources."""
    idx = pt.peaks_of_maps(np.asarray(maps, dtype=np.float64), cells, len(sources), 0.0)[1]
    return sum(bool(np.all(i >= 0)) and found_every_source(grid[i], sources) for i in idx)


@pytest.mark.parametrize('row', range(4))
def test_demonstration(row):
    rij, data, sources, W, inc = demo_case(row)
    N, S = 8, len(sources)
    grid, cells = demo_grid()
    xij = planner.co_array(rij)[0]
    Ls, Hs = planner.capon_snapshots(xij, grid, FS, [0.5], [W])
    coef, steer = ct.tables(xij, grid, FS, 0.5, Ls[0], N)
    R, _ = ct.csdm_reference(data, coef, W, inc, 19, int(Hs[0]))
    R = R.astype(np.complex128)
    found, powers, stray, left, counts = 0, [], [], [], []
    for w in range(19):
        ref = clt.clean_reference(R[w], steer, 32, 0.5, 0.02)
        c = ref['count']
        pw, sl = clean_sources(ref['index'], ref['power'], c, grid, RADIUS, S + 2)[:2]
        found += found_every_source(sl, sources)
        per, out = source_powers(ref['index'], ref['power'], c, grid, sources)
        powers.append(per)
        stray.append(out)
        left.append(ref['residual'] / ref['total'])
        counts.append(c)
    maps = [ct.spectra_reference(R[w], steer, 0.01) for w in range(19)]
    bartlett = peak_lists_find([m['PB'] for m in maps], grid, cells, sources)
    capon = peak_lists_find([m['PC'] for m in maps], grid, cells, sources)
    med = np.median(np.array(powers), axis=0)
    print('demonstration row %d: CLEAN-SC %d / 19, Capon peaks %d, Bartlett peaks %d; components %d..%d; median source powers %s, '
          'outside every radius %.4g, residual / total %.3f' % (row + 1, found, capon, bartlett, min(counts), max(counts),
                                                                 np.array2string(med, precision=1), np.median(stray), np.median(left)))
    want = MEASURED[row]
    assert found >= want['found'] - 2
    assert found > bartlett
    if row in (1, 2):
        assert found >= capon
    amp2 = np.array([a * a for _, _, a in sources])
    ratio = (med / med[0]) / (amp2 / amp2[0])
    assert np.all(ratio <= 2.0 * np.array(want['ratio'])) and np.all(ratio >= 0.5 * np.array(want['ratio']))
    assert np.median(stray) <= STRAY * med[0]


# What truth (a) measures on the 81 x 81 grid (the printed line of test_demonstration).  ``ratio``: the median power of
# source k over source 0's, over the squared-amplitude ratio.  The floor f = 0.02 ends a weak source's geometric series
# sum_i phi (1 - phi)^i early — a source 10 dB down is entered three or four times, 1 - 0.5^4 = 0.94 of it at best, and
# the strong source's sidelobe at its place goes to the strong source —, so the ratio reads low by construction: 0.63 for
# the 10 dB weaker wave, 0.85 and 0.87 for amplitudes 0.7 and 0.5.  Asserted to a factor of two either side.
MEASURED = [dict(found=19, ratio=[1.0, 1.006]),
            dict(found=19, ratio=[1.0, 0.627]),
            dict(found=19, ratio=[1.0, 0.629]),
            dict(found=19, ratio=[1.0, 0.845, 0.866])]
