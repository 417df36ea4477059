"""The NumPy restatement of the peak request (tests/peaks_truth.py) against ``capon_truth.local_maxima``
on full Cartesian grids, on a disc grid, on designed maps, and on the long-double reference maps of the two-source
demonstration of DESIGN.md section 18.4, where it must reproduce the counts of ``capon_truth.both_found``.  CPU only."""
import numpy as np
import pytest

import capon_truth as ct
import peaks_truth as pt
from narrow_band_least_squares_amd import planner, synthetic

FS = 20.0


def _full(n0, n1):
    i0, i1 = np.meshgrid(np.arange(n0), np.arange(n1), indexing='ij')
    return np.stack([i0.ravel(), i1.ravel()], axis=1)


@pytest.mark.parametrize('shape', [(1, 1), (1, 7), (6, 1), (5, 4), (9, 9)])
def test_same_peaks_in_the_same_order_as_local_maxima_on_full_grids(shape):
    rng = np.random.default_rng(sum(shape))
    cells = _full(*shape)
    G = len(cells)
    for trial in range(40):
        P = np.round(rng.random(G), 1 if trial % 2 else 6)           # one decimal: plenty of ties
        count, index, power, _ = pt.peaks(P, cells, 8, 0.0)
        want = ct.local_maxima(P, shape)
        assert count == len(want) >= 1
        np.testing.assert_array_equal(index[:min(count, 8)], want[:8])
        np.testing.assert_array_equal(power[:min(count, 8)], P[want[:8]])
        assert np.all(index[count:] == -1) and np.all(np.isnan(power[count:]))
        assert index[0] == ct.argmax_total(P)                        # the arg-max is always a peak, and rank 0


def test_neighbour_table():
    cells = _full(3, 3)
    nbr = pt.neighbours(cells)
    assert nbr.shape == (8, 9) and nbr.dtype == np.int32
    assert list(nbr[:, 4]) == [1, 7, 3, 5, 0, 2, 6, 8]               # (-1,0) (+1,0) (0,-1) (0,+1) (-1,-1) (-1,+1) (+1,-1) (+1,+1)
    assert list(nbr[:, 0]) == [-1, 3, -1, 1, -1, -1, -1, 4]
    perm = np.random.default_rng(1).permutation(9)
    nbr_p = pt.neighbours(cells[perm])
    inv = np.argsort(perm)
    for g in range(9):
        for d in range(8):
            assert nbr_p[d, inv[g]] == (-1 if nbr[d, g] < 0 else inv[nbr[d, g]])


def test_disc_grid_border_points_compare_with_what_they_have():
    grid = planner.slowness_grid(4.0, 9)
    cells, steps = planner.grid_cells(grid)
    assert len(grid) == 49 and np.all(steps == 1.0)
    # embed in the 9 x 9 square with -inf outside the disc: local_maxima on the square is the truth on the disc
    rng = np.random.default_rng(9)
    for _ in range(40):
        P = np.round(rng.random(49), 1)
        sq = np.full((9, 9), -np.inf)
        sq[cells[:, 0], cells[:, 1]] = P
        flat = {int(i) * 9 + int(j): g for g, (i, j) in enumerate(cells)}
        want = [flat[k] for k in ct.local_maxima(sq.ravel(), (9, 9)) if k in flat]
        count, index, _, _ = pt.peaks(P, cells, 8, 0.0)
        assert count == len(want) and list(index[:min(count, 8)]) == want[:8]
    # a border point with three neighbours only
    g = int(np.flatnonzero((cells[:, 0] == 0) & (cells[:, 1] == 4))[0])
    assert sorted(int(n) for n in pt.neighbours(cells)[:, g] if n >= 0) == sorted(
        int(np.flatnonzero((cells[:, 0] == 1) & (cells[:, 1] == j))[0]) for j in (3, 4, 5))
    P = np.zeros(49)
    P[g] = 1.0
    count, index, power, offset = pt.peaks(P, cells, 2, 0.5)
    assert count == 1 and index[0] == g and list(offset[0]) == [0.0, 0.0]     # no -1 neighbour on axis 0; a flat line on axis 1


def test_designed_maps():
    cells = _full(5, 5)
    at = lambda i, j: i * 5 + j
    # a 2 x 3 plateau: exactly the lowest-index point is the peak
    P = np.zeros(25)
    block = [at(1, 1), at(1, 2), at(1, 3), at(2, 1), at(2, 2), at(2, 3)]
    P[block] = 2.0
    count, index, power, offset = pt.peaks(P, cells, 8, 0.0)
    plateau = [int(g) for g in index[:count] if g in block]
    assert plateau == [at(1, 1)] and index[0] == at(1, 1) and power[0] == 2.0
    # NaN holes beside a maximum do not compete, and are no peaks
    P = np.full(25, 0.5)
    P[at(2, 2)] = 3.0
    P[[at(2, 1), at(1, 2), at(3, 3)]] = np.nan
    count, index, power, offset = pt.peaks(P, cells, 8, 1.0)
    assert count == 1 and index[0] == at(2, 2) and list(offset[0]) == [0.0, 0.0]      # a NaN neighbour: offset 0 on that axis
    assert not np.isin(pt.peaks(P, cells, 8, 0.0)[1], [at(2, 1), at(1, 2), at(3, 3)]).any()
    # an all-NaN map
    count, index, power, offset = pt.peaks(np.full(25, np.nan), cells, 3, 0.25)
    assert count == 0 and np.all(index == -1) and np.all(np.isnan(power)) and np.all(np.isnan(offset))
    # more peaks than ranks: the count is not capped, the K best are returned in order
    P = np.zeros(25)
    tops = [at(0, 0), at(0, 2), at(0, 4), at(2, 0), at(2, 2), at(2, 4), at(4, 0), at(4, 2), at(4, 4)]
    P[tops] = [5.0, 9.0, 1.0, 7.0, 3.0, 8.0, 2.0, 6.0, 4.0]
    count, index, power, _ = pt.peaks(P, cells, 4, 0.0)
    assert count == 9 and list(index) == [at(0, 2), at(2, 4), at(2, 0), at(4, 2)] and list(power) == [9.0, 8.0, 7.0, 6.0]
    # the floor: 0 keeps every peak, 0.25 those of at least 2.25, 1.0 the maximum (and its equals) only
    assert pt.peaks(P, cells, 8, 0.0)[0] == 9 and pt.peaks(P, cells, 8, 0.25)[0] == 7 and pt.peaks(P, cells, 8, 1.0)[0] == 1
    P[at(4, 4)] = 9.0
    count, index, _, _ = pt.peaks(P, cells, 8, 1.0)
    assert count == 2 and list(index[:2]) == [at(0, 2), at(4, 4)]
    # a negative maximum: the arg-max is kept although P < floor * P (floor * P is above it)
    count, index, _, _ = pt.peaks(-1.0 - np.arange(25.0), cells, 2, 0.5)
    assert count == 1 and index[0] == 0


def test_offsets():
    cells = _full(5, 5)
    at = lambda i, j: i * 5 + j
    # the vertex of a parabola through three points, positive towards the +1 neighbour
    P = np.zeros(25)
    P[at(2, 2)], P[at(1, 2)], P[at(3, 2)], P[at(2, 1)], P[at(2, 3)] = 4.0, 1.0, 3.0, 2.0, 2.0
    _, index, _, offset = pt.peaks(P, cells, 1, 0.0)
    assert index[0] == at(2, 2) and offset[0, 0] == 0.5 * (1.0 - 3.0) / ((1.0 - 8.0) + 3.0) == 0.25 and offset[0, 1] == 0.0
    assert pt.fraction(1.0, 4.0, 3.0) == 0.25 and pt.fraction(3.0, 4.0, 1.0) == -0.25
    # a maximum on the lattice edge: offset 0 on the axis that lacks a neighbour
    P = np.zeros(25)
    P[at(0, 2)], P[at(1, 2)], P[at(0, 1)], P[at(0, 3)] = 4.0, 3.0, 1.0, 3.0
    _, index, _, offset = pt.peaks(P, cells, 1, 0.0)
    assert index[0] == at(0, 2) and offset[0, 0] == 0.0 and offset[0, 1] == 0.25
    # three collinear equal values: denominator 0, so offset 0; -0.0 becomes 0.0
    assert pt.fraction(2.0, 2.0, 2.0) == 0.0
    z = pt.fraction(1.0, 2.0, 1.0)
    assert z == 0.0 and not np.signbit(z)
    # no strict maximum, and values that are not finite
    assert pt.fraction(1.0, 2.0, 3.0) == 0.0 and pt.fraction(3.0, 1.0, 3.0) == 0.0
    assert pt.fraction(np.inf, 2.0, 1.0) == 0.0 and pt.fraction(np.nan, 2.0, 1.0) == 0.0 and pt.fraction(1.0, np.inf, 1.0) == 0.0
    # the clamp at +-0.5: an equal neighbour (the index order made g the peak) puts the vertex half a step away, and rounding
    # may put it beyond
    assert pt.fraction(1.0, 2.0, 2.0) == 0.5 and pt.fraction(2.0, 2.0, 1.0) == -0.5
    assert 0.5 * (1.0 + 2.0 ** -52) / (1.0 - 2.0 ** -52) > 0.5 and pt.fraction(0.0, 1.0, 1.0 + 2.0 ** -52) == 0.5
    P = np.zeros(25)
    P[at(2, 2)], P[at(2, 3)] = 5.0, 5.0
    _, index, _, offset = pt.peaks(P, cells, 1, 0.0)
    assert index[0] == at(2, 2) and offset[0, 1] == 0.5 and offset[0, 0] == 0.0


def test_maps_at_once_and_bits():
    cells = _full(4, 4)
    maps = np.random.default_rng(3).random((5, 16))
    maps[2] = np.nan
    count, index, power, offset = pt.peaks_of_maps(maps, cells, 3, 0.25)
    assert count.dtype == np.int32 and index.dtype == np.int32 and index.shape == (5, 3) and offset.shape == (5, 3, 2)
    for w in range(5):
        one = pt.peaks(maps[w], cells, 3, 0.25)
        assert one[0] == count[w] and pt.same_bits(one[1], index[w]) and pt.same_bits(one[2], power[w]) and pt.same_bits(one[3], offset[w])
    assert count[2] == 0
    assert pt.same_bits(np.array([np.nan, 0.0]), np.array([np.nan, 0.0])) and not pt.same_bits(np.array([0.0]), np.array([-0.0]))


# ---- the two-source demonstration of DESIGN.md section 18.4 on the long-double reference maps ----

ROWS = [(8, 0.5, 20.0, 10.0, 18, 3), (8, 1.0, 10.0, 10.0, 19, 4), (16, 0.5, 15.0, 10.0, 17, 0), (4, 0.5, 25.0, 10.0, 19, 1),
        (8, 0.5, 20.0, 0.0, 19, 3)]          # N, f (Hz), separation (deg), SNR (dB), then the counts of section 18.4: Capon, Bartlett


def _reference_maps(N, f, sep, snr):
    W, inc, n = 2400, 1200, 81
    rij = synthetic.array_geometry(N, 1.0)
    rij = rij - rij.mean(axis=1, keepdims=True)
    baz = (60.0 - sep / 2, 60.0 + sep / 2)
    data = synthetic.plane_waves(rij, W + 18 * inc + 1, FS, 0.9 * f, 1.1 * f, [(baz[0], 0.34, 1.0), (baz[1], 0.34, 1.0)], snr_db=snr,
                                 seed=4242)
    ax = np.linspace(-4.0, 4.0, n)
    g0, g1 = np.meshgrid(ax, ax, indexing='ij')
    grid = np.ascontiguousarray(np.stack([g0.ravel(), g1.ravel()], axis=1))
    xij = planner.co_array(rij)[0]
    fc = planner.capon_frequencies([(0.9 * f, 1.1 * f)])
    Ls, Hs = planner.capon_snapshots(xij, grid, FS, fc, [W])
    coef, steer = ct.tables(xij, grid, FS, fc[0], Ls[0], N)
    R, _ = ct.csdm_reference(data, coef, W, inc, 19, int(Hs[0]))
    refs = [ct.spectra_reference(R[w].astype(np.complex128), steer, 0.01) for w in range(19)]
    return grid, (n, n), baz, refs


def _circ(a, b):
    return abs((a - b + 180.0) % 360.0 - 180.0)


def _both(index, count, grid, baz):
    """``both_found``'s criterion on the ranks 0 and 1 of the truth at K = 2, floor 0.25."""
    if count < 2:
        return False
    b = ct.grid_baz(grid, index[:2])
    sep = _circ(baz[0], baz[1])
    return bool((_circ(b[0], baz[0]) <= sep / 3 and _circ(b[1], baz[1]) <= sep / 3) or
                (_circ(b[0], baz[1]) <= sep / 3 and _circ(b[1], baz[0]) <= sep / 3))


@pytest.mark.parametrize('N,f,sep,snr,capon,bartlett', ROWS)
def test_the_demonstration_counts_through_the_peaks(N, f, sep, snr, capon, bartlett):
    """The same rule as ``both_found``'s own ``local_maxima``, so the counts of section 18.4 must come out, window by window.
    Also measured here: are the refined back-azimuths of the two peaks closer to the true ones than the grid points'?  Median
    absolute error over the two peaks of the windows with both sources, degrees (grid step 0.1 s/km), on the Capon map:
        N = 8,  0.5 Hz, 20 deg, 10 dB   grid 0.393   refined 0.113
        N = 8,  1.0 Hz, 10 deg, 10 dB   grid 0.225   refined 0.060
        N = 8,  0.5 Hz, 20 deg,  0 dB   grid 0.346   refined 0.133
        N = 16, 0.5 Hz, 15 deg, 10 dB   grid 0.630   refined 0.380
        N = 4,  0.5 Hz, 25 deg, 10 dB   grid 0.259   refined 0.457   (worse: four elements, two sources, a skewed lobe)
    Asserted at N = 8 only, which is what was asked: refined <= 0.6 grid (measured ratios 0.29, 0.27, 0.38).  On the Bartlett
    map the two sources are found in 0 to 4 windows, too few for a median, and the parabola on a merged lobe does not
    help (all its count >= 2 windows: 1.95 -> 1.92, 0.78 -> 1.44, 1.95 -> 1.92 degrees): nothing is asserted there."""
    grid, shape, baz, refs = _reference_maps(N, f, sep, snr)
    cells, steps = planner.grid_cells(grid)
    nbr = pt.neighbours(cells)
    assert np.array_equal(cells, _full(*shape))
    found = dict(PC=0, PB=0)
    err = dict(grid=[], refined=[])
    for ref in refs:
        for name in ('PC', 'PB'):
            P = np.asarray(ref[name], dtype=np.float64)
            count, index, power, offset = pt.peaks(P, cells, 2, 0.25, nbr)
            both = _both(index, count, grid, baz)
            assert both == bool(ct.both_found(P, grid, shape, baz))
            found[name] += both
            if both and name == 'PC':
                for k in range(2):
                    s = grid[index[k]] + offset[k] * steps
                    true = min(baz, key=lambda b: _circ(ct.grid_baz(grid, index[k]), b))
                    err['grid'].append(_circ(ct.grid_baz(grid, index[k]), true))
                    err['refined'].append(_circ(np.mod(np.degrees(np.arctan2(s[0], s[1])), 360.0), true))
    print('N=%d f=%.1f sep=%g snr=%g: Capon %d / 19, Bartlett %d / 19; Capon baz error, median: grid %.3f, refined %.3f deg'
          % (N, f, sep, snr, found['PC'], found['PB'], np.median(err['grid']), np.median(err['refined'])))
    assert (found['PC'], found['PB']) == (capon, bartlett)
    if N == 8:
        assert np.median(err['refined']) <= 0.6 * np.median(err['grid'])
