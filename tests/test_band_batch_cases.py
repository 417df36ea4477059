"""The conditions of the case of tests/band_batch_cases.py, on the CPU: the truths (``filter_truth``'s long-double band-pass,
``grid_truth``, ``seeded_truth``, ``refine_truth``, ``capon_truth``) show that the two bands' tables cannot be mixed up, nor
the row formulas, without a result moving by far more than any tolerance — so that tests/test_gpu_band_batch.py, which
compares bits, would see it — and that the checkers that test reuses meet their own conditions on this case.  If one of
these fails, the seeds or the tables of the case change, never a margin."""
import numpy as np
import pytest

import band_batch_cases as bb
import capon_truth as ct
import grid_truth as gt
import refine_truth as rt
import seeded_truth as sdt
from narrow_band_least_squares_amd import planner

MARGIN = 1000.0          # a spectrum made with the other band's tables is this many summed truth bounds away, at least


@pytest.fixture(scope='module')
def geometry():
    _, rij, _ = bb.recordings()
    xij, pair_idx, _ = planner.co_array(rij)
    return xij, [tuple(p) for p in pair_idx]


@pytest.fixture(scope='module')
def spectra(geometry):
    """[s][b][tables of band t] -> the list of ``capon_truth.spectra_reference`` per window of band b of recording s."""
    xij, _ = geometry
    out = {}
    for s in range(bb.S):
        for b, (W, inc, n) in enumerate(bb.window_plans()):
            for t in range(bb.B):
                Ls, Hs = bb.CAPON_SNAPSHOTS[0][t], bb.CAPON_SNAPSHOTS[1][t]
                coef, steer = ct.tables(xij, bb.CAPON_GRID, bb.FS, bb.CAPON_FREQS[t], Ls, bb.N)
                R, _ = ct.csdm_reference(bb.filtered_truth(s, b), coef, W, inc, n, Hs)
                out[s, b, t] = [ct.spectra_reference(R[w].astype(np.complex128), steer, bb.CAPON_LOADING) for w in range(n)]
    return out


@pytest.fixture(scope='module')
def picks(geometry):
    """[s][b] -> (grid reference, lags under the band's own half-width, lags under the other band's, refinement of the own)."""
    xij, pairs = geometry
    d, tau = gt.delay_table(xij, bb.SEED_GRID, bb.FS, bb.N)
    assert not gt.near_tie(tau), 'a delay of the seed grid lies within 1e-6 of a rounding tie: change the grid'
    out = {}
    for s in range(bb.S):
        for b, (W, inc, n) in enumerate(bb.window_plans()):
            filt = bb.filtered_truth(s, b)
            starts = [w * inc for w in range(n)]
            ref = gt.grid_reference(filt, bb.FS, xij, bb.SEED_GRID, W, inc, n)
            c = sdt.centres(d, ref['index'], pairs)
            own, _ = sdt.pick_windows(filt, W, starts, pairs, c, bb.SEED_HALFWIDTHS[b])          # (asserts every gap)
            other, _ = sdt.pick_windows(filt, W, starts, pairs, c, bb.SEED_HALFWIDTHS[1 - b], exact=True)
            out[s, b] = (ref, own, other, rt.refine_windows(filt, W, starts, pairs, own))
    return out


def test_shapes_and_tables_differ():
    """(a)"""
    assert bb.B != bb.S and bb.B >= 2 and bb.S >= 2
    rows = [(r // bb.S, r // bb.B, r % bb.B, r % bb.S) for r in range(bb.B * bb.S)]
    for i in range(4):
        for j in range(i + 1, 4):
            assert [r[i] for r in rows] != [r[j] for r in rows]
    plans = bb.window_plans()
    assert [p[0] for p in plans] == list(bb.WINDOWS) and plans[0][2] != plans[1][2] and min(p[2] for p in plans) >= 3
    for table in (bb.CAPON_FREQS, bb.CAPON_SNAPSHOTS[0], bb.CAPON_SNAPSHOTS[1], bb.SEED_HALFWIDTHS, bb.EDGES, bb.WINLENS):
        assert len(table) == bb.B and len(set(map(repr, table))) == bb.B
    assert len(bb.SEED_GRID) != len(bb.CAPON_GRID)
    data, rij, t0s = bb.recordings()
    assert len(data) == bb.S and all(d.shape == (bb.N, bb.NPTS) for d in data) and rij.shape == (2, bb.N)
    for i in range(bb.S):
        for j in range(i + 1, bb.S):
            assert not np.array_equal(data[i], data[j]) and t0s[i] != t0s[j]
    planner.check_capon(bb.N, bb.CAPON_GRID, bb.CAPON_FREQS, bb.CAPON_SNAPSHOTS, bb.CAPON_LOADING, bb.WINDOWS, True, True)
    planner.check_capon_peaks(len(bb.CAPON_GRID), planner.grid_cells(bb.CAPON_GRID)[0], bb.PEAKS, bb.PEAK_FLOOR)
    # the other band's snapshots fit either window too: a mix-up would not be refused, it would compute
    planner.check_capon(bb.N, bb.CAPON_GRID, bb.CAPON_FREQS[::-1], [t[::-1] for t in bb.CAPON_SNAPSHOTS], bb.CAPON_LOADING,
                        bb.WINDOWS, True, True)


def test_the_other_bands_capon_tables_move_both_spectra_far_beyond_the_bounds(spectra):
    """(b) for every (recording, window) of either band; (d) for every unit of the case."""
    worst = dict(C=np.inf, B=np.inf, kappa=0.0)
    for s in range(bb.S):
        for b, (_, _, n) in enumerate(bb.window_plans()):
            for w in range(n):
                own, other = spectra[s, b, b][w], spectra[s, b, 1 - b][w]
                assert own['chol_ok'] and other['chol_ok'] and not own['degenerate']
                assert own['kappa'] * bb.N * ct.U < 1e-6, (s, b, w)
                worst['kappa'] = max(worst['kappa'], own['kappa'] * bb.N * ct.U)
                for name, P, tol in (('C', 'PC', 'tolC'), ('B', 'PB', 'tolB')):
                    ratio = float(np.max(np.abs(own[P] - other[P]).astype(np.float64) / (own[tol] + other[tol])))
                    assert ratio > MARGIN, (name, s, b, w, ratio)
                    worst[name] = min(worst[name], ratio)
    print('other band\'s tables: smallest largest |difference| / summed bounds, Capon %.3g, Bartlett %.3g; largest kappa N u %.3g'
          % (worst['C'], worst['B'], worst['kappa']))


def test_the_other_bands_half_width_moves_a_lag_of_every_recording(picks):
    """(c)"""
    for s in range(bb.S):
        for b in range(bb.B):
            _, own, other, _ = picks[s, b]
            moved = int(np.count_nonzero(own != other))
            print('recording %d band %d: %d of %d lags differ under half-width %d instead of %d'
                  % (s, b, moved, own.size, bb.SEED_HALFWIDTHS[1 - b], bb.SEED_HALFWIDTHS[b]))
            assert moved >= 1


def test_the_reused_checkers_meet_their_own_conditions(picks):
    """What tests/test_gpu_grid.py, test_gpu_seeded.py and test_gpu_subsample.py ask of a case ("change the seed" otherwise),
    here on the truth's filtered samples: no grid cell is ``power_only``, the grid maximum leads by more than both bounds
    (the GPU's index, and with it the seed, is then the truth's), every pick's best and second-best are MIN_GAP apart
    (asserted by ``pick_windows``), no pick lies at the end of the lag range, every refined pair has a clear maximum, and
    most fractions are not zero."""
    for s in range(bb.S):
        for b, (W, _, n) in enumerate(bb.window_plans()):
            ref, own, _, fine = picks[s, b]
            assert not ref['power_only'].any(), (s, b)
            assert np.all(ref['index'] >= 0)
            for k in range(n):
                g = int(ref['index'][k])
                rest = np.delete(ref['F'][k] + ref['tol_fstat'][k], g)
                assert ref['F'][k, g] - ref['tol_fstat'][k, g] > rest.max(), (s, b, k)
            assert np.all(np.abs(own) < W - 1), (s, b)
            assert np.all(np.abs(fine['D']) >= 2.0 ** 20 * fine['E']), (s, b)
            assert np.count_nonzero(fine['frac']) >= fine['frac'].size // 2, (s, b)
