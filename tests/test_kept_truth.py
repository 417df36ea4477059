"""The kept-element truth of tests/kept_truth.py on weight tables designed by hand, and the demonstration that motivates the
feature: FAST-LTS names the mistimed element, and the beam and the Capon spectrum formed without it
recover what the full array loses.  CPU only."""
import numpy as np
import pytest

import beam_truth
import capon_truth as ct
import kept_truth as kt
from narrow_band_least_squares_amd import planner, synthetic


def _weights(N, zero_pairs):
    w = np.ones(N * (N - 1) // 2, dtype=np.uint8)
    for a, b in zero_pairs:
        w[kt.pair_index(N, min(a, b), max(a, b))] = 0
    return w


def _all_pairs_of(N, m):
    return [(m, o) for o in range(N) if o != m]


def test_pair_index_is_the_lexicographic_list():
    for N in range(3, 33):
        assert [kt.pair_index(N, a, b) for a, b in kt.pair_list(N)] == list(range(N * (N - 1) // 2))


@pytest.mark.parametrize('N', list(range(3, 33)))
def test_one_element_first_middle_last(N):
    """Every pair of one element at weight 0: that element and no other at q = N - 1; at q = 1 every element, because
    each of the others has lost one pair — fewer than 3 remain and the kept set falls back to the whole array."""
    for m in (0, N // 2, N - 1):
        w = _weights(N, _all_pairs_of(N, m))
        assert list(kt.zero_counts(w, N)) == [N - 1 if e == m else 1 for e in range(N)]
        mask, kept, M = kt.rule(w, N, N - 1)
        if N >= 4:
            assert mask == 1 << m and list(kept) == [e for e in range(N) if e != m] and M == N - 1
        else:                                                     # N = 3: two would remain — the fallback
            assert mask == 1 << m and list(kept) == [0, 1, 2] and M == 3
        mask, kept, M = kt.rule(w, N, 1)
        assert mask == (1 << N) - 1 and list(kept) == list(range(N)) and M == N
        if N >= 5:
            # q = N - 2: still that element alone (the others have lost one pair, and N - 2 >= 3)
            mask, kept, M = kt.rule(w, N, N - 2)
            assert mask == 1 << m and M == N - 1


@pytest.mark.parametrize('N', [5, 6, 8, 9, 16, 32])
def test_two_elements(N):
    """Both elements' pairs at weight 0: each has lost N - 1, every other element 2."""
    a, b = 1, N - 1
    w = _weights(N, _all_pairs_of(N, a) + _all_pairs_of(N, b))
    c = kt.zero_counts(w, N)
    assert c[a] == N - 1 and c[b] == N - 1 and all(c[e] == 2 for e in range(N) if e not in (a, b))
    mask, kept, M = kt.rule(w, N, N - 1)
    assert mask == (1 << a) | (1 << b)
    if N - 2 >= 3:
        assert list(kept) == [e for e in range(N) if e not in (a, b)] and M == N - 2
    else:
        assert list(kept) == list(range(N)) and M == N
    # q = N - 2 names the same two as long as 2 < N - 2
    if N >= 5 and N - 2 > 2:
        assert kt.rule(w, N, N - 2)[0] == mask
    # q = 2 names everyone: the fallback
    mask, kept, M = kt.rule(w, N, 2)
    assert mask == (1 << N) - 1 and list(kept) == list(range(N)) and M == N


def test_partial_loss_and_thresholds():
    """N = 8, element 3 has lost 5 of its 7 pairs: named at q <= 5, not above; an element that lost one pair with it is
    named at q = 1 only."""
    N = 8
    w = _weights(N, [(3, o) for o in (0, 1, 2, 4, 5)])
    assert kt.rule(w, N, 7)[0] == 0 and kt.rule(w, N, 6)[0] == 0 and kt.rule(w, N, 6)[2] == 8
    assert kt.rule(w, N, 5)[0] == 1 << 3 and kt.rule(w, N, 2)[0] == 1 << 3
    mask, kept, M = kt.rule(w, N, 1)
    assert mask == sum(1 << e for e in (0, 1, 2, 3, 4, 5)) and M == 8 and list(kept) == list(range(8))      # 2 would remain
    # nothing lost: nothing named at any q
    for q in range(1, N):
        mask, kept, M = kt.rule(np.ones(28, dtype=np.uint8), N, q)
        assert mask == 0 and list(kept) == list(range(N)) and M == N


def test_fallback_keeps_the_mask():
    """N = 4, elements 0 and 3 dropped: two would remain, so the kept set is the whole array and the mask still says 9."""
    N = 4
    w = _weights(N, _all_pairs_of(N, 0) + _all_pairs_of(N, 3))
    mask, kept, M = kt.rule(w, N, 3)
    assert mask == 0b1001 and M == 4 and list(kept) == [0, 1, 2, 3]
    assert list(kt.kept_of_mask(mask, N)) == [0, 1, 2, 3] and list(kt.kept_of_mask(0b0001, N)) == [1, 2, 3]
    m2, c2 = kt.rule_table(np.stack([w, np.ones(6, dtype=np.uint8)]).reshape(1, 2, 6), N, 3)
    assert m2.dtype == np.uint32 and c2.dtype == np.int32 and m2.tolist() == [[9, 0]] and c2.tolist() == [[4, 4]]


def test_kept_coarray_rows():
    N = 6
    rij = synthetic.array_geometry(N, 1.0)
    xij = planner.co_array(rij)[0]
    kept = np.array([1, 2, 4, 5])
    rows = kt.kept_coarray(xij, N, kept)
    sub = planner.co_array(rij[:, kept])[0]
    np.testing.assert_array_equal(rows, sub[:3])                   # the pairs (0, i) of the sub-array's own co-array


# ---- the demonstration ----

FS, W, HOP, NWIN, BAD = 20.0, 2400, 1200, 20, 7
NPTS = W + (NWIN - 1) * HOP + 1
BAZ, VEL = 225.0, 0.34


def _band(data):
    from scipy import signal
    return signal.sosfiltfilt(signal.butter(2, [0.45, 0.55], 'bandpass', fs=FS, output='sos'), data, axis=1)


def _lts(oracle, data, rij, alpha):
    """The oracle's full-lag picks and FAST-LTS of the 20 windows -> (z (2, nwin), weights (P, nwin))."""
    xij, idx = oracle.co_array(rij)
    _, _, intervals = oracle.window_plan(data.shape[1], FS, W / FS, 1.0 - HOP / W)
    assert len(intervals) == NWIN
    tau, _, _ = oracle.correlate_windows(np.ascontiguousarray(data.T), W, intervals, idx, FS)
    zraw = oracle.fast_lts(tau, xij, alpha)
    z, weights, _ = oracle.lts_post_process(tau, xij, zraw, alpha)
    return z, weights


@pytest.fixture(scope='module')
def demo(oracle):
    rij = synthetic.array_geometry(8, 1.0)
    bad = _band(synthetic.plane_wave(rij, NPTS, FS, 0.1, 5.0, snr_db=10.0, timing_error_s=0.25, bad_element=BAD))
    clean = _band(synthetic.plane_wave(rij, NPTS, FS, 0.1, 5.0, snr_db=10.0))
    return dict(rij=rij, bad=bad, clean=clean, lts_bad=_lts(oracle, bad, rij, 0.5), lts_clean=_lts(oracle, clean, rij, 0.5))


def test_lts_names_the_mistimed_element(demo):
    N = 8
    z, weights = demo['lts_bad']
    named = [kt.rule(weights[:, w], N, N - 1)[0] for w in range(NWIN)]
    exactly = sum(m == 1 << BAD for m in named)
    others = max(int(np.delete(kt.zero_counts(weights[:, w], N), BAD).max()) for w in range(NWIN))
    vel = 1.0 / np.hypot(z[0], z[1])
    baz = np.mod(np.degrees(np.arctan2(z[0], z[1])), 360.0)
    right = int(np.sum((np.abs((baz - BAZ + 180.0) % 360.0 - 180.0) <= 5.0) & (np.abs(vel - VEL) <= 0.1 * VEL)))
    print('mistimed element %d: named exactly in %d / %d windows, LTS within 5 deg and 10 %% in %d / %d, the most pairs '
          'another element lost: %d of %d' % (BAD, exactly, NWIN, right, NWIN, others, N - 1))
    assert exactly >= 18
    zc, wc = demo['lts_clean']
    named_clean = [kt.rule(wc[:, w], N, N - 1)[0] for w in range(NWIN)]
    print('clean trace: elements named in %d / %d windows' % (sum(m != 0 for m in named_clean), NWIN))
    assert all(m == 0 for m in named_clean)


def test_beam_f_recovers_on_the_kept_elements(demo):
    N = 8
    rij, data = demo['rij'], demo['bad']
    z, weights = demo['lts_bad']
    xij = planner.co_array(rij)[0]
    zt = np.ascontiguousarray(z.T)
    full = beam_truth.beam_reference(data, FS, xij, zt, W, HOP, NWIN)['fstat']
    kept = np.array([kt.beam_reference(data, FS, xij, zt, W, HOP, w, kt.rule(weights[:, w], N, N - 1)[1])['fstat'][0]
                     for w in range(NWIN)])
    print('median beam F at the LTS slowness: full array %.1f, kept elements %.1f (%.2f x)'
          % (np.median(full), np.median(kept), np.median(kept) / np.median(full)))
    assert np.median(kept) >= 2.0 * np.median(full)


def test_capon_power_recovers_on_the_kept_elements(demo):
    N = 8
    rij, data = demo['rij'], demo['bad']
    _, weights = demo['lts_bad']
    xij = planner.co_array(rij)[0]
    grid = planner.slowness_grid(4.0, 41)
    f = planner.capon_frequencies([(0.45, 0.55)])
    Ls, Hs = planner.capon_snapshots(xij, grid, FS, f, [W])
    coef, steer = ct.tables(xij, grid, FS, f[0], Ls[0], N)
    R, _ = ct.csdm_reference(data, coef, W, HOP, NWIN, int(Hs[0]))
    s_true = np.array([np.sin(np.radians(BAZ)), np.cos(np.radians(BAZ))]) / VEL      # (the slowness points to the source)
    nearest = int(np.argmin(np.hypot(grid[:, 0] - s_true[0], grid[:, 1] - s_true[1])))
    pf, pk, right_f, right_k = [], [], 0, 0
    for w in range(NWIN):
        Rw = R[w].astype(np.complex128)
        full = ct.spectra_reference(Rw, steer, 0.01)
        kept = kt.spectra_reference(Rw, steer, 0.01, kt.rule(weights[:, w], N, N - 1)[1])
        pf.append(float(full['PC'][full['index_C']]))
        pk.append(float(kept['PC'][kept['index_C']]))
        near = lambda g: np.hypot(*(grid[g] - grid[nearest])) <= 1.5 * (8.0 / 40)
        right_f += bool(near(full['index_C']))
        right_k += bool(near(kept['index_C']))
    ratio = np.median(pf) / np.median(pk)
    print('median Capon peak power: full array %.4g, kept elements %.4g (full / kept = 1 / %.2f); arg-max within a grid '
          'step and a half of the truth: full %d / %d, kept %d / %d' % (np.median(pf), np.median(pk), 1.0 / ratio, right_f,
                                                                      NWIN, right_k, NWIN))
    assert ratio <= 1.0 / 3.0
