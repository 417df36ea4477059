"""The closure truth of tests/closure_truth.py on tables worked out by hand, and the count that motivates the feature
(DESIGN.md section 17): closure tells a mistimed element, which it cannot see, from a noisy one, which it names."""
import numpy as np
import pytest

import closure_truth as ct
from narrow_band_least_squares_amd import synthetic


def _plane_table(N, delays):
    """lag_ij = d_j - d_i in list order."""
    return np.array([delays[j] - delays[i] for i in range(N - 1) for j in range(i + 1, N)], dtype=np.int64)


@pytest.mark.parametrize('N', [3, 4, 8, 9])
def test_a_plane_wave_table_closes(N):
    rng = np.random.default_rng(N)
    lag = _plane_table(N, rng.integers(-40, 40, N))
    Q, cmax, E = ct.closure_int(lag, N)
    assert Q == 0 and cmax == 0 and E == [0] * N
    cons, cm, el, _ = ct.outputs_int(lag, N, 20.0)
    assert cons == 0.0 and cm == 0.0 and not el.any()
    # clock offsets are delays too: they leave the closure at zero, and so does any curvature of the wavefront
    ref = ct.outputs_refined(lag, np.zeros(len(lag)), N, 20.0, 64)
    assert ref['cons'] == 0.0 and ref['cmax'] == 0.0 and not ref['el'].any()


@pytest.mark.parametrize('N,a,b,g', [(4, 0, 3, 5), (8, 2, 5, -7), (9, 0, 1, 1)])
def test_one_pair_off_by_g(N, a, b, g):
    """Pair (a, b) off by g: the N - 2 triplets that hold a and b miss by |g|, no other one.  Q = (N - 2) g^2,
    E_a = E_b = (N - 2) g^2, every other element sits in exactly one of them: E_m = g^2."""
    rng = np.random.default_rng(10 + N)
    lag = _plane_table(N, rng.integers(-40, 40, N))
    lag[ct.pair_index(N)[(a, b)]] += g
    Q, cmax, E = ct.closure_int(lag, N)
    assert Q == (N - 2) * g * g and cmax == abs(g)
    assert E == [(N - 2) * g * g if m in (a, b) else g * g for m in range(N)]
    fs = 20.0
    T, Tm = ct.counts(N)
    cons, cm, el, _ = ct.outputs_int(lag, N, fs)
    assert cons == np.sqrt((N - 2) * g * g / T) / fs and cm == abs(g) / fs
    assert el[a] == np.sqrt((N - 2) * g * g / Tm) / fs
    # sum_m E_m = 3 Q: every triplet holds three elements
    assert sum(E) == 3 * Q
    # the refined form with zero fractions is the same numbers
    ref = ct.outputs_refined(lag, np.zeros(len(lag)), N, fs, 64)
    assert abs(ref['cons'] - cons) <= ref['tol_cons'] and abs(ref['cmax'] - cm) <= ref['tol_cmax']
    assert np.all(np.abs(ref['el'] - el) <= ref['tol_el'])


def test_three_elements():
    """One triplet: T = T_m = 1, all three outputs are |l_01 + l_12 - l_02| / fs."""
    lag = np.array([4, 1, -6])                                     # (0,1), (0,2), (1,2): c = (4 - 6) - 1 = -3
    assert ct.counts(3) == (1, 1)
    assert ct.closure_int(lag, 3) == (9, 3, [9, 9, 9])
    cons, cm, el, _ = ct.outputs_int(lag, 3, 20.0)
    assert cons == cm == 3 / 20.0 and list(el) == [3 / 20.0] * 3
    ref = ct.outputs_refined(lag, np.array([0.25, -0.5, 0.125]), 3, 20.0, 64)      # c = (4.25 - 5.875) - 0.5 = -2.125
    assert ref['cons'] == ref['cmax'] and abs(ref['cons'] - 2.125 / 20.0) < 1e-16 and 0 < ref['tol_cons'] < 1e-13


def test_the_refined_bound_is_the_stated_one():
    rng = np.random.default_rng(5)
    N, W, fs = 4, 257, 20.0
    lag, frac = rng.integers(-200, 200, 6), rng.uniform(-0.5, 0.5, 6)
    ref = ct.outputs_refined(lag, frac, N, fs, W)
    t = lag + frac
    idx = ct.pair_index(N)
    c = np.array([(t[idx[(i, j)]] + t[idx[(j, k)]]) - t[idx[(i, k)]] for i, j, k in ct.triplets(N)])
    delta, T = 5 * W * 2.0 ** -53, 4
    Q = float(np.sum(c * c))
    EQ = float(np.sum(2 * np.abs(c) * delta + delta * delta) + 2 * T * 2.0 ** -53 * Q)
    tol = (np.sqrt((Q + EQ) / T) - np.sqrt(max(Q - EQ, 0.0) / T)) / fs + 4 * 2.0 ** -52 * np.sqrt(Q / T) / fs
    assert ref['tol_cons'] == pytest.approx(tol, rel=1e-6)
    assert ref['tol_cmax'] == pytest.approx(delta / fs + 4 * 2.0 ** -52 * ref['cmax'], rel=1e-9)


def _medians(data, rij, fs, W, hop, nwin):
    """Per window NumPy full-lag picks -> medians over the windows of (consistency, element closure (N,), per element the
    rms OLS residual over the pairs that hold it (N,)), seconds."""
    N = data.shape[0]
    pairs = [(i, j) for i in range(N - 1) for j in range(i + 1, N)]
    xij = np.array([rij[:, i] - rij[:, j] for i, j in pairs])
    cons, el, res = [], [], []
    for w in range(nwin):
        lag = ct.numpy_lags(data[:, w * hop:w * hop + W])
        c, _, e, _ = ct.outputs_int(lag, N, fs)
        tau = lag / fs
        z = np.linalg.lstsq(xij, tau, rcond=None)[0]
        r = tau - xij @ z
        cons.append(c)
        el.append(e)
        res.append([np.sqrt(np.mean([r[k] ** 2 for k, p in enumerate(pairs) if m in p])) for m in range(N)])
    return np.median(cons), np.median(el, axis=0), np.median(res, axis=0)


def test_what_closure_tells_apart():
    """8 elements in 0.3 km, a 0.5 - 4 Hz wave at 12 dB and 40 Hz, 600-sample windows hopping by 300, the first 20.  Element
    3 mistimed by 0.25 s: its closure stays within 10 % of the clean value while its plane-wave residual rises at least
    tenfold (measured: equal to 3 decimals, 18 x).  Element 3 replaced by white noise: its closure is the largest of the
    eight, at least 1.5 x the second largest (measured: 1.79 x)."""
    fs, npts, W, hop, nwin = 40.0, 7200, 600, 300, 20
    rij = synthetic.array_geometry(8, 0.3)
    clean = synthetic.plane_wave(rij, npts, fs, 0.5, 4.0, snr_db=12.0)
    mistimed = synthetic.plane_wave(rij, npts, fs, 0.5, 4.0, snr_db=12.0, timing_error_s=0.25, bad_element=3)
    replaced = clean.copy()
    replaced[3] = np.random.default_rng(7).standard_normal(npts)
    c0, el0, r0 = _medians(clean, rij, fs, W, hop, nwin)
    c1, el1, r1 = _medians(mistimed, rij, fs, W, hop, nwin)
    c2, el2, r2 = _medians(replaced, rij, fs, W, hop, nwin)
    print('clean     consistency %.3f  element 3 %.3f / largest other %.3f  residual %.3f' % (c0, el0[3], np.delete(el0, 3).max(), r0[3]))
    print('mistimed  consistency %.3f  element 3 %.3f / largest other %.3f  residual %.3f' % (c1, el1[3], np.delete(el1, 3).max(), r1[3]))
    print('replaced  consistency %.3f  element 3 %.3f / largest other %.3f  residual %.3f' % (c2, el2[3], np.delete(el2, 3).max(), r2[3]))
    assert abs(el1[3] - el0[3]) <= 0.1 * el0[3]
    assert r1[3] >= 10.0 * r0[3]
    others = np.sort(np.delete(el2, 3))
    assert el2[3] > others[-1] and el2[3] >= 1.5 * others[-1]
