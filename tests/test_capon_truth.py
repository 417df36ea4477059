"""The long-double reference of the Capon / Bartlett spectra (tests/capon_truth.py) against ``numpy.linalg`` in complex128,
its sign convention against the delay-and-sum reference of tests/grid_truth.py, and the two-source demonstration of
DESIGN.md section 18 with the default snapshot rule ``planner.capon_snapshots``.  CPU only."""
import numpy as np
import pytest

import capon_truth as ct
import grid_truth as gt
from narrow_band_least_squares_amd import planner, synthetic

FS = 20.0


def _centred(N):
    rij = synthetic.array_geometry(N, 1.0)
    return rij - rij.mean(axis=1, keepdims=True)


@pytest.mark.parametrize('N,delta', [(3, 0.01), (8, 0.01), (8, 1e-6), (32, 0.01)])
def test_agrees_with_numpy_linalg(N, delta):
    rng = np.random.default_rng(5 + N)
    rij = _centred(N)
    xij = planner.co_array(rij)[0]
    grid = planner.slowness_grid(3.0, 5)
    W, Ls, Hs, f = 200, 40, 20, 1.0
    data = rng.standard_normal((N, W + 50))
    coef, steer = ct.tables(xij, grid, FS, f, Ls, N)
    R, tol = ct.csdm_reference(data, coef, W, 25, 2, Hs)
    K = ct.snapshot_count(W, Ls, Hs)
    for w in range(2):
        X = np.array([[np.dot(coef, data[i, w * 25 + k * Hs:w * 25 + k * Hs + Ls]) for i in range(N)] for k in range(K)])
        Rn = X.T @ np.conj(X) / K
        assert np.all(np.abs(Rn - R[w].astype(np.complex128)) <= 2 * tol[w] + 1e-300)
        ref = ct.spectra_reference(Rn, steer, delta)
        assert ref['chol_ok'] and not ref['degenerate']
        t = np.trace(Rn).real
        Rp = Rn + delta * t / N * np.eye(N)
        assert ref['kappa'] <= (N + delta) / delta * (1 + 1e-9)
        PB = np.einsum('gi,ij,gj->g', np.conj(steer), Rn, steer).real / N ** 2
        PC = 1.0 / np.einsum('gi,gi->g', np.conj(steer), np.linalg.solve(Rp, steer.T).T).real
        assert np.all(np.abs(PB - ref['PB'].astype(np.float64)) <= ref['tolB'])
        if ref['kappa'] * N * ct.U < 1e-6:
            assert np.all(np.abs(PC - ref['PC'].astype(np.float64)) <= 2 * ref['tolC'])
        assert ref['index_B'] == int(np.argmax(PB)) or abs(PB[ref['index_B']] - PB.max()) <= 2 * ref['tolB'][0]


def test_degenerate_matrices():
    steer = np.ones((3, 4), dtype=np.complex128)
    assert ct.spectra_reference(np.zeros((4, 4), dtype=np.complex128), steer, 0.01)['degenerate']
    R = np.eye(4, dtype=np.complex128)
    R[1, 2] = np.nan
    assert ct.spectra_reference(R, steer, 0.01)['degenerate']
    R = np.diag([1.0, 0.0, 1.0, 1.0]).astype(np.complex128)
    ref = ct.spectra_reference(R, steer, 0.0)
    assert not ref['degenerate'] and not ref['chol_ok'] and ref['index_C'] == -1 and ref['index_B'] == 0
    assert ct.spectra_reference(R, steer, 0.01)['chol_ok']
    assert ct.argmax_total([np.nan, 2.0, 2.0, 1.0]) == 1 and ct.argmax_total([np.nan]) == -1


def test_single_wave_sign_convention():
    """One wave: both maxima at the grid point nearest its slowness, the point the delay-and-sum reference finds."""
    N, W, npts = 8, 2400, 2400 + 1200 + 1
    rij = _centred(N)
    xij = planner.co_array(rij)[0]
    grid = planner.slowness_grid(4.0, 21)
    s_true = np.array([2.4, 1.6])                          # a grid point: 0.347 km/s from 56.3 degrees
    data = synthetic.plane_wave(rij, npts, FS, 0.45, 0.55, baz_deg=float(np.degrees(np.arctan2(s_true[0], s_true[1]))),
                                vel_kms=float(1.0 / np.hypot(*s_true)), snr_db=10.0, seed=77)
    f = planner.capon_frequencies([(0.45, 0.55)])
    Ls, Hs = planner.capon_snapshots(xij, grid, FS, f, [W])
    coef, steer = ct.tables(xij, grid, FS, f[0], Ls[0], N)
    R, _ = ct.csdm_reference(data, coef, W, 1200, 2, int(Hs[0]))
    nearest = int(np.argmin(np.hypot(grid[:, 0] - s_true[0], grid[:, 1] - s_true[1])))
    dref = gt.grid_reference(data, FS, xij, grid, W, 1200, 2)
    for w in range(2):
        ref = ct.spectra_reference(R[w].astype(np.complex128), steer, 0.01)
        assert ref['index_C'] == nearest and ref['index_B'] == nearest and int(dref['index'][w]) == nearest


BAZ = (50.0, 70.0)


def two_source_case(n=81):
    """N = 8, 0.5 Hz, two waves of equal power 20 degrees apart at 10 dB, 19 windows of 2400 samples hopping by 1200."""
    N, W, inc = 8, 2400, 1200
    npts = W + 18 * inc + 1
    rij = _centred(N)
    data = synthetic.plane_waves(rij, npts, FS, 0.45, 0.55, [(BAZ[0], 0.34, 1.0), (BAZ[1], 0.34, 1.0)], snr_db=10.0, seed=4242)
    ax = np.linspace(-4.0, 4.0, n)
    g0, g1 = np.meshgrid(ax, ax, indexing='ij')
    grid = np.ascontiguousarray(np.stack([g0.ravel(), g1.ravel()], axis=1))
    return rij, data, grid, (n, n), W, inc


def count_both(maps, grid, shape):
    return sum(bool(ct.both_found(m, grid, shape, BAZ)) for m in maps)


def test_two_sources():
    rij, data, grid, shape, W, inc = two_source_case()
    N = rij.shape[1]
    xij = planner.co_array(rij)[0]
    f = planner.capon_frequencies([(0.45, 0.55)])
    Ls, Hs = planner.capon_snapshots(xij, grid, FS, f, [W])
    coef, steer = ct.tables(xij, grid, FS, f[0], Ls[0], N)
    R, _ = ct.csdm_reference(data, coef, W, inc, 19, int(Hs[0]))
    refs = [ct.spectra_reference(R[w].astype(np.complex128), steer, 0.01) for w in range(19)]
    kmax = max(r['kappa'] for r in refs)
    assert kmax <= (N + 0.01) / 0.01
    capon = count_both([r['PC'] for r in refs], grid, shape)
    bartlett = count_both([r['PB'] for r in refs], grid, shape)
    print('two sources, Ls = %d, Hs = %d: Capon %d / 19, Bartlett %d / 19, kappa <= %.0f' % (Ls[0], Hs[0], capon, bartlett, kmax))
    assert capon >= 15
    assert bartlett < capon
