"""The truth of the eigenvalues and the MUSIC spectrum (tests/music_truth.py) against LAPACK and mpmath,
the condition on the inputs of the GPU tests, and the demonstration of section 25.4.  CPU only."""
import functools

import numpy as np
import pytest

import capon_truth as ct
import music_cases as mc
import music_truth as mt
import test_clean_truth as tct
from narrow_band_least_squares_amd import planner, synthetic

FS = tct.FS


def _matrix(N, K, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((K, N)) + 1j * rng.standard_normal((K, N))
    return np.einsum('ki,kj->ij', X, np.conj(X)) / K


@pytest.mark.parametrize('N,K', [(3, 1), (3, 7), (8, 3), (8, 13), (32, 4), (32, 40)])
def test_truth_agrees_with_lapack(N, K):
    """Full rank and rank-deficient (K < N): the eigenvalues within LAPACK's own 4 N u ||R||, R E = E L and E^H E = I far
    below it, the order descending."""
    R = _matrix(N, K, 100 * N + K)
    lam, E, sweeps = mt.jacobi(R)
    ref = np.linalg.eigvalsh(R)[::-1]
    nrm = np.linalg.norm(R)
    assert np.all(np.diff(lam.astype(np.float64)) <= 0)
    assert np.max(np.abs(lam.astype(np.float64) - ref)) <= 4 * N * 2.0 ** -52 * nrm
    Rl = R.astype(mt.CLD)
    assert float(np.abs(Rl @ E - E * lam[None, :]).max()) <= 2.0 ** -55 * nrm
    assert float(np.abs(np.conj(E.T) @ E - np.eye(N)).max()) <= 2.0 ** -55
    assert np.sum(lam.astype(np.float64) > 1e-12 * nrm) == min(N, K)
    print('N=%d K=%d: the truth took %d sweeps' % (N, K, sweeps))


@pytest.mark.parametrize('N,K', [(3, 7), (8, 3), (32, 13)])
def test_truth_agrees_with_mpmath(N, K):
    mp = pytest.importorskip('mpmath')
    R = _matrix(N, K, 200 * N + K)
    lam = mt.jacobi(R)[0]
    with mp.workdps(40):
        ev = mp.eighe(mp.matrix(R.tolist()), eigvals_only=True)
        ref = sorted((mp.mpf(v) for v in ev), reverse=True)
        err = max(abs(mp.mpf(float(l)) + mp.mpf(float(l - mt.LD(float(l)))) - r) for l, r in zip(lam, ref))
    assert float(err) <= 2.0 ** -58 * np.linalg.norm(R)


def test_order_is_total_and_the_floor_rule():
    lam, E, sweeps = mt.jacobi(np.diag([2.0, 5.0, 2.0, 0.0]).astype(complex))
    assert sweeps == 0 and list(lam) == [5.0, 2.0, 2.0, 0.0]
    assert np.array_equal(np.abs(E).astype(np.float64), np.eye(4)[:, [1, 0, 2, 3]])       # equal values: the lower column first
    assert mt.sources_by_floor([5.0, 2.0, 2.0, 0.0], 0.05) == 3
    assert mt.sources_by_floor([5.0, 0.2, 0.1, 0.0], 0.05) == 1
    assert mt.sources_by_floor([5.0, 5.0, 5.0, 5.0], 0.05) == 3                             # clamped to N - 1
    assert mt.sources_by_floor([5.0, 0.25, 0.1], 0.05) == 2                                 # >= : the floor itself counts
    assert mt.argmin_total(np.array([3.0, 1.0, np.nan, 1.0])) == 1 and mt.argmin_total(np.array([np.nan])) == -1


def test_one_wave_at_a_grid_point_has_a_pole_there():
    rij = mc.geometry(8)
    steer = ct.tables(planner.co_array(rij)[0], mc.grid(129), FS, mc.FREQ, 16, 8)[1]
    R = 3.5 * np.outer(steer[17], np.conj(steer[17])) + 1e-3 * np.eye(8)
    m = mt.music(R, steer, 1)
    assert m['index'] == 17 and float(m['D'][17]) <= 2.0 ** -100 and m['M'] == 1
    assert abs(float(m['lam'][0]) - (28.0 + 1e-3)) <= 1e-12 and mt.music(R, steer, 0)['M'] == 1
    assert float(np.abs(m['Pn'] @ steer[17].astype(mt.CLD)).max()) <= 2.0 ** -50           # (R is rank one up to its float64 rounding)


@functools.lru_cache(maxsize=None)
def set_matrices(N, G, W, Ls, Hs, S):
    data, rij = mc.traces(N, W, S)
    coef, steer = ct.tables(planner.co_array(rij)[0], mc.grid(G), FS, mc.FREQ, Ls, N)
    inc, nwin = mc.windows(W, data.shape[1])
    R = ct.csdm_reference(data, coef, W, inc, nwin, Hs)[0]
    return R.astype(np.complex128), steer


@pytest.mark.parametrize('N,G,shape,S', mc.sets())
def test_condition_on_the_inputs(N, G, shape, S):
    """Every input set of the GPU tests: where a gap can exist at all (``music_cases.has_gap``) the truth has gap >= 1e-3
    lambda_1 behind M = S, and behind the M of the rho rule in every set."""
    R, steer = set_matrices(N, G, *shape, S)
    assert 2 <= len(R) <= 4
    for w in range(len(R)):
        lam = mt.jacobi(R[w])[0].astype(np.float64)
        if mc.has_gap(N, *shape, S):
            assert lam[S - 1] - lam[S] >= mc.GAP * lam[0], 'a condition on the inputs: change the seed'
        M = mt.sources_by_floor(lam, mc.EIG_FLOOR)
        assert lam[M - 1] - lam[M] >= mc.GAP * lam[0], 'a condition on the inputs: change the seed'


# ---- the demonstration: the cases, the grid and the criterion of section 24.4 ----
# Windows of 19 in which the S strongest local maxima of the map are the S sources, as measured on this truth's inputs with
# numpy.linalg.eigh: Capon peaks | MUSIC with M = S | MUSIC with M by lambda >= 0.05 lambda_1 | MUSIC with M = S + 1.
# The classical MDL count is left out on purpose: the overlapping Hann snapshots are correlated, and MDL says 2 for a single
# wave in 19 of 19 windows.
MEASURED = [dict(capon=18, music=19, rule=19, over=18),
            dict(capon=15, music=19, rule=17, over=7),
            dict(capon=11, music=19, rule=18, over=10),
            dict(capon=14, music=18, rule=18, over=18)]


def music_map(R, steer, M):
    """1 / D of the noise subspace behind the M largest eigenvalues (numpy.linalg.eigh), float64."""
    lam, E = np.linalg.eigh(R)
    En = E[:, ::-1][:, M:]
    with np.errstate(divide='ignore'):
        return R.shape[0] / (np.abs(steer @ np.conj(En)) ** 2).sum(axis=1)


@functools.lru_cache(maxsize=None)
def demo_matrices(row, sources=None):
    rij, data, src, W, inc = tct.demo_case(row)
    if sources is not None:
        src = list(sources)
        data = synthetic.plane_waves(rij, W + 18 * inc + 1, FS, 0.45, 0.55, src, snr_db=10.0, seed=4242)
    grid, cells = tct.demo_grid()
    xij = planner.co_array(rij)[0]
    Ls, Hs = planner.capon_snapshots(xij, grid, FS, [0.5], [W])
    coef, steer = ct.tables(xij, grid, FS, 0.5, Ls[0], 8)
    R = ct.csdm_reference(data, coef, W, inc, 19, int(Hs[0]))[0]
    return R.astype(np.complex128), steer, grid, cells, src


@pytest.mark.parametrize('row', range(4))
def test_demonstration(row):
    R, steer, grid, cells, sources = demo_matrices(row)
    S = len(sources)
    lam = [np.linalg.eigvalsh(R[w])[::-1] for w in range(19)]
    counts = {}
    counts['music'] = tct.peak_lists_find([music_map(R[w], steer, S) for w in range(19)], grid, cells, sources)
    counts['rule'] = tct.peak_lists_find([music_map(R[w], steer, mt.sources_by_floor(lam[w], 0.05)) for w in range(19)], grid, cells, sources)
    counts['over'] = tct.peak_lists_find([music_map(R[w], steer, S + 1) for w in range(19)], grid, cells, sources)
    counts['capon'] = tct.peak_lists_find([ct.spectra_reference(R[w], steer, 0.01)['PC'] for w in range(19)], grid, cells, sources)
    gap = min((l[S - 1] - l[S]) / l[0] for l in lam)
    print('demonstration row %d: Capon peaks %d, MUSIC M = S %d, by the floor %d, M = S + 1 %d of 19; min gap / lambda_1 %.3f'
          % (row + 1, counts['capon'], counts['music'], counts['rule'], counts['over'], gap))
    assert counts['music'] >= 17
    assert counts['rule'] >= 15
    if row >= 1:
        assert counts['music'] > counts['capon']


def test_one_wave_is_one_source_by_the_floor():
    R = demo_matrices(0, ((50.0, 0.34, 1.0),))[0]
    assert [mt.sources_by_floor(np.linalg.eigvalsh(R[w])[::-1], 0.05) for w in range(19)] == [1] * 19
