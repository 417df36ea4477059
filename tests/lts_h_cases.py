"""Every subset size h that a FAST-LTS kernel can be given, and the inputs on which a wrong h shows.  CPU only: nothing
here loads the GPU library (``planner`` and ``synthetic`` are plain NumPy).

**h and ALPHA.**  The kernels take ``h = planner.lts_h(P, alpha) = floor(2 n2 - P + 2 (P - n2) alpha)``, n2 = (P + 3) // 2, as
a run-time value: any integer from ``h(0.5) = n2`` to ``P - 1``.  ``alpha_of(P, h)`` is the midpoint of the ALPHA interval
that maps to h, half a step of ``1 / (2 (P - n2))`` (1e-3 at 496 pairs) away from both edges, so no rounding of the
product moves it to a neighbour.

**H_LIST.**  4 ... 9 elements: every h (2, 4, 6, 9, 13, 17 values; 4 ... 8 run the register-resident kernel, whose pruned
instance exists for h(0.5) alone, 9 the bucket kernel).  12, 16, 23, 24, 32 (bucket kernel; 23 is the last size with u8
counters and subset merging, 24 the first with u16 counters and none): h(0.5), h(0.5) + 1, h(0.75), the first h whose
ALPHA is above 0.875 (the second branch of the small-sample factor ``_cnp2``), P - 2 and P - 1.

**Pulse tables.**  ``solve_truth.tables(N)`` (the ``short`` set from 16 elements on).  b mistimed elements leave
C(N - b, 2) pairs on one plane, so the ``one_bad`` / ``two_bad`` rows are exact fits up to h = C(N - b, 2) and cannot be
from there on (``exact_fit_expected``): sweeping h walks them across that edge (8 elements: 21 and 15).

**Noisy windows.**  ``noisy_trace(N)``: 64-sample windows, hop 64, of ``synthetic.plane_wave`` on
``solve_truth.grid_geometry(N)`` — a band-limited plane wave in white noise at low SNR with the last element mistimed.
The lags the correlator picks from them do not close, and a part of them are gross outliers (a noise peak won): the
h-subset, the raw scale and the first weights then depend on h exactly, which is what tests/test_lts_h_cases.py asserts
(by the oracle alone) before tests/test_gpu_lts_h.py relies on it."""
import functools

import numpy as np

import solve_truth as st
from narrow_band_least_squares_amd import planner, synthetic

SMALL_N = (4, 5, 6, 7, 8, 9)
LARGE_N = (12, 16, 23, 24, 32)
ALL_N = SMALL_N + LARGE_N

# the noisy trace: a 0.5 - 4 Hz wave at 2.5 km/s from 225 degrees (at most 34 samples across the 4.2 km of the grid)
NOISY_BAND = (0.5, 4.0)
NOISY_BAZ = 225.0
NOISY_VEL = 2.5
NOISY_SNR_DB = -6.0
NOISY_TIMING_S = 0.35                           # 7 samples on the last element
NOISY_SEED = 4100                               # element count N draws with NOISY_SEED + N ...
# ... unless that trace misses a condition of tests/test_lts_h_cases.py: then a later seed (in steps of 100) that meets
# them all, found on the CPU with the oracle alone.  Two conditions decide: the discrimination minimum at every h and
# neighbour (the large arrays have 8 or 3 windows for it), and no window, at any h, whose confidence ellipse passes the
# origin so closely that 20 000 samples of it are too few for the checker's 1e-4 (``sampler_gap``)
NOISY_SEEDS = {6: 4206, 7: 4907, 8: 5208, 9: 4709, 12: 5012, 16: 4616, 23: 5923, 24: 6624, 32: 6232}
# (N, h, searched h) whose mutant changes none of that trace's windows: with 3 windows, no seed of 80 tried per size
# serves all ten neighbours at once.  tests/test_lts_h_cases.py prints and pins the list
NOT_DISCRIMINATED = ((23, 128, 129), (24, 139, 140), (32, 434, 435))


def npairs(N):
    return N * (N - 1) // 2


def alpha_of(P, h):
    """The midpoint of the ALPHA interval that ``planner.lts_h`` maps to h (h(0.5) <= h <= P - 1)."""
    n2 = (P + 3) // 2
    assert n2 <= h <= P - 1, (P, h)
    return (h + 0.5 - (2 * n2 - P)) / (2.0 * (P - n2))


def h_range(N):
    P = npairs(N)
    return list(range(st.half_h(P), P))


def _h_list(N):
    P = npairs(N)
    every = h_range(N)
    if N in SMALL_N:
        return tuple(every)
    above = next(h for h in every if alpha_of(P, h) > 0.875)
    return tuple(sorted({every[0], every[0] + 1, planner.lts_h(P, 0.75), above, P - 2, P - 1}))


H_LIST = {N: _h_list(N) for N in ALL_N}
CASES = tuple((N, h) for N in ALL_N for h in H_LIST[N])


def case_id(case):
    return 'N%d-h%d' % case


def exact_fit_expected(N, nbad, h):
    """Whether the pairs of the N - nbad clean elements alone fill an h-subset."""
    m = N - nbad
    return m * (m - 1) // 2 >= h


def bad_elements(name):
    """The number of mistimed elements of a pulse row by its name, None for every other row."""
    kind = name.partition(' ')[0]
    return {'one_bad': 1, 'one_bad_past_breakdown': 1, 'two_bad': 2, 'two_bad_past_breakdown': 2}.get(kind)


def pulse_tables(N):
    """``solve_truth.tables(N)``, the ``short`` set from 16 elements on (the oracle takes seconds per exact-fit window there)."""
    return st.tables(N, short=N >= 16)


def clean_pairs(N, nbad):
    """-> (P,) uint8: 1 for the pairs of the clean elements of a ``one_bad`` (last element mistimed) or ``two_bad`` (last and
    first) row."""
    bad = {N - 1} if nbad == 1 else {N - 1, 0}
    return np.array([i not in bad and j not in bad for i, j in st.pair_table(N)], dtype=np.uint8)


def noisy_windows(N):
    return 40 if N <= 9 else 8 if N <= 16 else 3


@functools.lru_cache(maxsize=None)
def noisy_trace(N):
    """(N, nwin * W + 1) float64, read-only: window w is samples [w W, (w + 1) W), as ``solve_truth.pulse_trace``."""
    x = synthetic.plane_wave(st.grid_geometry(N), noisy_windows(N) * st.W + 1, st.FS, NOISY_BAND[0], NOISY_BAND[1],
                             baz_deg=NOISY_BAZ, vel_kms=NOISY_VEL, snr_db=NOISY_SNR_DB, timing_error_s=NOISY_TIMING_S,
                             bad_element=N - 1, seed=NOISY_SEEDS.get(N, NOISY_SEED + N))
    x = np.ascontiguousarray(x, dtype=np.float64)
    x.flags.writeable = False
    return x


@functools.lru_cache(maxsize=None)
def noisy_lags(N):
    """The oracle's lags of ``noisy_trace(N)`` -> (nwin, P) int64, read-only (``oracle.correlate_windows``: FP64 full-lag
    correlation, first maximum)."""
    import nbls_oracle as oracle
    n = noisy_windows(N)
    tau, _, _ = oracle.correlate_windows(noisy_trace(N).T, st.W, np.arange(n) * st.W, st.pair_table(N), st.FS)
    lag = np.rint(tau.T * st.FS).astype(np.int64)
    assert np.array_equal(lag / st.FS, tau.T)
    lag.flags.writeable = False
    return lag


def plane_lags(N):
    """The lags of the noise-free wave of ``noisy_trace`` in (fractional) samples, the mistimed element included -> (P,)."""
    rij = st.grid_geometry(N)
    baz = np.radians(NOISY_BAZ)
    d = (-np.array([np.sin(baz), np.cos(baz)]) @ rij) / NOISY_VEL
    d[N - 1] += NOISY_TIMING_S
    # element i records s(t - d_i): the correlation of i with j peaks where ``lag_ij = (d_j - d_i) fs`` in the oracle's sign
    return np.array([(d[j] - d[i]) * st.FS for i, j in st.pair_table(N)])


def oracle_noisy(oracle, N, h):
    """``solve_truth.oracle_lts`` on the noisy lags at the ALPHA of h (its cache serves the GPU test of the same session)."""
    xij = planner.co_array(st.grid_geometry(N))[0]
    return st.oracle_lts(oracle, noisy_lags(N), xij, alpha_of(npairs(N), h))


def oracle_search(oracle, N, h):
    """``oracle.fast_lts`` on the noisy lags with subset size h -> zraw (2, nwin)."""
    return oracle_noisy(oracle, N, h)['zraw']


def sampler_gap(oracle, xij, z, sigma_tau, nphi=20000):
    """The distance between the oracle's two evaluations of the confidence intervals of (z, sigma_tau) — the ellipse sampled
    at ``nphi`` points, as ``test_gpu_solve._check_against_oracle`` asks for it, and the closed form — in units of that
    checker's tolerance for the sampled one (rtol 1e-4; atol 1e-12 for the velocity, 1e-7 for the back-azimuth)
    -> (vel (nwin,), baz (nwin,)), NaN where both are NaN."""
    cv, cb = oracle.confidence_intervals_closed_form(xij, z, sigma_tau)
    dv, db = oracle.confidence_intervals(xij, z, sigma_tau, nphi=nphi)
    assert np.array_equal(np.isnan(cv), np.isnan(dv)) and np.array_equal(np.isnan(cb), np.isnan(db))
    with np.errstate(invalid='ignore'):
        return np.abs(cv - dv) / (1e-4 * np.abs(dv) + 1e-12), np.abs(cb - db) / (1e-4 * np.abs(db) + 1e-7)


def mutant_differs(oracle, N, h, h_search):
    """The oracle mutant: FAST-LTS searches with ``h_search`` and ``lts_post_process`` keeps h.  -> bool (nwin,): the
    windows whose final weights, or the bits of whose z, differ from the oracle's with h in both places."""
    xij = planner.co_array(st.grid_geometry(N))[0]
    tau = np.ascontiguousarray(noisy_lags(N).T / st.FS)
    alpha = alpha_of(npairs(N), h)
    r = oracle_noisy(oracle, N, h)
    z, w = np.ascontiguousarray(r['z']), r['weights']
    zm, wm, _ = oracle.lts_post_process(tau, xij, oracle_search(oracle, N, h_search), alpha)
    return np.any(w != wm, axis=0) | np.any(z.view(np.uint64) != zm.view(np.uint64), axis=0)
