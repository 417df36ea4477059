"""The input sets of the MUSIC tests (tests/test_music_truth.py on the CPU, tests/test_gpu_music.py on the GPU; DESIGN.md section
25.3): prefiltered traces of S plane waves at 40 dB, fs = 20 Hz, 2 W + 2 samples (three windows), and grids of G points around
the kernel's 128 lanes.  The condition on the inputs — gap = lambda_M - lambda_{M+1} >= 1e-3 lambda_1 in every compared cell
— is asserted on the CPU for the truth of every set (the seeds below were chosen for it) and again on the GPU's own R."""
import numpy as np

from narrow_band_least_squares_amd import planner, synthetic

FS = 20.0
FREQ = 1.3
BAND = (0.7, 1.9)                              # the waves' band: more Fourier bins than sources, all inside the snapshot's bin
SHAPES = [(65, 16, 8), (257, 64, 16)]          # (W, Ls, Hs): K = 7 and 13 snapshots
ELEMENTS = [3, 4, 5, 8, 31, 32]
GRID_SIZES = [1, 129, 300]
GAP = 1e-3
EIG_FLOOR = 0.05
SEEDS = {}                                     # (N, W, S) -> seed where the default N + S misses the condition


def geometry(N):
    rij = synthetic.array_geometry(N, 1.0)
    return rij - rij.mean(axis=1, keepdims=True)


def sources(S):
    """S waves of amplitudes 1 .. 0.6, back-azimuths spread over the circle from 50 degrees, 0.34 km/s."""
    return [(50.0 + 360.0 * i / S, 0.34, 1.0 - 0.4 * i / max(S - 1, 1)) for i in range(S)]


def source_counts(N):
    """The numbers of sources of an array's sets: 1, 2 and N - 1 (once each)."""
    return sorted({1, 2, N - 1})


def has_gap(N, W, Ls, Hs, S):
    """R of K snapshots has rank K at most, so behind M = S >= K + 1 there is no gap at all; and with S = K the last signal
    eigenvalue is what the K-th snapshot adds to the K - 1 others, which for half-overlapping Hann snapshots of a
    band-limited trace is 1e-6 lambda_1 (N = 8, K = 7), whatever the seed.  So the D of M = S is compared where S < K and
    S < N: at N = 31, 32 and at N = 8, K = 7 the sets with S = N - 1 check everything but D against the truth."""
    return S < 1 + (W - Ls) // Hs and S < N


def traces(N, W, S):
    rij = geometry(N)
    seed = SEEDS.get((N, W, S), 1000 + 37 * N + S)
    return synthetic.plane_waves(rij, 2 * W + 2, FS, BAND[0], BAND[1], sources(S), snr_db=40.0, seed=seed), rij


def grid(G):
    """G slowness vectors: the first G of a fixed 300-point draw in +-3 s/km, rounded to 1e-3."""
    rng = np.random.default_rng(41)
    return np.ascontiguousarray(np.round(rng.uniform(-3.0, 3.0, (300, 2)), 3)[:G])


def windows(W, npts, overlap=0.5):
    """(inc, nwin) of the plan for one band of window length W (planner.window_plan)."""
    Wp, inc, nwin = planner.window_plan(npts, FS, (W + 0.5) / FS, overlap)[:3]
    assert int(Wp) == W
    return int(inc), int(nwin)


def sets():
    """Every (N, G, (W, Ls, Hs), S): G cycles so that every array sees every grid size."""
    out = []
    for N in ELEMENTS:
        k = 0
        for shape in SHAPES:
            for S in source_counts(N):
                out.append((N, GRID_SIZES[k % 3], shape, S))
                k += 1
    return out
