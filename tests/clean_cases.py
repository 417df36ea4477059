"""The input sets of the CLEAN-SC tests (tests/test_clean_truth.py on the CPU, tests/test_gpu_clean.py on the GPU; DESIGN.md
section 24.3): traces of 6 W samples of smoothed noise plus a 6 dB two-wave mix at fs = 20 Hz, prefiltered, and the grids of
G points around the kernel's 128 lanes.  The CPU test asserts for every set that truth (a) against truth (b) needs no
waived stop decision; the GPU test runs the same sets."""
import numpy as np

from narrow_band_least_squares_amd import planner, synthetic

FS = 20.0
FREQ = 1.3
FLOOR = 0.02
SHAPES = [(65, 16, 8), (257, 64, 16)]          # (W, Ls, Hs)
ELEMENTS = [3, 8, 32]
GRID_SIZES = [1, 127, 128, 129, 1257]
GAINS = [0.5, 1.0]
STEPS = 6                                      # the one-step check runs i = 0 .. 5


def geometry(N):
    rij = synthetic.array_geometry(N, 1.0)
    return rij - rij.mean(axis=1, keepdims=True)


def traces(N, W, seed=77):
    """(N, 6 W): white noise smoothed by a 5-point Hann kernel, plus two waves (amplitudes 1 and 0.7, 60 and 200 degrees) at 6 dB."""
    rij = geometry(N)
    waves = synthetic.plane_waves(rij, 6 * W, FS, 0.5, 4.0, [(60.0, 0.34, 1.0), (200.0, 0.5, 0.7)], snr_db=6.0, seed=seed + N)
    rng = np.random.default_rng(seed + 1000 + N)
    k = np.hanning(7)[1:-1]
    noise = np.array([np.convolve(rng.standard_normal(6 * W + 4), k / k.sum(), mode='valid') for _ in range(N)])
    return waves + 0.5 * noise, rij


def grid(G):
    """G slowness vectors: the first G of a fixed 1257-point draw in +-3 s/km, rounded to 1e-3 (G = 1257 is cfg-3's size)."""
    rng = np.random.default_rng(40)
    return np.ascontiguousarray(np.round(rng.uniform(-3.0, 3.0, (1257, 2)), 3)[:G])


def single_wave(N, W, g, grid_points):
    """One noise-free sinusoid at FREQ whose delays are those of grid point ``g`` (tau_i = xij[i-1] . s_g, the tables' own):
    every snapshot is a multiple of a[g] up to the leakage of the negative frequency through the Hann taper (Ls = 64 at
    1.3 / 20 cycles per sample: 8.3 bins away, below 2e-4 in amplitude, so below 1e-7 in what CLEAN-SC leaves)."""
    rij = geometry(N)
    xij = planner.co_array(rij)[0]
    tau = np.concatenate([[0.0], xij[:N - 1] @ np.asarray(grid_points)[g]])
    t = np.arange(6 * W) / FS
    return np.cos(2.0 * np.pi * FREQ * (t[None, :] - tau[:, None])), rij


def windows(W, npts, overlap=0.5):
    """(inc, nwin) of the plan for one band of window length W (planner.window_plan)."""
    Wp, inc, nwin = planner.window_plan(npts, FS, (W + 0.5) / FS, overlap)[:3]
    assert int(Wp) == W
    return int(inc), int(nwin)
