"""ONE call with every opt-in request that combines, shared by tests/test_requests_host.py (CPU: the record of the call
against a stand-in handle) and tests/test_gpu_requests.py (GPU: the call in the three forms of a pass).  N = 5 elements, two
bands that differ in every per-band table (window length 65 and 33, Capon frequency, snapshots, seed half-width, shift
range), a 3 x 3 slowness grid for the grid search and for the spectra (G = 9), K = 2 peaks, I = 2 CLEAN-SC iterations.  A
seed does not combine with ``min_velocity`` and MUSIC not with the spectra of the kept elements: those two stay off.  CPU
only: nothing here opens the GPU library."""
import functools

import numpy as np

from narrow_band_least_squares_amd import planner, synthetic

N, FS, NPTS, ALPHA = 5, 20.0, 601, 0.5
EDGES = [(0.5, 1.5), (1.5, 4.0)]
WINLENS = [65.5 / FS, 33.5 / FS]
WINDOWS = (65, 33)
OVERLAP = 0.5
FILTER = ('butter', 2, 0.01)
T0 = 17884.0729166667
VECTOR_LEN = 4                                   # of the CPU tests' results (the GPU call has its own window count)

_AXIS = np.array([-2.0, 0.0, 2.0])
GRID = np.ascontiguousarray(np.stack(np.meshgrid(_AXIS, _AXIS, indexing='ij'), axis=-1).reshape(-1, 2))      # (9, 2) s/km
PEAKS, ITERATIONS = 2, 2
SEED_HALFWIDTHS = [4, 2]
SHIFTS = [3, 2]
SNAPSHOTS = ([16, 8], [8, 4])                    # (Ls, Hs), one per band
FAMILIES = dict(mdccm_min=0.2, vel_min=0.05, vel_max=50.0, baz_tol=180.0, vel_tol=50.0, min_pixels=1)

# the keywords ``engine.process`` and ``engine.process_batch`` share
ALL_ON = dict(want_uncert=True, want_beam=True, want_subsample=True, slowness_grid=GRID, want_grid_map=True,
              seed_halfwidths=SEED_HALFWIDTHS, want_consistency=True, capon_grid=GRID, capon_freqs=planner.capon_frequencies(EDGES),
              capon_snapshots=SNAPSHOTS, want_capon_maps=True, want_capon_csdm=True, capon_peaks=PEAKS, capon_peak_floor=0.0,
              kept=(None, True, False), capon_clean=(ITERATIONS, 0.5, 0.02, True), capon_music=(2, 0.05, True, True, True, 0.0),
              families=FAMILIES, element_max_shift=SHIFTS, element_delays_kept=True,
              want_beam_trace=dict(window='hann', kept=True), beam_taps=4)
LAGS = dict(want_lag=True, want_cmax=True, want_z=True)          # ... and those of ``process`` alone


@functools.lru_cache(maxsize=None)
def recording():
    """-> (data (N, NPTS), the centred geometry (2, N)): a plane wave with one mistimed element, so that LTS drops pairs."""
    rij = synthetic.array_geometry(N, 1.0)
    data = np.ascontiguousarray(synthetic.plane_wave(rij, NPTS, FS, 0.5, 4.0, baz_deg=87.0, timing_error_s=0.25, bad_element=N - 1,
                                                     seed=77))
    data.flags.writeable = False
    return data, rij - rij.mean(axis=1, keepdims=True)
