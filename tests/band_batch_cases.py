"""ONE case of B = 2 bands x S = 3 recordings, shared by tests/test_band_batch_cases.py (CPU: the conditions that make the
case worth running) and tests/test_gpu_band_batch.py (GPU: a batch against its single calls and against the truths).

In a batch the result row is r = b * S + s while the filter tables and every per-band table of the opt-in results stay per
band.  B != S and both are at least 2, so r / S, r / B, r % B and r % S all differ on the six rows; the two bands differ in
window length (257 and 65 samples: ``nwin`` differs, the shorter row has padding cells), Capon frequency, snapshot length
and hop, and seed half-width, and the recordings in noise and back-azimuth.  N = 4 elements with one mistimed under
alpha = 0.5, so that LTS runs and drops something.  CPU only: nothing here imports the GPU library."""
import functools

import numpy as np

import filter_truth as ft
from narrow_band_least_squares_amd import planner, synthetic

N, FS, NPTS, ALPHA = 4, 20.0, 2401, 0.5
B, S = 2, 3
EDGES = [(0.5, 1.5), (1.5, 4.0)]
WINLENS = [257.5 / FS, 65.5 / FS]
WINDOWS = (257, 65)
OVERLAP = 0.5
FILTER = ('butter', 2, 0.01)
T0 = 17884.0729166667
SEED = 510                # recording s is drawn with seed SEED + s (at 500 two seeded picks of recording 1 lie at lag W - 1,
                          # which the refinement checker excludes: test_band_batch_cases.py holds the case to that)

CAPON_GRID = planner.slowness_grid(3.07, 5)                      # 13 points (5 x 5, those beyond 3.07 s/km dropped)
CAPON_FREQS = planner.capon_frequencies(EDGES)
CAPON_SNAPSHOTS = ([64, 16], [16, 8])                            # (Ls, Hs), one per band
CAPON_LOADING = 0.01
PEAKS, PEAK_FLOOR = 3, 0.0
SEED_GRID = planner.slowness_grid(3.5, 11)                       # 81 points: not the Capon grid's count
SEED_HALFWIDTHS = [6, 3]
MIN_VELOCITY = 0.3

CAPON = dict(capon_grid=CAPON_GRID, capon_freqs=CAPON_FREQS, capon_snapshots=CAPON_SNAPSHOTS, capon_loading=CAPON_LOADING)
SEEDED = dict(slowness_grid=SEED_GRID, seed_halfwidths=SEED_HALFWIDTHS)
# one opt-in result at a time: the keywords ``engine.process`` and ``engine.process_batch`` share
EXTRAS = {
    'beam': dict(want_beam=True),
    'subsample': dict(want_subsample=True),
    'min_velocity': dict(min_velocity=MIN_VELOCITY),
    'grid_map': dict(slowness_grid=SEED_GRID, want_grid_map=True),
    'grid_seed': dict(SEEDED),
    'consistency': dict(want_consistency=True),
    'capon_maps': dict(CAPON, want_capon_maps=True, want_capon_csdm=True),
    'capon_peaks': dict(CAPON, capon_peaks=PEAKS, capon_peak_floor=PEAK_FLOOR),
}
# everything at once (min_velocity is the one option that does not combine with a seed)
ALL_ON = dict(CAPON, want_uncert=True, want_beam=True, want_subsample=True, want_consistency=True, want_grid_map=True,
              want_capon_maps=True, want_capon_csdm=True, capon_peaks=PEAKS, capon_peak_floor=PEAK_FLOOR, **SEEDED)
PICKS = dict(SEEDED, want_subsample=True)                        # the options of ALL_ON that change the picked lags
# the parts of ALL_ON, each with the options that change the picks: (keywords, the fields they own)
PARTS = {
    'uncert': (dict(PICKS, want_uncert=True), ('vel_uncert', 'baz_uncert')),
    'beam': (dict(PICKS, want_beam=True), ('beam_power', 'fstat')),
    'consistency': (dict(PICKS, want_consistency=True), ('consistency', 'closure_max', 'element_consistency')),
    'grid': (dict(PICKS, want_grid_map=True), ('grid_index', 'grid_fstat', 'grid_power', 'grid_map')),
    'capon': (dict(PICKS, want_capon_maps=True, want_capon_csdm=True, capon_peaks=PEAKS, capon_peak_floor=PEAK_FLOOR, **CAPON),
              None),                                             # (None: every Capon and peak field)
}

PLAIN_FIELDS = ('vel', 'baz', 'mdccm', 'sigma_tau', 'mask')
CAPON_FIELDS = ('capon_index', 'capon_power', 'bartlett_index', 'bartlett_power', 'capon_map', 'bartlett_map', 'capon_csdm')
PEAK_FIELDS = tuple(w + f for w in ('capon', 'bartlett') for f in ('_peak_count', '_peak_index', '_peak_power', '_peak_offset'))
# every array a ``BandBatch`` of ``process_batch`` carries (None where the option is off)
FIELDS = (PLAIN_FIELDS + ('vel_uncert', 'baz_uncert', 'beam_power', 'fstat', 'consistency', 'closure_max', 'element_consistency',
                          'grid_index', 'grid_fstat', 'grid_power', 'grid_map') + CAPON_FIELDS + PEAK_FIELDS)


@functools.lru_cache(maxsize=None)
def recordings(npts=NPTS):
    """-> (S arrays (N, npts): different noise and back-azimuth each — what ``_recordings`` of tests/test_gpu_batch.py makes —,
    the centred geometry (2, N), the S start dates)."""
    rij = synthetic.array_geometry(N, 1.0)
    data = [np.ascontiguousarray(synthetic.plane_wave(rij, npts, FS, 0.5, 4.0, baz_deg=20.0 + 67.0 * i, timing_error_s=0.25,
                                                      bad_element=N - 1, seed=SEED + i)) for i in range(S)]
    for d in data:
        d.flags.writeable = False
    return data, rij - rij.mean(axis=1, keepdims=True), [T0 + 0.0173 * i for i in range(S)]


def window_plans():
    """-> per band (W, inc, nwin)."""
    return [planner.window_plan(NPTS, FS, wl, OVERLAP) for wl in WINLENS]


@functools.lru_cache(maxsize=None)
def filtered_truth(s, b):
    """Band ``b`` of recording ``s`` as the filter stage defines it, from the long-double cascade -> (N, NPTS) float64."""
    sos, zero_phase, _ = planner.design_bandpass_many(FILTER[0], EDGES, FILTER[1], FILTER[2], FS)[b]
    y = ft.df2t_truth(sos, recordings()[0][s], zero_phase).astype(np.float64)
    y.flags.writeable = False
    return y
