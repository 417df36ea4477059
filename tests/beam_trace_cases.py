"""Shapes and inputs shared by the beam-trace tests (``nbls_set_beam_trace``, csrc/beam_trace.hip).

``SEAMS`` lists the smallest shapes at which ``beam_trace_kernel`` can go wrong; tests/test_beam_trace_host.py holds the list
to the tile constants in the kernel's source, tests/test_gpu_beam_trace.py runs it.  The kernel gives one output sample to
one thread: a workgroup of ``THREADS`` threads takes a tile of ``TILE = THREADS * SPT`` consecutive samples of one row, wave
v the ``64 * SPT`` samples [v * 64 * SPT, (v + 1) * 64 * SPT) of the tile, and loops over the windows that can touch the
tile."""
import numpy as np

THREADS, SPT = 256, 4               # BT_THREADS, BT_SPT of csrc/beam_trace.hip
TILE = THREADS * SPT                # BT_TILE: samples of a workgroup's tile
WAVE_SPAN = 64 * SPT                # samples of a wave's share of the tile
FS = 20.0

# (label, N, W, overlap, npts, delay scale): exact traces (``exact_trace``), boxcar synthesis window.  ``delay scale`` k: the
# designed delays are k times the base pattern of ``exact_geometry`` (|D| <= 3 k samples).
SEAMS = (
    ('W=16 (shorter than a wave, 10 windows and more per wave span)', 4, 16, 0.5, TILE + 77, 1),
    ('W=255 (one sample short of a wave span)', 4, WAVE_SPAN - 1, 0.5, 2 * TILE + 1, 4),
    ('W=256 (a wave span)', 4, WAVE_SPAN, 0.5, 2 * TILE + 1, 4),
    ('W=257 (one sample past a wave span: every window straddles a wave edge, some a tile edge)', 4, WAVE_SPAN + 1, 0.5,
     2 * TILE + 1, 4),
    ('W=tile-1', 3, TILE - 1, 0.5, 3 * TILE + 5, 4),
    ('W=tile', 3, TILE, 0.5, 3 * TILE + 5, 4),
    ('W=tile+1 (a window touches three tiles)', 3, TILE + 1, 0.5, 3 * TILE + 5, 4),
    ('npts below one tile', 4, 65, 0.5, 601, 2),
    ('npts = 2 tile - 1', 4, 257, 0.5, 2 * TILE - 1, 4),
    ('npts = 2 tile + 1 (the last tile holds one sample)', 4, 257, 0.5, 2 * TILE + 1, 4),
    ('a tail no window covers', 4, 200, 0.0, TILE + 150, 4),
    ('overlap 0 (C = 1)', 4, 200, 0.0, 2 * TILE + 9, 4),
    ('overlap 0.5 (C = 2)', 4, 200, 0.5, 2 * TILE + 9, 4),
    ('overlap 0.75 (C = 4)', 4, 200, 0.75, 2 * TILE + 9, 4),
    ('overlap 0.9 (C = 10)', 4, 200, 0.9, 2 * TILE + 9, 4),
    ('reads fall off both ends of the trace', 4, 257, 0.5, TILE + 5, 13),
)
EXACT_N = (3, 4, 8, 9, 32)


def exact_geometry(N, scale=1):
    """-> (rij (2, N) km, slow (2,) s/km, D (N,) whole samples): element m records s[n - D_m] of a wave of slowness ``slow``;
    FS * rij . slow = D exactly (coordinates are multiples of 1 / FS km, the slowness is whole), element 0 at the origin,
    D_0 = 0, |D| <= 3 * scale, both signs present."""
    pts = [(0, 0), (1, 0), (0, -1), (-1, 1), (1, 1), (-1, -1), (2, -1), (-2, 1), (1, -2)]
    k = 3
    while len(pts) < N:                                   # more distinct lattice points, delays still within +-3
        for a in range(-k, k + 1):
            for b in (-k, k):
                for p in ((a, b), (b, a)):
                    if p not in pts and abs(2 * p[0] + p[1]) <= 3 and len(pts) < N:
                        pts.append(p)
        k += 1
    q = np.array(pts[:N], dtype=np.int64)
    slow = np.array([2.0, 1.0]) * scale
    rij = np.ascontiguousarray(q.T / FS)
    D = (2 * q[:, 0] + q[:, 1]) * scale
    assert np.array_equal(np.rint(FS * (slow @ rij)).astype(np.int64), D) and D[0] == 0 and len({tuple(p) for p in pts[:N]}) == N
    return rij, slow, D


def exact_trace(N, npts, scale=1, seed=5):
    """Small-integer traces with designed whole-sample delays: x_m = np.roll(s, D_m), s integers in [-8, 8] -> (data (N, npts),
    rij, s, D).  Every sum of a beam over them is exact in float64."""
    rij, _, D = exact_geometry(N, scale)
    s = np.random.default_rng(seed).integers(-8, 9, size=npts).astype(np.float64)
    return np.stack([np.roll(s, int(d)) for d in D]), rij, s, D


# ---- the demonstration: a plane wave at low SNR over 8 elements ----

# ``mdccm_min``: the demonstration's gate, between the MdCCM of its windows (0.31 and more) and of windows of band-passed noise
# alone (0.28 and less; tests/test_beam_trace_truth.py holds both sides on the CPU)
DEMO = dict(N=8, fs=FS, W=2400, hop=1200, nwin=20, band=(0.8, 1.2), snr_db=-6.0, baz=225.0, vel=0.34, mdccm_min=0.295)
DEMO['npts'] = DEMO['W'] + (DEMO['nwin'] - 1) * DEMO['hop'] + 1


def demo_traces():
    """-> (noisy (8, npts), clean (8, npts), rij): ``synthetic.plane_wave`` on ``array_geometry(8, 1.0)`` at -6 dB and the same
    wave without noise (the generator draws the signal first: the same seed gives the same wave), both band-passed
    0.8 - 1.2 Hz with a zero-phase Butterworth filter (scipy, as the oracle's filter is)."""
    from scipy import signal
    from narrow_band_least_squares_amd import synthetic
    rij = synthetic.array_geometry(DEMO['N'], 1.0)
    sos = signal.butter(2, DEMO['band'], 'bandpass', fs=FS, output='sos')
    noisy = synthetic.plane_wave(rij, DEMO['npts'], FS, 0.1, 5.0, baz_deg=DEMO['baz'], vel_kms=DEMO['vel'], snr_db=DEMO['snr_db'])
    clean = synthetic.plane_wave(rij, DEMO['npts'], FS, 0.1, 5.0, baz_deg=DEMO['baz'], vel_kms=DEMO['vel'], snr_db=400.0)
    band = lambda d: np.ascontiguousarray(signal.sosfiltfilt(sos, d, axis=1))
    return band(noisy), band(clean), rij


def demo_noise(seed=11):
    """-> (8, npts) white noise through the demonstration's band-pass: what its windows look like without the wave."""
    from scipy import signal
    sos = signal.butter(2, DEMO['band'], 'bandpass', fs=FS, output='sos')
    return np.ascontiguousarray(signal.sosfiltfilt(sos, np.random.default_rng(seed).standard_normal((DEMO['N'], DEMO['npts'])), axis=1))


def residual_ratio(trace, noisy0, clean0):
    """Residual power of the beam trace against the noise-free element 0 over that of element 0 itself, over the samples the
    windows cover.  Incoherent noise predicts 1 / N."""
    n = DEMO['W'] + (DEMO['nwin'] - 1) * DEMO['hop']
    return float(np.mean((trace[:n] - clean0[:n]) ** 2) / np.mean((noisy0[:n] - clean0[:n]) ** 2))
