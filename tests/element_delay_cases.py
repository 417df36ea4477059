"""The inputs shared by tests/test_element_delay_truth.py (CPU) and tests/test_gpu_element_delay.py: the shapes at which the
loops of csrc/element_delay.hip change, and the traces they run on."""
import numpy as np

from narrow_band_least_squares_amd import synthetic

FS = 20.0
T0 = 17884.0729166667
WAVES = 16                      # waves of a workgroup of element_delay_kernel

# (N, W, K): N over the element counts, W around the 64-lane stride and the four-sample unroll (256), K small, the two K at
# which 2K + 1 crosses the wave count (15 and 17 items per element), and the maximum
SHAPES = ([(4, W, 2) for W in (16, 63, 64, 65, 255, 256, 257, 513, 1025)] +
          [(N, 65, 7) for N in (3, 4, 8, 9, 32)] +
          [(8, 257, K) for K in (0, 1, 2, 7, 8, 256)])
# both sides of the staged / global boundary (156 KiB) at N = 32: in W at K = 256 and at K = 100, in K at W = 200
# (19 968 doubles: 33 W + 64 K <= 19 968)
BOUNDARY = [(32, 108, 256), (32, 109, 256), (32, 411, 100), (32, 412, 100), (32, 200, 208), (32, 200, 209)]


def lds_bytes(N, W, K):
    """The formula of ``nbls_element_delay_lds_bytes``."""
    b = (N * (W + 2 * K) + W) * 8
    return b if b <= 156 * 1024 else 0


def trace(N, W, kind, seed=0):
    """About 20 W samples: ``'noise'`` alone, or ``'wave'``, a plane wave at 6 dB over an array of 300 m -> (data, rij)."""
    npts = 20 * W + 7
    rij = synthetic.array_geometry(N, 0.15)
    if kind == 'noise':
        data = np.random.default_rng(1000 + seed + N + W).standard_normal((N, npts))
    else:
        data = synthetic.plane_wave(rij, npts, FS, 0.5, 4.0, baz_deg=60.0, snr_db=6.0, seed=900 + seed + N + W)
    return np.ascontiguousarray(data), rij - rij.mean(axis=1, keepdims=True)


def cpu_slowness(kind, nwin, seed=0):
    """Slowness vectors for the CPU check of an input set, where no solve has run: around the wave's own, or scattered."""
    rng = np.random.default_rng(77 + seed)
    if kind == 'noise':
        return rng.uniform(-6.0, 6.0, size=(nwin, 2))
    s = 1.0 / 0.34
    true = np.array([s * np.sin(np.deg2rad(60.0)), s * np.cos(np.deg2rad(60.0))])
    return true[None, :] + 0.3 * rng.standard_normal((nwin, 2))
