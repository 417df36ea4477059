"""The cases of tests/test_gpu_seams.py — window lengths, array sizes and halos at which the loops of beam_fstat_kernel
(csrc/beam.hip), beam_grid_kernel (csrc/beam_grid.hip) and refine_lag_kernel (csrc/refine.hip) change — built from the
kernels' constants, and their inputs.  CPU only: tests/test_seam_cases.py checks here, without a GPU, that every case
reaches the seam it was built for and that the references alone meet the conditions of the comparisons.

Constants the library does not export are stated below beside their source line; test_seam_cases.py reads the source
and fails when one of them has moved."""
import functools
import os

import numpy as np

import beam_truth as bt
import grid_truth as gt
import test_gpu_beam as tb
import test_gpu_grid as tg
import test_gpu_subsample as ts
from narrow_band_least_squares_amd import planner, _hip

FS = 20.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'narrow_band_least_squares_amd', 'csrc')

LANES = 64               # a wave
BEAM_WAVES = 4           # beam.hip:22   constexpr int BEAM_WAVES = 4;
BEAM_WAVE_W = 512        # beam.hip:23   constexpr int BEAM_WAVE_W = 512;   (up to here one wave sums a unit)
BEAM_TU = 4              # beam.hip:52   constexpr int BEAM_TU = 4;         (samples of a lane per trip of the t loop)
GRID_TU = 4              # beam_grid.hip:34   constexpr int GRID_TU = 4;    (GRID_BLOCK = 64 * GRID_TU samples per step)
REFINE_STEP = 64         # refine.hip:82   for (int n = lane; n < W; n += 64)
REFINE_WAVES = (4, 8)    # refine.hip:27-28   REFINE_WAVES (global-memory form), REFINE_LDS_WAVES (LDS form)
# (file, regular expression with one group, the value stated above): what test_seam_cases.py holds the source to
STATED = (('beam.hip', r'constexpr int BEAM_WAVES = (\d+);', BEAM_WAVES),
          ('beam.hip', r'constexpr int BEAM_WAVE_W = (\d+);', BEAM_WAVE_W),
          ('beam.hip', r'constexpr int BEAM_TU = (\d+);', BEAM_TU),
          ('beam.hip', r'if \(coop\) beam_sums<BEAM_WAVES \* (\d+)>\(', LANES),
          ('beam.hip', r'else beam_sums<(\d+)>\(', LANES),
          ('beam_grid.hip', r'constexpr int GRID_TU = (\d+);', GRID_TU),
          ('beam_grid.hip', r'constexpr int GRID_BLOCK = (\d+) \* GRID_TU;', LANES),
          ('refine.hip', r'for \(int n = lane; n < W; n \+= (\d+)\)', REFINE_STEP),
          ('refine.hip', r'constexpr int REFINE_WAVES = (\d+);', REFINE_WAVES[0]),
          ('refine.hip', r'constexpr int REFINE_LDS_WAVES = (\d+);', REFINE_WAVES[1]))

BEAM_WAVE_STEP = LANES * BEAM_TU                    # 256: one trip of a wave that sums a unit alone
BEAM_COOP_STEP = BEAM_WAVES * LANES * BEAM_TU       # 1024: one trip of the four waves of a long unit
GRID_BLOCK = LANES * GRID_TU                        # 256: one step of a wave of the search kernel


def _around(*edges):
    return sorted({w for e, both in edges for w in ((e - 1, e, e + 1) if both else (e - 1, e))})


# one short of, at (and, where the next length takes another path, one past) every edge of the t loops
BEAM_SEAMS = _around((BEAM_WAVE_STEP, False), (BEAM_WAVE_W, True), (BEAM_COOP_STEP, True))
GRID_SEAMS = _around((GRID_BLOCK, False), (2 * GRID_BLOCK, True))
REFINE_SEAMS = _around((REFINE_STEP, False), (2 * REFINE_STEP, True))
REFINE_SWITCH_N = (3, 32)
GRID_CAP_SHAPES = ((4, 257, 24), (32, 65, 11))      # (N, W, windows): enough of them for the far end of the block to hold samples
SIZES = ((16, 0.5), (17, 1.0), (32, 0.5))           # LTS (bucket kernel) at 16 and 32 elements, OLS at 17
SIZE_W = (LANES + 1, BEAM_WAVE_W + 1)               # 65: one wave per unit; 513: the four waves of a workgroup
BEAM_SIZE_CASES = tuple((N, a, W) for N, a in SIZES for W in SIZE_W)
OTHER_SIZE_CASES = tuple(c for c in BEAM_SIZE_CASES if c[0] != 32 or c[2] == SIZE_W[0])
MIXED_BANDS = ((0.5, 1.5), (1.5, 4.0))
MIXED_W = (BEAM_WAVE_W + 1, LANES + 1)              # one cooperative band and one of one wave per unit
MIXED_NPTS = 2001
SUB_REMOVE = (3, 17)                                # the sub-array estimator: 30 of 32 elements
CRAFTED_W = (16, 65)


def winlen(W):
    return (W + 0.5) / FS


def trace_len(W, nwin=11, overlap=0.5):
    """An odd trace length (the padded row length differs from it) that holds exactly ``nwin`` windows of W samples and
    ends two or three samples behind the last one: a delay of four samples reads behind the trace's end."""
    inc = planner.window_plan(10 ** 9, FS, winlen(W), overlap)[1]
    n = W + (nwin - 1) * inc + 2
    return n + 1 - n % 2


def refine_switch(N):
    """The longest window of N elements that refine_lag_kernel stages in LDS (``nbls_refine_lds_bytes``)."""
    assert _hip.refine_lds_bytes(N, 2) > 0
    lo, hi = 2, 4
    while _hip.refine_lds_bytes(N, hi) > 0:
        lo, hi = hi, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _hip.refine_lds_bytes(N, mid) > 0 else (lo, mid)
    return lo


def largest_staged_halo(N, W):
    """The largest halo with which beam_grid_kernel stages a unit of N x W samples in LDS (``nbls_beam_grid_lds_bytes``)."""
    lib = _hip.load_library()
    assert lib.nbls_beam_grid_lds_bytes(N, W, 0) == N * W * 8
    lo, hi = 0, 1
    while lib.nbls_beam_grid_lds_bytes(N, W, hi) > 0:
        lo, hi = hi, 2 * hi
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if lib.nbls_beam_grid_lds_bytes(N, W, mid) > 0 else (lo, mid)
    return lo


def point_with_delay(xij, N, H):
    """One slowness vector along the axis of the largest |xij| component of the pairs (0, i) whose largest delay is
    exactly H samples, clear of rounding ties (``gt.near_tie``): the element of that component is read at H + delta
    samples, delta the first of 0, +-0.1, +-0.2, +-0.3 that leaves no other element near a tie."""
    x = np.asarray(xij, dtype=np.float64)[:N - 1]
    k, c = np.unravel_index(np.argmax(np.abs(x)), x.shape)
    for delta in (0.0, 0.1, -0.1, 0.2, -0.2, 0.3, -0.3):
        s = np.zeros(2)
        s[c] = (H + delta) / (FS * abs(x[k, c]))
        d, tau = gt.delay_table(xij, s[None], FS, N)
        if int(np.abs(d).max()) == H and abs(int(d[0, k + 1])) == H and not gt.near_tie(tau):
            return s
    raise AssertionError('no grid point with a largest delay of %d samples clear of ties' % H)


def far_grid(xij, N, W):
    """GRID5 and one point whose delay is past the LDS cap for windows of W samples: the plan takes the global form."""
    return np.concatenate((tg.GRID5, point_with_delay(xij, N, largest_staged_halo(N, W) + 233)[None]))


def cap_grids(xij, N, W):
    """-> (H, GRID5 + a point with largest delay H, GRID5 + a point with largest delay H + 1), H the largest staged halo."""
    H = largest_staged_halo(N, W)
    return H, [np.concatenate((tg.GRID5, point_with_delay(xij, N, h)[None])) for h in (H, H + 1)]


@functools.lru_cache(maxsize=None)
def _plane_wave(N, npts, mistimed):
    data, rij = tb._wave(N, npts, mistimed=mistimed)
    return data, rij


def plane_wave(N, W, mistimed=False, nwin=11, npts=None, swap=False):
    """The plane wave of test_gpu_beam.py / test_gpu_grid.py (6 dB SNR over a 1 km array), ``trace_len(W, nwin)`` samples.
    ``swap``: elements 0 and 1 change places — the delays are relative to element 0, and the generator's element 0 is
    the last one the wave reaches: every delay then has one sign, and a window reads outside one end of the trace only."""
    data, rij = _plane_wave(N, trace_len(W, nwin) if npts is None else npts, bool(mistimed))
    if swap:
        order = [1, 0] + list(range(2, N))
        data, rij = np.ascontiguousarray(data[order]), np.ascontiguousarray(rij[:, order])
    return data, rij


@functools.lru_cache(maxsize=None)
def _sinusoids(N, W, npts, mistimed):
    data, rij = ts._wave(N, W, npts=npts, mistimed=mistimed)
    return data, rij


def sinusoids(N, W, mistimed=False, nwin=11):
    """The band-limited wave at fractional delays of test_gpu_subsample.py, ``trace_len(W, nwin)`` samples."""
    return _sinusoids(N, W, trace_len(W, nwin), bool(mistimed))


def reads_outside(xij, z, W, inc, nwin, npts, N):
    """-> (windows that read before the trace's start, windows that read behind its end) at the slowness ``z`` (nwin, 2)."""
    before = behind = 0
    for w in range(nwin):
        d, _ = bt.delays(xij[:N - 1], z[w], FS)
        if d is not None:
            before += bool(w * inc + d.min() < 0)
            behind += bool(w * inc + W - 1 + d.max() >= npts)
    return before, behind


# ---- crafted windows for the last refined lag -------------------------------------------------------------------------
# Four channels, hop = W.  A "plus" window: channel 0 holds 1.0, 0.5 at samples 0, 1; channel 1 holds 1.0, 0.25 at samples
# W-2, W-1; channel 2 a unit pulse at 0, channel 3 one at W-1.  With R(m) = sum_n a[n - m] b[n]:
#   pair (0, 1): R(W-1) = 0.25 (one term), R(W-2) = 1 + 0.125 (two), R(W-3) = 0.5 (three, one of them 0)
#                -> lag +(W-2), Nn = 0.25, D = -1.5, frac = -1/12
#   pair (1, 2): R(-(W-1)) = 0.25, R(-(W-2)) = 1, R(-(W-3)) = 0 -> lag -(W-2), Nn = 0.25, D = -1.75, frac = -1/14
#   pairs (0, 3), (2, 3): lag +(W-1) -> frac 0 by the rule |l| >= W-1
# A "minus" window swaps channels 0 <-> 1 and 2 <-> 3: pair (0, 1) has lag -(W-2) and frac +1/12, pair (2, 3) lag -(W-1).
# Every window's neighbours hold pulses at their first and last samples: a term read outside the window is not a zero.
PLUS = ([(0, 1.0), (1, 0.5)], [(-2, 1.0), (-1, 0.25)], [(0, 1.0)], [(-1, 1.0)])
MINUS = (PLUS[1], PLUS[0], PLUS[3], PLUS[2])
CRAFTED_PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def crafted_trace(W, kinds):
    """``kinds``: one of '+', '-' per window -> (4, len(kinds) * W + 1): window w is samples [w W, (w + 1) W)."""
    x = np.zeros((4, len(kinds) * W + 1))
    for w, kind in enumerate(kinds):
        for ch, pulses in enumerate(PLUS if kind == '+' else MINUS):
            for pos, amp in pulses:
                x[ch, w * W + pos % W] = amp
    return x


def crafted_lags(kinds, W):
    """The designed lags (nwin, 6) of ``CRAFTED_PAIRS``: p_j - p_i of the 1.0 pulses."""
    main = {'+': (0, W - 2, 0, W - 1), '-': (W - 2, 0, W - 1, 0)}
    return np.array([[main[k][j] - main[k][i] for i, j in CRAFTED_PAIRS] for k in kinds], dtype=np.int64)


CRAFTED_KINDS = '-+-+-'
CRAFTED_GEOMETRY = np.array([[0.0, 0.30, -0.20, 0.10], [0.0, 0.10, 0.40, -0.35]])
# the NaN trace: '+' at window 1 with a NaN in channel 0 one sample before it, '-' at window 2 with one right behind it
NAN_KINDS = '++-+'


def crafted_nan_trace(W):
    """Channel 0 is ``a`` of pair (0, 1).  At l = +(W-2) the term R(l+1) leaves out reads a[-1], at l = -(W-2) the term
    R(l-1) leaves out reads a[W]: NaN at exactly those two samples of the trace (the last of window 0, the first of window
    3), so a kernel that added them "as zeros" would give NaN.  (A NaN inside a window makes every lag of its pairs NaN
    and the pick W-1 by NumPy's semantics, which the rule |l| >= W-1 answers with 0: nothing left to refine.)"""
    x = crafted_trace(W, NAN_KINDS)
    x[0, W - 1] = np.nan
    x[0, 3 * W] = np.nan
    return x
