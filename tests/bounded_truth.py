"""The bounded lag search (``nbls_set_lag_limits``, csrc/xcorr_bounded.hip), stated literally in NumPy.
CPU only: nothing here imports the GPU library.

For a pair of windows a, b of W samples and a limit ``max_lag >= 0``, L = min(max_lag, W-1):

    cij  = np.correlate(a, b, 'full') / sqrt(sum a^2 * sum b^2)          (index W-1-m holds R(m) = sum_n a[n-m] b[n])
    lag  = L - np.argmax(cij[W-1-L : W+L])        first maximum of the slice: among equal maxima the LARGEST lag
    cmax = cij[W-1-lag]

np.argmax treats NaN as the maximum, so a window with NaN or Inf samples gives the first NaN of the slice and cmax = NaN.

**Which cases can be compared exactly.**  A float64 dot product of W <= 130 terms is within W 2^-53 |a| |b| < 2e-14 of the
norm of its true value whatever the order of the sums, so two correct implementations agree on the arg-max whenever the
best and the second-best value of the slice are at least 1e-9 apart in normalised units.  ``pick_windows`` ASSERTS that gap
for every pair it is given (``exact`` names the constructed ties, whose sums are exact); no pair is skipped."""
import numpy as np

MIN_GAP = 1e-9


def limits(xij, fs, vmin):
    """L_k = int(ceil(fs * hypot(xij[k, 0], xij[k, 1]) / vmin)) + 1 -> int64 (P,)."""
    return np.array([int(np.ceil(fs * np.hypot(x, y) / vmin)) + 1 for x, y in np.asarray(xij, dtype=np.float64)], dtype=np.int64)


def pick(a, b, max_lag):
    """One pair -> (lag, cmax, gap): the slice arg-max above; ``gap`` = best minus second-best value of the slice in
    normalised units (inf for a slice of one lag, NaN where the slice holds a NaN)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    W = len(a)
    L = int(min(int(max_lag), W - 1))
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        cij = np.correlate(a, b, 'full') / np.sqrt(np.sum(a * a) * np.sum(b * b))
    sl = cij[W - 1 - L:W + L]
    i = int(np.argmax(sl))
    if len(sl) == 1:
        gap = np.inf
    elif np.isnan(sl).any():
        gap = np.nan
    else:
        top = np.partition(sl, len(sl) - 2)[-2:]
        gap = float(top[1] - top[0])
    return L - i, float(sl[i]), gap


def pick_brute(a, b, max_lag):
    """The same by explicit loops over R(m) = sum_n a[n-m] b[n] (no np.correlate, no slicing) -> (lag, cmax)."""
    W = len(a)
    L = min(int(max_lag), W - 1)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        nrm = np.sqrt(sum(float(x) * float(x) for x in a) * sum(float(x) * float(x) for x in b))
        best, best_m = None, None
        for m in range(L, -L - 1, -1):                     # np.correlate index order: lag descending
            r = 0.0
            for n in range(W):
                if 0 <= n - m < W:
                    r += float(a[n - m]) * float(b[n])
            q = r / nrm
            if best is None or (not np.isnan(best) and (np.isnan(q) or q > best)):      # first NaN, else first maximum
                best, best_m = q, m
    return best_m, best


def pick_windows(data, W, starts, pairs, max_lag, exact=False):
    """``data`` (N, npts), windows of W samples at ``starts``, ``max_lag`` (P,) -> (lag (nwin, P) int64, cmax (nwin, P)).
    Asserts the gap of every finite pair (``exact``: exact-arithmetic cases, where ties are the point)."""
    n, P = len(starts), len(pairs)
    lag = np.zeros((n, P), dtype=np.int64)
    cmax = np.zeros((n, P))
    for w, s in enumerate(starts):
        win = data[:, s:s + W]
        for k, (i, j) in enumerate(pairs):
            lag[w, k], cmax[w, k], gap = pick(win[i], win[j], max_lag[k])
            assert exact or np.isnan(gap) or gap >= MIN_GAP, \
                'window %d pair %d: best and second-best %.3g apart (choose another seed)' % (w, k, gap)
    return lag, cmax


def pair_table(N):
    return [(i, j) for i in range(N - 1) for j in range(i + 1, N)]


def outside(lag, lim):
    """Number of picks outside the physical range: |lag| > L_k."""
    return int(np.count_nonzero(np.abs(lag) > np.asarray(lim)[None, :]))
