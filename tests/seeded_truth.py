"""The seeded lag search (``nbls_set_lag_seed``, csrc/xcorr_seeded.hip), stated literally in NumPy.
CPU only: nothing here imports the GPU library.

For a pair of windows a, b of W samples, a centre c (the delay ``d[g][j] - d[g][i]`` the unit's grid maximum predicts for
the pair; 0 where the unit has none) and a half-width K >= 0:

    c'   = min(max(c, -(W-1)), W-1)
    lo   = max(c' - K, -(W-1)),  hi = min(c' + K, W-1)                     (never empty)
    cij  = np.correlate(a, b, 'full') / sqrt(sum a^2 * sum b^2)            (index W-1-m holds R(m) = sum_n a[n-m] b[n])
    lag  = hi - np.argmax(cij[W-1-hi : W-lo])      first maximum of the slice: among equal maxima the LARGEST lag
    cmax = cij[W-1-lag]

A pair whose sum of squares of either window is not finite (NaN or +-Inf samples) gives lag = hi, cmax = NaN: NumPy's own
answer for NaN samples (every lag is NaN, the first one wins), a deliberate simplification for Inf samples.

**Which cases can be compared exactly** is ``bounded_truth``'s argument: ``pick_windows`` ASSERTS that best and second-best
value of every slice are at least ``bounded_truth.MIN_GAP`` apart (``exact`` names the constructed ties); no pair is skipped."""
import numpy as np

from bounded_truth import MIN_GAP


def search_range(W, c, K):
    """-> (lo, hi) of the contract above, Python integers (no overflow whatever c and K are)."""
    c = min(max(int(c), -(W - 1)), W - 1)
    return max(c - int(K), -(W - 1)), min(c + int(K), W - 1)


def pick(a, b, c, K):
    """One pair -> (lag, cmax, gap): the slice arg-max above; ``gap`` = best minus second-best value of the slice in
    normalised units (inf for a slice of one lag, NaN where the slice holds a NaN)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    W = len(a)
    lo, hi = search_range(W, c, K)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        nrm2 = np.sum(a * a) * np.sum(b * b)
        if not np.isfinite(np.sum(a * a)) or not np.isfinite(np.sum(b * b)):
            return hi, float('nan'), float('nan')
        cij = np.correlate(a, b, 'full') / np.sqrt(nrm2)
    sl = cij[W - 1 - hi:W - lo]
    i = int(np.argmax(sl))
    if len(sl) == 1:
        gap = np.inf
    elif np.isnan(sl).any():
        gap = np.nan
    else:
        top = np.partition(sl, len(sl) - 2)[-2:]
        gap = float(top[1] - top[0])
    return hi - i, float(sl[i]), gap


def pick_brute(a, b, c, K):
    """The same by explicit loops over R(m) = sum_n a[n-m] b[n] (no np.correlate, no slicing) -> (lag, cmax)."""
    W = len(a)
    c = int(c)
    if c < -(W - 1):
        c = -(W - 1)
    if c > W - 1:
        c = W - 1
    lo, hi = c - int(K), c + int(K)
    if lo < -(W - 1):
        lo = -(W - 1)
    if hi > W - 1:
        hi = W - 1
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        ssa, ssb = sum(float(x) * float(x) for x in a), sum(float(x) * float(x) for x in b)
        if not (abs(ssa) < np.inf) or not (abs(ssb) < np.inf):      # NaN or Inf
            return hi, float('nan')
        nrm = np.sqrt(ssa * ssb)
        best, best_m = None, None
        for m in range(hi, lo - 1, -1):                    # np.correlate index order: lag descending
            r = 0.0
            for n in range(W):
                if 0 <= n - m < W:
                    r += float(a[n - m]) * float(b[n])
            q = r / nrm
            if best is None or (not np.isnan(best) and (np.isnan(q) or q > best)):      # first NaN, else first maximum
                best, best_m = q, m
    return best_m, best


def centres(delays, index, pairs):
    """The plan's delay table (G, N) int, the units' grid maxima ``index`` (nwin,) and the pair list -> c (nwin, P) int64:
    ``d[g][j] - d[g][i]``, 0 where the index is -1."""
    d = np.asarray(delays, dtype=np.int64)
    index = np.asarray(index, dtype=np.int64)
    i, j = np.asarray(pairs, dtype=np.int64).T
    c = d[np.maximum(index, 0)][:, j] - d[np.maximum(index, 0)][:, i]
    return np.where((index < 0)[:, None], 0, c)


def pick_windows(data, W, starts, pairs, c, K, exact=False):
    """``data`` (N, npts), windows of W samples at ``starts``, centres ``c`` (nwin, P), half-width K -> (lag (nwin, P)
    int64, cmax (nwin, P)).  Asserts the gap of every finite pair (``exact``: exact-arithmetic cases, where ties are the
    point)."""
    n, P = len(starts), len(pairs)
    lag = np.zeros((n, P), dtype=np.int64)
    cmax = np.zeros((n, P))
    for w, s in enumerate(starts):
        win = data[:, s:s + W]
        for k, (i, j) in enumerate(pairs):
            lag[w, k], cmax[w, k], gap = pick(win[i], win[j], c[w][k], K)
            assert exact or np.isnan(gap) or gap >= MIN_GAP, \
                'window %d pair %d: best and second-best %.3g apart (choose another seed)' % (w, k, gap)
    return lag, cmax
