"""CPU reference of the slowness-grid search of the beam F-statistic (``nbls_set_beam_grid``), written
from the definition with the ``np.longdouble`` sums of tests/beam_truth.py — and the rounding bounds the GPU's float64
sums are held to.

For one result row (the N element rows ``filt`` (N, npts), the co-array ``xij`` whose first N-1 rows are the pairs (0, i))
and a grid of G slowness vectors ``grid`` (G, 2) s/km:

    d[g, 0] = 0, d[g, i] = rint(fs * (xij[i-1, 0] * s_g0 + xij[i-1, 1] * s_g1))      float64, un-fused, ties to even
    x_i[t] = filt[i, s0 + t + d[g, i]] for t in [0, W), 0.0 outside [0, npts)        s0 = w * inc
    S_b, S_t, D = N S_t - S_b as in beam_truth
    F(g) = (N - 1) S_b / D;  +inf if D <= 0 and S_b > 0;  NaN if S_t == 0 or a NaN sample was read
    P(g) = S_b / (N^2 W)
    index = the g with the largest F under "F descending (+inf first), g ascending", NaN not a candidate; -1 if none

Tolerances, per cell (window, g), those of beam_truth — derived, not measured:

    E = 64 (N W) 2^-53 N S_t;   |d P| <= E / (N^2 W);   |d F| <= (N - 1) (E D + 2 E S_b) / D^2

``power_only`` marks the cells whose F bound exceeds 1e-3 F (or whose F is not finite): the sums line up so well that D is
rounding noise.  A grid is fit for a comparison of delays only if no fs xij . s_g lies within 1e-6 of a half-integer
(``near_tie``): the table is computed from the caller's float64 values, so this is a property of the inputs alone."""
import numpy as np

import beam_truth as bt

LD = np.longdouble


def delay_table(xij, grid, fs, N):
    """-> (d (G, N) int64, tau (G, N-1) float64): the float64 expression of the contract, ``np.rint`` of it."""
    xij = np.asarray(xij, dtype=np.float64)[:N - 1]
    grid = np.asarray(grid, dtype=np.float64)
    tau = np.float64(fs) * (xij[None, :, 0] * grid[:, None, 0] + xij[None, :, 1] * grid[:, None, 1])
    assert np.all(np.abs(tau) < bt.MAX_DELAY)
    d = np.concatenate((np.zeros((len(grid), 1), dtype=np.int64), np.rint(tau).astype(np.int64)), axis=1)
    return d, tau


def near_tie(tau):
    """Whether some fs xij . s_g lies within 1e-6 of a half-integer."""
    return bool(np.any(np.abs(np.abs(tau - np.floor(tau)) - 0.5) < bt.HALF_MARGIN))


def better(f, g, bf, bg):
    """The total order: F descending (+inf first), g ascending; NaN is no candidate, bg < 0 is "none yet"."""
    if np.isnan(f):
        return False
    if bg < 0:
        return True
    return f > bf or (f == bf and g < bg)


def grid_reference(filt, fs, xij, grid, W, inc, nwin, first=0):
    """The windows [first, first + nwin) of one result row -> dict: ``F``, ``P`` (nwin, G) float64 of the long-double values,
    ``tol_fstat``, ``tol_power``, ``power_only`` (nwin, G), ``index`` (nwin,) and ``fstat`` / ``power`` (nwin,) at the index (NaN
    for -1), ``d`` (G, N) and ``tau``."""
    filt = np.asarray(filt, dtype=np.float64)
    N = filt.shape[0]
    W, inc = int(W), int(inc)
    d, tau = delay_table(xij, grid, fs, N)
    G = len(d)
    out = dict(F=np.full((nwin, G), np.nan), P=np.full((nwin, G), np.nan), tol_fstat=np.full((nwin, G), np.inf),
               tol_power=np.zeros((nwin, G)), power_only=np.ones((nwin, G), dtype=bool), index=np.full(nwin, -1, dtype=np.int64),
               fstat=np.full(nwin, np.nan), power=np.full(nwin, np.nan), d=d, tau=tau)
    for k in range(nwin):
        s0 = (first + k) * inc
        seen = {}                                  # identical delay rows give identical values
        bf, bg = LD(0), -1
        for g in range(G):
            key = tuple(d[g])
            if key not in seen:
                S_b, S_t = bt.window_sums(filt, s0, W, d[g])
                power, fstat, D = bt.outputs(N, W, S_b, S_t)
                tp, tf, po = 0.0, np.inf, True
                if not np.isnan(S_t):
                    E = LD(64.0) * (N * W) * LD(2.0) ** -53 * N * S_t
                    tp = float(E / (LD(N) * N * W))
                    if np.isfinite(fstat) and D > 0:
                        tf = float((N - 1) * (E * D + 2 * E * S_b) / (D * D))
                        po = bool(tf > 1e-3 * fstat)
                seen[key] = (power, fstat, tp, tf, po)
            power, fstat, tp, tf, po = seen[key]
            out['F'][k, g], out['P'][k, g] = float(fstat), float(power)
            out['tol_power'][k, g], out['tol_fstat'][k, g], out['power_only'][k, g] = tp, tf, po
            if better(fstat, g, bf, bg):
                bf, bg = fstat, g
        out['index'][k] = bg
        if bg >= 0:
            out['fstat'][k], out['power'][k] = out['F'][k, bg], out['P'][k, bg]
    return out


def check_window(k, ref, idx, fstat, power, fmap=None):
    """Assert one window of the GPU's results (index, F and P there, the map row or None) against ``grid_reference``'s."""
    F, tol = ref['F'][k], ref['tol_fstat'][k]
    nan_ref = np.isnan(F)
    if fmap is not None:
        assert np.array_equal(np.isnan(fmap), nan_ref), (k, np.flatnonzero(np.isnan(fmap) != nan_ref))
        fin = ~nan_ref & np.isfinite(F)
        assert np.all(np.abs(fmap[fin] - F[fin]) <= tol[fin]), (k, np.max(np.abs(fmap[fin] - F[fin]) / tol[fin]))
        inf_ref = ~nan_ref & ~np.isfinite(F)                    # +inf of the reference: D is rounding noise
        assert np.all(fmap[inf_ref] > 1e6), (k, fmap[inf_ref])
    if ref['index'][k] < 0:
        assert idx == -1 and np.isnan(fstat) and np.isnan(power), (k, idx, fstat, power)
        return
    assert 0 <= idx < len(F) and not nan_ref[idx], (k, idx)
    if fmap is not None:
        assert fstat == fmap[idx] or (np.isnan(fstat) and np.isnan(fmap[idx])), (k, idx, fstat, fmap[idx])     # bit-equal
        cand = np.flatnonzero(~np.isnan(fmap))                   # the GPU's own arg-max: first of the largest
        best = cand[np.argmax(fmap[cand])]
        assert idx == best, (k, idx, best)
    assert abs(power - ref['P'][k, idx]) <= ref['tol_power'][k, idx], (k, power, ref['P'][k, idx], ref['tol_power'][k, idx])
    if np.isfinite(F[idx]):
        assert abs(fstat - F[idx]) <= tol[idx], (k, fstat, F[idx], tol[idx])
    ok = ~nan_ref
    with np.errstate(invalid='ignore'):
        lower = np.where(np.isfinite(tol[ok]), F[ok] - tol[ok], np.where(np.isfinite(F[ok]), -np.inf, F[ok]))
        upper_i = F[idx] + tol[idx]
        assert upper_i >= np.max(lower), (k, idx, F[idx], tol[idx], np.max(lower))
        gt = int(ref['index'][k])
        others = np.flatnonzero(ok)
        others = others[others != gt]
        if np.isfinite(F[gt]) and (len(others) == 0 or F[gt] - tol[gt] > np.max(F[others] + tol[others])):
            assert idx == gt, (k, idx, gt)       # the truth's maximum leads by more than both tolerances


def grid_fstat_fast(filt, W, starts, d):
    """F of every (window, grid point) in float64, vectorised over the grid (counting experiments, not a reference for
    bits) -> (nwin, G).  ``d`` (G, N) int."""
    filt = np.asarray(filt, dtype=np.float64)
    N, npts = filt.shape
    d = np.asarray(d, dtype=np.int64)
    H = int(np.abs(d).max())
    pad = np.zeros((N, npts + 2 * H))
    pad[:, H:H + npts] = filt
    views = [np.lib.stride_tricks.sliding_window_view(pad[i], W) for i in range(N)]
    F = np.empty((len(starts), len(d)))
    for k, s0 in enumerate(starts):
        b = np.zeros((len(d), W))
        st = np.zeros(len(d))
        for i in range(N):
            x = views[i][s0 + H + d[:, i]]
            b += x
            st += np.einsum('gt,gt->g', x, x)
        sb = np.einsum('gt,gt->g', b, b)
        with np.errstate(invalid='ignore', divide='ignore'):
            F[k] = np.where(st == 0, np.nan, (N - 1) * sb / (N * st - sb))
    return F
