"""CPU reference of the fractional-sample steering of the beam and the slowness grid (``nbls_set_beam_interpolation``;
DESIGN.md section 22), written from the definition and nothing else: (a) a float64 restatement, operation by operation, and
(b) the same in ``np.longdouble`` with exact coefficients, and the rounding bounds the GPU's float64 results are held to.

L = taps, K = L / 2, k = -K+1 .. K.  For one element with delay tau (float64, |tau| < 2^30):

    n = floor(tau), mu = tau - n in [0, 1)                                   exact
    c_k = (((1.0 * (mu - j_1)) * (mu - j_2)) * ...) / D_k                    j ascending over -K+1 .. K without k,
                                                                             D_k = prod_{j != k} (k - j), an exact integer
    x[t] = ((0.0 + c_{-K+1} y_{-K+1}) + ...) + c_K y_K,  y_k = filt[s0 + t + n + k], 0.0 outside [0, npts)

and b[t], S_b, S_t, D, F, P and the NaN / inf rules are those of tests/beam_truth.py and tests/grid_truth.py.

Tolerances, per cell — derived, not measured.  u = 2^-53.  (b) forms c_k exactly (long double products of exact factors,
2^-64 relative: noise here).  The float64 c_k carries L - 1 rounded subtractions, L - 2 rounded products (the first is by
1.0) and one division: relative error below 2 L u.  The float64 x[t] adds L rounded products in a chain of L additions:
below (L + 1) u sum_k |c_k y_k|.  Together 3 L + 1, and one more u for the terms of second order; with
A[t] = sum_k |c_k| |y_k|:

    e_x[t] = (3 L + 2) u A[t]                                                |x_GPU[t] - x[t]| <= e_x[t]
    e_b[t] = sum_i e_x[i, t]
    E   = 64 (N W) u N S_t                                                   the sums themselves, as in beam_truth
    E_b = E + sum_t (2 |b[t]| e_b[t] + e_b[t]^2)                             |d S_b| <= E_b
    E_t = E + N sum_{i,t} (2 |x_i[t]| e_x[i, t] + e_x[i, t]^2)               |d (N S_t)| <= E_t
    |d P| <= E_b / (N^2 W)
    |d F| <= (N - 1) (E_b D + S_b (E_b + E_t)) / (D (D - E_b - E_t))         inf unless D > E_b + E_t

``power_only`` marks the cells whose F bound exceeds 1e-3 F (or whose F is not finite), as grid_truth does.  No cell is
skipped for a delay near a tie: floor has its jump at the integers, where mu = 0 and mu -> 1 give the same x in the limit,
so one ulp of tau moves x by one ulp's worth — but (a) and the GPU compute tau from the same float64 values anyway."""
import numpy as np

import beam_truth as bt
import grid_truth as gt

LD = np.longdouble
U = LD(2.0) ** -53
TAPS = (4, 6, 8)


def split(tau):
    """tau (float64 array, |tau| < 2^30) -> (n int64, mu float64): floor and the exact remainder."""
    tau = np.asarray(tau, dtype=np.float64)
    fl = np.floor(tau)
    return fl.astype(np.int64), tau - fl


def denominators(taps):
    """D_k, k = -K+1 .. K, as Python integers."""
    K = taps // 2
    out = []
    for k in range(-K + 1, K + 1):
        D = 1
        for j in range(-K + 1, K + 1):
            if j != k:
                D *= k - j
        out.append(D)
    return out


def coefficients(taps, mu, dtype=np.float64):
    """c_k(mu) -> (..., taps) of ``dtype``, in the contract's operation order (``dtype`` long double: (b)'s exact ones)."""
    assert taps in TAPS
    mu = np.asarray(mu, dtype=np.float64).astype(dtype)
    K = taps // 2
    out = np.empty(mu.shape + (taps,), dtype=dtype)
    for m, k in enumerate(range(-K + 1, K + 1)):
        p = np.ones(mu.shape, dtype=dtype)
        for j in range(-K + 1, K + 1):
            if j != k:
                p = p * (mu - dtype(j))
        out[..., m] = p / dtype(denominators(taps)[m])
    return out


def taus_of(xij, s, fs):
    """fs * (xij[:, 0] * s0 + xij[:, 1] * s1), un-fused float64, for the rows ``xij`` (R, 2) and one slowness ``s``."""
    xij = np.asarray(xij, dtype=np.float64)
    return np.float64(fs) * (xij[:, 0] * np.float64(s[0]) + xij[:, 1] * np.float64(s[1]))


def grid_tables(xij, grid, fs, N, taps):
    """The plan's tables -> (n (G, N) int64, c (G, N, taps) float64, tau (G, N) float64, halo); element 0 has tau = 0."""
    grid = np.asarray(grid, dtype=np.float64)
    tau = np.zeros((len(grid), N))
    for g in range(len(grid)):
        tau[g, 1:] = taus_of(np.asarray(xij)[:N - 1], grid[g], fs)
    assert np.all(np.abs(tau) < bt.MAX_DELAY)
    n, mu = split(tau)
    K = taps // 2
    halo = int(max(np.abs(n - K + 1).max(), np.abs(n + K).max()))
    return n, coefficients(taps, mu), tau, halo


def taps_of(row, s0, W, n, taps, dtype):
    """y[k, t] = row[s0 + t + n + k], k = -K+1 .. K, 0.0 outside the trace -> (taps, W) of ``dtype``."""
    K = taps // 2
    t = np.arange(W, dtype=np.int64)
    y = np.zeros((taps, W), dtype=dtype)
    for m, k in enumerate(range(-K + 1, K + 1)):
        idx = s0 + t + int(n) + k
        ok = (idx >= 0) & (idx < len(row))
        y[m, ok] = row[idx[ok]].astype(dtype)
    return y


def rows64(filt, s0, W, n, c):
    """(a): the interpolated rows x (N, W) float64, every product rounded before its addition, the taps ascending."""
    filt = np.asarray(filt, dtype=np.float64)
    N, taps = len(n), c.shape[-1]
    x = np.zeros((N, W))
    for i in range(N):
        y = taps_of(filt[i], s0, W, n[i], taps, np.float64)
        v = np.zeros(W)
        for m in range(taps):
            v = v + c[i, m] * y[m]
        x[i] = v
    return x


def outputs64(x):
    """(a): the float64 sums of the rows x (N, W) in plain t order -> (P, F) by the rules of the kernels."""
    N, W = x.shape
    b = np.zeros(W)
    for i in range(N):
        b = b + x[i]
    S_b, S_t = np.float64(0.0), np.float64(0.0)
    for t in range(W):
        S_b = S_b + b[t] * b[t]
        q = np.float64(0.0)
        for i in range(N):
            q = q + x[i, t] * x[i, t]
        S_t = S_t + q
    if np.isnan(S_b) or np.isnan(S_t):
        return np.nan, np.nan
    if S_t == 0.0:
        return 0.0, np.nan
    D = N * S_t - S_b
    P = S_b / (np.float64(N) * N * W)
    if D <= 0.0 and S_b > 0.0:
        return P, np.inf
    return P, (N - 1.0) * S_b / D


def cell(filt, s0, W, n, mu, taps):
    """(b): one (window, delay row) in long double -> dict: ``power``, ``fstat`` (float64 of the long-double values),
    ``S_b``, ``S_t``, ``D`` (long double), ``tol_power``, ``tol_fstat``, ``power_only``."""
    filt = np.asarray(filt, dtype=np.float64)
    N = len(n)
    c = coefficients(taps, mu, LD)
    x = np.zeros((N, W), dtype=LD)
    ex = np.zeros((N, W), dtype=LD)
    for i in range(N):
        y = taps_of(filt[i], s0, W, n[i], taps, LD)
        x[i] = (c[i][:, None] * y).sum(axis=0)
        ex[i] = (3 * taps + 2) * U * (np.abs(c[i])[:, None] * np.abs(y)).sum(axis=0)
    b = x.sum(axis=0)
    S_b, S_t = (b * b).sum(), (x * x).sum()
    power, fstat, D = bt.outputs(N, W, S_b, S_t)
    out = dict(power=float(power), fstat=float(fstat), S_b=S_b, S_t=S_t, D=D, tol_power=0.0, tol_fstat=np.inf, power_only=True)
    if np.isnan(S_t) or np.isnan(S_b):
        return out
    eb = ex.sum(axis=0)
    E = LD(64.0) * (N * W) * U * N * S_t
    E_b = E + (2 * np.abs(b) * eb + eb * eb).sum()
    E_t = E + N * (2 * np.abs(x) * ex + ex * ex).sum()
    out['tol_power'] = float(E_b / (LD(N) * N * W))
    if np.isfinite(fstat) and D > E_b + E_t:
        tf = (N - 1) * (E_b * D + S_b * (E_b + E_t)) / (D * (D - E_b - E_t))
        out['tol_fstat'] = float(tf)
        out['power_only'] = bool(tf > 1e-3 * fstat)
    return out


def beam_delays(xij_rows, z, fs):
    """The delays of the elements for the co-array rows ``xij_rows`` (N-1, 2) of the pairs (e_0, e_i) and one slowness ``z``
    -> (n (N,) int64, mu (N,) float64), or None where the results are NaN by definition."""
    z0, z1 = np.float64(z[0]), np.float64(z[1])
    if not (np.isfinite(z0) and np.isfinite(z1)):
        return None
    tau = np.concatenate(([0.0], taus_of(xij_rows, (z0, z1), fs)))
    if not np.all(np.abs(tau) < bt.MAX_DELAY):
        return None
    return split(tau)


def beam_reference(filt, fs, xij, z, W, inc, nwin, taps, first=0):
    """(b) for the beam at the solved slowness: the windows [first, first + nwin) of one result row -> dict of (nwin,) arrays
    with the keys of ``beam_truth.beam_reference`` (``skip`` all False), so that ``beam_truth.compare`` judges the GPU's rows.
    ``filt`` (N, npts): the rows of the elements that are summed, ``xij``: the co-array rows of the pairs (e_0, e_i) first;
    ``z`` (>= first + nwin, 2) as fetched from the GPU."""
    filt = np.asarray(filt, dtype=np.float64)
    N = filt.shape[0]
    rows = np.asarray(xij, dtype=np.float64)[:N - 1]
    out = dict(beam_power=np.zeros(nwin), fstat=np.zeros(nwin), tol_power=np.zeros(nwin), tol_fstat=np.zeros(nwin),
               skip=np.zeros(nwin, dtype=bool), power_only=np.zeros(nwin, dtype=bool))
    for k in range(nwin):
        w = first + k
        nm = beam_delays(rows, z[w], fs)
        if nm is None:
            out['beam_power'][k] = out['fstat'][k] = np.nan
            continue
        c = cell(filt, w * int(inc), int(W), nm[0], nm[1], taps)
        out['beam_power'][k], out['fstat'][k] = c['power'], c['fstat']
        out['tol_power'][k], out['tol_fstat'][k], out['power_only'][k] = c['tol_power'], c['tol_fstat'], c['power_only']
    return out


def grid_reference(filt, fs, xij, grid, W, inc, nwin, taps, first=0):
    """(b) for the slowness grid: the windows [first, first + nwin) of one result row -> the dict of
    ``grid_truth.grid_reference`` (``d`` is the n table), so that ``grid_truth.check_window`` judges the GPU's results:
    an arg-max that differs is accepted only where two F values lie within their bounds of each other."""
    filt = np.asarray(filt, dtype=np.float64)
    N = filt.shape[0]
    W, inc = int(W), int(inc)
    n, _, tau, _ = grid_tables(xij, grid, fs, N, taps)
    mu = split(tau)[1]
    G = len(n)
    out = dict(F=np.full((nwin, G), np.nan), P=np.full((nwin, G), np.nan), tol_fstat=np.full((nwin, G), np.inf),
               tol_power=np.zeros((nwin, G)), power_only=np.ones((nwin, G), dtype=bool), index=np.full(nwin, -1, dtype=np.int64),
               fstat=np.full(nwin, np.nan), power=np.full(nwin, np.nan), d=n, tau=tau)
    for k in range(nwin):
        s0 = (first + k) * inc
        bf, bg = LD(0), -1
        for g in range(G):
            c = cell(filt, s0, W, n[g], mu[g], taps)
            out['F'][k, g], out['P'][k, g] = c['fstat'], c['power']
            out['tol_power'][k, g], out['tol_fstat'][k, g], out['power_only'][k, g] = c['tol_power'], c['tol_fstat'], c['power_only']
            if gt.better(c['fstat'], g, bf, bg):
                bf, bg = c['fstat'], g
        out['index'][k] = bg
        if bg >= 0:
            out['fstat'][k], out['power'][k] = out['F'][k, bg], out['P'][k, bg]
    return out


def grid_fstat64(filt, W, starts, n, c):
    """(a), vectorised over the grid: F of every (window, grid point) in float64 -> (nwin, G).  x is formed in the
    contract's operation order; the sums are NumPy's (counting experiments and the demonstration, not a reference for bits:
    equal delay rows still give equal values).  ``n`` (G, N) int, ``c`` (G, N, taps) float64, or None for whole-sample delays
    ``n``."""
    filt = np.asarray(filt, dtype=np.float64)
    N, npts = filt.shape
    n = np.asarray(n, dtype=np.int64)
    taps = 1 if c is None else c.shape[-1]
    K = taps // 2
    lo = 0 if c is None else -K + 1
    H = int(np.abs(n).max()) + K + 1
    pad = np.zeros((N, npts + 2 * H))
    pad[:, H:H + npts] = filt
    views = [np.lib.stride_tricks.sliding_window_view(pad[i], W) for i in range(N)]
    F = np.empty((len(starts), len(n)))
    for k, s0 in enumerate(starts):
        b = np.zeros((len(n), W))
        st = np.zeros(len(n))
        for i in range(N):
            if c is None:
                x = views[i][s0 + H + n[:, i]]
            else:
                x = np.zeros((len(n), W))
                for m in range(taps):
                    x = x + c[:, i, m, None] * views[i][s0 + H + n[:, i] + lo + m]
            b += x
            st += np.einsum('gt,gt->g', x, x)
        sb = np.einsum('gt,gt->g', b, b)
        with np.errstate(invalid='ignore', divide='ignore'):
            F[k] = np.where(st == 0, np.nan, (N - 1) * sb / (N * st - sb))
    return F


def demonstration(taps=8):
    """The small-aperture demonstration of DESIGN.md section 22 -> dict: the filtered trace ``filt`` (8, 6001), ``fs``, ``xij``,
    ``rij``, the 41 x 41 ``grid`` over +-4 s/km, ``W``, ``starts`` (8 windows), ``true`` (the wave's slowness vector in the
    project's convention) and ``max_tau``."""
    from scipy.signal import butter, sosfiltfilt
    from narrow_band_least_squares_amd import planner, synthetic
    fs = 20.0
    rij = synthetic.array_geometry(8, 0.05)
    data = synthetic.plane_wave(rij, 6001, fs, 0.1, 8.0, baz_deg=225, vel_kms=0.34, snr_db=6.0)
    filt = sosfiltfilt(butter(2, [1.0, 3.0], btype='bandpass', fs=fs, output='sos'), np.asarray(data, dtype=np.float64), axis=1)
    xij = planner.co_array(rij)[0]
    ax = np.arange(-20, 21) * 0.2
    grid = np.ascontiguousarray(np.stack(np.meshgrid(ax, ax, indexing='ij'), axis=-1).reshape(-1, 2))
    s = 1.0 / 0.34
    true = np.array([s * np.sin(np.deg2rad(225.0)), s * np.cos(np.deg2rad(225.0))])
    return dict(filt=np.ascontiguousarray(filt), fs=fs, xij=xij, rij=rij, grid=grid, W=400,
                starts=[600 * w + 300 for w in range(8)], true=true)
