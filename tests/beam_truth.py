"""CPU reference of the beam results (``nbls_set_beam``), written from the definition and nothing
else, with ``np.longdouble`` sums — and the rounding bound the GPU's float64 sums are held to.

For one result row (the N element rows ``filt`` (N, npts) of an estimator, its co-array ``xij`` (P, 2) whose first N-1
rows are the pairs (0, i), and the slowness ``z`` (nwin, 2) AS FETCHED FROM THE GPU):

    d_0 = 0, d_i = rint(fs * (xij[i-1, 0] * z0 + xij[i-1, 1] * z1))            float64, ties to even
    x_i[t] = filt[i, s0 + t + d_i] for t in [0, W), 0.0 outside [0, npts)       s0 = w * inc
    b[t] = sum_i x_i[t];  S_b = sum_t b[t]^2;  S_t = sum_t sum_i x_i[t]^2;  D = N S_t - S_b
    beam_power = S_b / (N^2 W);  fstat = (N - 1) S_b / D
    D <= 0 and S_b > 0: fstat = +inf;  S_t == 0: fstat = NaN, beam_power = 0
    z not finite, some |fs xij . z| >= 2^30, a NaN sample read: both NaN

Tolerance (float64 sums of N W terms in any order, 64 ulps of slack per term):

    E = 64 (N W) 2^-53 N S_t;   |dS_b| <= E, |d(N S_t)| <= E
    |d beam_power| <= E / (N^2 W);   |d fstat| <= (N - 1) (E D + 2 E S_b) / D^2

A window is left out of a comparison (``skip``) when some fs xij . z lies within 1e-6 of a half-integer: one ulp of z
could flip its delay.  Windows whose fstat bound exceeds 1e-3 fstat (``power_only``) are compared on beam_power alone."""
import numpy as np

LD = np.longdouble
HALF_MARGIN = 1e-6
MAX_DELAY = 2.0 ** 30


def delays(xij, z, fs):
    """The delays of the elements for the co-array rows ``xij`` (N-1, 2) of the pairs (0, i) and one slowness ``z`` ->
    (d (N,) int64 — None where the results are NaN by definition —, whether some fs xij . z is within 1e-6 of a tie)."""
    xij = np.asarray(xij, dtype=np.float64)
    z0, z1 = np.float64(z[0]), np.float64(z[1])
    if not (np.isfinite(z0) and np.isfinite(z1)):
        return None, False
    tau = np.float64(fs) * (xij[:, 0] * z0 + xij[:, 1] * z1)
    if not np.all(np.abs(tau) < MAX_DELAY):
        return None, False
    near = bool(np.any(np.abs(np.abs(tau - np.floor(tau)) - 0.5) < HALF_MARGIN))
    return np.concatenate(([0], np.rint(tau).astype(np.int64))), near


def window_sums(filt, s0, W, d):
    """The aligned samples of one window and their two sums, long double -> (S_b, S_t)."""
    N, npts = filt.shape
    t = np.arange(W, dtype=np.int64)
    x = np.zeros((N, W), dtype=LD)
    for i in range(N):
        idx = s0 + t + int(d[i])
        ok = (idx >= 0) & (idx < npts)
        x[i, ok] = filt[i, idx[ok]].astype(LD)
    b = x.sum(axis=0)
    return (b * b).sum(), (x * x).sum()


def outputs(N, W, S_b, S_t):
    """-> (beam_power, fstat, D) from the two sums (any float type)."""
    D = N * S_t - S_b
    if np.isnan(S_b) or np.isnan(S_t):
        return np.nan, np.nan, D
    if S_t == 0:
        return 0.0, np.nan, D
    power = S_b / (LD(N) * N * W)
    if D <= 0 and S_b > 0:
        return power, np.inf, D
    return power, (N - 1) * S_b / D, D


def beam_reference(filt, fs, xij, z, W, inc, nwin, first=0):
    """The windows [first, first + nwin) of one result row -> dict of (nwin,) arrays: ``beam_power``, ``fstat`` (float64
    of the long-double values), ``S_b``, ``S_t``, ``D`` (long double), ``tol_power``, ``tol_fstat``, ``skip`` (delay within
    1e-6 of a tie) and ``power_only`` (fstat bound above 1e-3 fstat).  ``xij``: the estimator's co-array, pairs (0, i)
    first; ``z`` (>= first + nwin, 2)."""
    filt = np.asarray(filt, dtype=np.float64)
    N = filt.shape[0]
    xij0 = np.asarray(xij, dtype=np.float64)[:N - 1]
    out = dict(beam_power=np.zeros(nwin), fstat=np.zeros(nwin), S_b=np.zeros(nwin, dtype=LD), S_t=np.zeros(nwin, dtype=LD),
               D=np.zeros(nwin, dtype=LD), tol_power=np.zeros(nwin), tol_fstat=np.zeros(nwin),
               skip=np.zeros(nwin, dtype=bool), power_only=np.zeros(nwin, dtype=bool))
    for k in range(nwin):
        w = first + k
        d, near = delays(xij0, z[w], fs)
        out['skip'][k] = near
        if d is None:
            out['beam_power'][k] = out['fstat'][k] = np.nan
            out['S_b'][k] = out['S_t'][k] = out['D'][k] = np.nan
            continue
        S_b, S_t = window_sums(filt, w * int(inc), int(W), d)
        power, fstat, D = outputs(N, int(W), S_b, S_t)
        out['S_b'][k], out['S_t'][k], out['D'][k] = S_b, S_t, D
        out['beam_power'][k], out['fstat'][k] = float(power), float(fstat)
        if np.isnan(S_t):
            continue
        E = LD(64.0) * (N * int(W)) * LD(2.0) ** -53 * N * S_t
        out['tol_power'][k] = float(E / (LD(N) * N * int(W)))
        if np.isfinite(fstat) and D > 0:
            tf = (N - 1) * (E * D + 2 * E * S_b) / (D * D)
            out['tol_fstat'][k] = float(tf)
            out['power_only'][k] = bool(tf > 1e-3 * fstat)
        else:
            out['tol_fstat'][k] = np.inf
            out['power_only'][k] = True
    return out


def compare(got_power, got_fstat, ref, max_skipped=0.01):
    """Assert the GPU's (nwin,) rows against ``beam_reference``'s -> (cells compared on fstat, cells skipped).  NaN and
    beam_power 0 must sit in exactly the reference's cells; at most ``max_skipped`` of the cells may be left out."""
    n = len(ref['beam_power'])
    skip = ref['skip']
    assert skip.sum() <= max_skipped * n, '%d of %d cells are within 1e-6 of a delay tie: change the seed' % (skip.sum(), n)
    on_f = 0
    for k in range(n):
        if skip[k]:
            continue
        p, f = float(got_power[k]), float(got_fstat[k])
        rp, rf = ref['beam_power'][k], ref['fstat'][k]
        if np.isnan(rp):
            assert np.isnan(p) and np.isnan(f), (k, p, f)
            continue
        assert abs(p - rp) <= ref['tol_power'][k], (k, p, rp, ref['tol_power'][k])
        if np.isnan(rf):
            assert np.isnan(f) and p == 0.0, (k, p, f)
        elif ref['power_only'][k]:
            assert not np.isnan(f), (k, f)
        else:
            assert abs(f - rf) <= ref['tol_fstat'][k], (k, f, rf, ref['tol_fstat'][k])
            on_f += 1
    return on_f, int(skip.sum())
