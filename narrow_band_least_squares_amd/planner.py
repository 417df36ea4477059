"""Host-side planning for the HIP path: filter design, taper ramps, window plan, co-array,
and the FAST-LTS constants / start list.  Everything here is small NumPy/SciPy work done once
per call; the per-sample and per-window arithmetic runs in ``csrc/*.hip``.

Reference sources restated (file:line relative to the reference checkout; [R] = recalled
public algorithm of a dependency whose source is not in the checkout):

* filter design ............ helpers.py:126-130; obspy ``bandpass`` [R]
* taper .................... helpers.py:139; obspy ``Trace.taper`` [R]
* windows .................. lts_array ``DataBin`` [R]
* co-array, h, starts ...... lts_array ``LsBeam`` / ``LTSEstimator`` [R]
* scale factors ............ R ``robustbase::ltsReg`` (``LTScnp2``, ``LTScnp2.rew``) [R]
"""
import math

import functools

import numpy as np
from scipy import signal
from scipy.stats import norm

# ---- FAST-LTS constants [R]; one place to correct them against the real lts_array ----
LTS_N_SAMPLES = 500
LTS_CSTEPS = 4
LTS_CSTEPS2 = 100
LTS_CANDIDATES = 10
LTS_DIM = 2
LTS_QUANTILE = float(norm.ppf(0.9875))
LTS_ZERO_SCALE = 1e-7
MAD_CONST = 1.4826
TAPER_FRACTION = 0.01          # helpers.py:139


def design_bandpass(filter_type, fmin, fmax, order, ripple, fs):
    """-> (sos applied to the data, zero_phase flag, sos returned to the caller).  The design itself is
    cached (a band set is usually reused for many traces); the Nyquist warning is raised on every call."""
    sos_apply, zero_phase, sos_ret, nyquist = _design_cached(filter_type, float(fmin), float(fmax), int(order),
                                                             float(ripple), float(fs))
    if nyquist:
        import warnings
        warnings.warn('Selected high corner frequency (%s) of bandpass is at or above Nyquist (%s). '
                      'Applying a high-pass instead.' % (fmax, 0.5 * fs))
    return sos_apply.copy(), zero_phase, sos_ret.copy()


@functools.lru_cache(maxsize=4096)
def _design_cached(filter_type, fmin, fmax, order, ripple, fs):
    if filter_type == 'butter':
        fe = 0.5 * fs
        low, high = fmin / fe, fmax / fe
        nyquist = high - 1.0 > -1e-6
        if nyquist:
            z, p, k = signal.iirfilter(order, low, btype='highpass', ftype='butter', output='zpk')
            sos_apply = signal.zpk2sos(z, p, k)
            sos_ret = signal.iirfilter(order, [fmin, fmax], btype='band', ftype='butter', fs=fs, output='sos')
            return sos_apply, True, sos_ret, nyquist
        if low > 1:
            raise ValueError('Selected low corner frequency is above Nyquist.')
        # obspy designs on [fmin / (fs/2), fmax / (fs/2)] (zpk -> zpk2sos), helpers.py:128 on [fmin, fmax] with
        # fs=Fs (SciPy then forms 2*f/fs): the same floating-point numbers (scaling by two is exact), so
        # the two SOS arrays are bit-identical (tests/test_host.py checks it) and ONE design serves both
        sos = signal.iirfilter(order, [fmin, fmax], btype='band', ftype='butter', fs=fs, output='sos')
        return sos, True, sos, nyquist
    if filter_type == 'cheby1':
        sos = signal.iirfilter(order, [fmin, fmax], rp=ripple, btype='band', analog=False,
                               ftype='cheby1', fs=fs, output='sos')
        return sos, False, sos, False
    raise ValueError('unknown FILTER_TYPE %r (expected "butter" or "cheby1")' % (filter_type,))


def _bandpass_sos_batch(filter_type, f_lo, f_hi, N, rp, fs):
    """SciPy's ``iirfilter(N, [lo, hi], rp, btype='band', ftype=..., fs=fs, output='sos')`` for MANY bands at
    once: the same floating-point operations (analog prototype -> ``lp2bp_zpk`` -> ``bilinear_zpk`` ->
    ``zpk2sos`` with 'nearest' pairing), element-wise over a (bands, poles) array instead of one Python call chain
    per band (0.14 ms per band in SciPy — 7 ms of host time per 48-band call).  Band-pass only (every pole complex,
    N zeros at +1 and N at -1).  -> (B, N, 6), or None if a band does not fit the assumptions (the caller then uses
    SciPy).  tests/test_host.py compares the result bit for bit with SciPy over orders 1..8, both filter types."""
    f_lo = np.asarray(f_lo, dtype=np.float64)
    f_hi = np.asarray(f_hi, dtype=np.float64)
    B = len(f_lo)
    Wn = np.stack((f_lo, f_hi), axis=1) / (fs / 2)
    if B == 0 or np.any(Wn <= 0) or np.any(Wn >= 1) or np.any(Wn[:, 0] >= Wn[:, 1]):
        return None
    m = np.arange(-N + 1, N, 2)
    if filter_type == 'butter':
        p0 = -np.exp(1j * np.pi * m / (2 * N))
        k0 = 1
    else:
        eps = np.sqrt(10 ** (0.1 * rp) - 1.0)
        mu = 1.0 / N * np.arcsinh(1 / eps)
        theta = np.pi * m / (2 * N)
        p0 = -np.sinh(mu + 1j * theta)
        k0 = np.prod(-p0, axis=0).real
        if N % 2 == 0:
            k0 = k0 / np.sqrt(1 + eps * eps)
    fs_ = 2.0
    warped = 2 * fs_ * np.tan(np.pi * Wn / fs_)
    bw = warped[:, 1] - warped[:, 0]
    wo = np.sqrt(warped[:, 0] * warped[:, 1])
    wo2 = np.array([float(x) ** 2 for x in wo])              # Python float powers, as in lp2bp_zpk
    kbp = np.array([k0 * float(x) ** N for x in bw])
    p_lp = (p0[None, :] * bw[:, None] / 2).astype(complex)
    root = np.sqrt(p_lp ** 2 - wo2[:, None])
    p_bp = np.concatenate((p_lp + root, p_lp - root), axis=1)          # (B, 2N)
    fs2 = 2.0 * fs_
    p_z = (fs2 + p_bp) / (fs2 - p_bp)
    # gain: k * real(prod(fs2 - z) / prod(fs2 - p)); the N analog zeros sit at the origin
    num = np.prod(fs2 - np.zeros(N, dtype=complex))
    den = np.prod(fs2 - p_bp, axis=1)                                   # left-to-right along the row, as on a 1-D array
    k_z = kbp * np.real(num / den)
    # zpk2sos, 'nearest': one member of every conjugate pair, in _cplxreal's order (by real part, then |imag|)
    tol = 100 * np.finfo(float).eps
    idx = np.lexsort((np.abs(p_z.imag), p_z.real), axis=1)
    pz = np.take_along_axis(p_z, idx, axis=1)
    if np.any(np.abs(pz.imag) <= tol * np.abs(pz)):
        return None                                                     # a real pole: not the band-pass structure assumed here
    up = pz.imag > 0
    if not np.all(up.sum(axis=1) == N):
        return None
    zp = pz[up].reshape(B, N)
    zn = pz[~up].reshape(B, N)
    if N > 1 and np.any(np.diff(zp.real, axis=1) <= tol * np.abs(zp[:, :-1])):
        return None                                                     # equal real parts: _cplxreal re-sorts such runs, leave it to SciPy
    pc = (zp + zn.conj()) / 2
    # sections are filled from the last one: the pole closest to the unit circle first (argmin with removal = a
    # stable ascending sort), each with its two nearest remaining zeros (all real: N at -1, N at +1)
    order = np.argsort(np.abs(1 - np.abs(pc)), axis=1, kind='stable')
    n_minus = np.full(B, N)
    n_plus = np.full(B, N)
    sos = np.zeros((B, N, 6))
    sos[:, :, 0] = 1.0
    sos[:, :, 3] = 1.0
    rows = np.arange(B)
    for kk in range(N):
        si = N - 1 - kk
        p1 = pc[rows, order[:, kk]]
        d_minus = np.abs(-1.0 - p1)
        d_plus = np.abs(1.0 - p1)
        if np.any(d_minus == d_plus):
            return None                                                 # a tie: argsort's pick is arbitrary, leave it to SciPy
        zz = []
        for _ in range(2):
            take_minus = (n_minus > 0) & ((d_minus < d_plus) | (n_plus == 0))
            zz.append(np.where(take_minus, -1.0, 1.0))
            n_minus = n_minus - take_minus
            n_plus = n_plus - (~take_minus)
        z1, z2 = zz
        pr, pi_ = p1.real, p1.imag
        sos[:, si, 1] = (-z2) + (-z1)                                   # np.poly([z1, z2]) by convolution
        sos[:, si, 2] = (-z1) * (-z2)
        sos[:, si, 4] = (-pr) + (-pr)                                   # np.poly([p1, conj(p1)]).real
        sos[:, si, 5] = pr * pr + pi_ * pi_
    sos[:, 0, :3] *= k_z[:, None]
    return sos


def design_bandpass_many(filter_type, edges, order, ripple, fs):
    """``design_bandpass`` for a list of (fmin, fmax): cached designs are reused, the others are designed in one
    vectorised pass (``_bandpass_sos_batch``) and entered into the same cache.  -> list of (applied sos, zero_phase,
    returned sos), exactly what ``design_bandpass`` returns band by band."""
    out = [None] * len(edges)
    todo = []
    for n, (fmin, fmax) in enumerate(edges):
        key = (filter_type, float(fmin), float(fmax), int(order), float(ripple), float(fs))
        hit = _batch_cache.get(key)
        if hit is not None:
            out[n] = (hit.copy(), filter_type == 'butter', hit.copy())
        else:
            todo.append((n, key))
    if todo and filter_type in ('butter', 'cheby1'):
        fe = 0.5 * fs
        ok = [t for t in todo if (filter_type != 'butter' or not (t[1][2] / fe - 1.0 > -1e-6))]
        batch = _bandpass_sos_batch(filter_type, [t[1][1] for t in ok], [t[1][2] for t in ok], int(order), float(ripple), float(fs)) if ok else None
        if batch is not None:
            for (n, key), sos in zip(ok, batch):
                if len(_batch_cache) > 8192:
                    _batch_cache.clear()
                _batch_cache[key] = sos
                out[n] = (sos.copy(), filter_type == 'butter', sos.copy())
    for n, (fmin, fmax) in enumerate(edges):
        if out[n] is None:              # Nyquist high-pass case, unusual pole structure, unknown type (raises): band by band
            out[n] = design_bandpass(filter_type, fmin, fmax, order, ripple, fs)
    return out


_batch_cache = {}


def design_cache_clear():
    """Forget cached filter designs (bench.py clears them before every timed call)."""
    _design_cached.cache_clear()
    _batch_cache.clear()


def pad_sections(sos_list):
    """Stack per-band SOS arrays to (B, Smax, 6), padding with identity sections."""
    smax = max(s.shape[0] for s in sos_list)
    out = np.zeros((len(sos_list), smax, 6))
    out[:, :, 0] = 1.0
    out[:, :, 3] = 1.0
    for b, s in enumerate(sos_list):
        out[b, :s.shape[0], :] = s
    return out


@functools.lru_cache(maxsize=8)
def _taper_ramps_cached(npts, max_percentage):
    wlen = min(int(max_percentage * npts), int(npts / 2))
    if wlen == 0:
        return np.zeros(0), np.zeros(0)
    sides = signal.windows.hann(2 * wlen if 2 * wlen == npts else 2 * wlen + 1)
    tl, tr = np.ascontiguousarray(sides[:wlen]), np.ascontiguousarray(sides[len(sides) - wlen:])
    tl.flags.writeable = False
    tr.flags.writeable = False
    return tl, tr


def taper_ramps(npts, max_percentage=TAPER_FRACTION):
    """Left and right ramps of obspy's Hann taper (ones in between are implicit).  A pure function of the trace
    length: kept for the last few lengths (read-only arrays)."""
    return _taper_ramps_cached(int(npts), float(max_percentage))


def window_plan(npts, fs, window_length, window_overlap):
    """(W, inc, number of windows): W = int(winlen*fs), inc = int(round((1-ov)*W)),
    windows start at arange(0, npts - W, inc)."""
    W = int(window_length * fs)
    inc = int(np.round((1 - window_overlap) * W))
    if W < 2 or inc < 1:
        raise ValueError('window length / overlap give an empty window or zero hop')
    nwin = max(0, -(-(int(npts) - W) // inc))          # = len(np.arange(0, npts - W, inc)), without building it
    return W, inc, nwin


def pair_table(nchans):
    return np.array([(i, j) for i in range(nchans - 1) for j in range(i + 1, nchans)], dtype=np.int32)


@functools.lru_cache(maxsize=8)
def _co_array_cached(shape, raw):
    out = _co_array(np.frombuffer(raw, dtype=np.float64).reshape(shape))
    for a in out:
        a.flags.writeable = False
    return out


def co_array(rij):
    """rij (2, N) km -> xij (P, 2) = r_i - r_j, pair table (P, 2), pinv(xij) (2, P).  A pure function of the
    coordinates: the last few geometries are kept (read-only arrays; ``functools.lru_cache``: safe under the host threads
    that drive several handles — the dict with manual eviction it replaces was not)."""
    rij = np.ascontiguousarray(rij, dtype=np.float64)
    return _co_array_cached(rij.shape, rij.tobytes())


def _co_array(rij):
    idx = pair_table(rij.shape[1])
    xij = np.ascontiguousarray((rij[:, idx[:, 0]] - rij[:, idx[:, 1]]).T)
    if np.linalg.matrix_rank(xij) < LTS_DIM:
        raise RuntimeError('Co-array is ill posed for the least squares problem. Check array coordinates.')
    return xij, idx, np.ascontiguousarray(np.linalg.pinv(xij))


def lts_h(P, alpha, p=LTS_DIM):
    n2 = (P + p + 1) // 2
    return int(math.floor(2 * n2 - P + 2 * (P - n2) * alpha))


@functools.lru_cache(maxsize=64)
def _uniran_cached(P, n_samples, p):
    seed = 0
    out = np.empty((n_samples, p), dtype=np.int64)
    for s in range(n_samples):
        chosen = []
        for _ in range(p):
            while True:
                seed = (seed * 5761 + 999) % 65536
                num = int(math.floor(seed / 65536.0 * P))
                if num not in chosen:
                    break
            chosen.append(num)
        out[s] = chosen
    out.flags.writeable = False
    return out


def uniran_subsets(P, n_samples=LTS_N_SAMPLES, p=LTS_DIM):
    """robustbase LCG (seed*5761+999 mod 65536), seed 0, carried across subsets.  A pure function of
    the pair count (the sequence is generated once per P and kept)."""
    return _uniran_cached(int(P), int(n_samples), int(p)).copy()


@functools.lru_cache(maxsize=64)
def _all_pairs(P):
    out = np.array([(i, j) for i in range(P - 1) for j in range(i + 1, P)], dtype=np.int64)
    out.flags.writeable = False
    return out


def lts_starts(xs):
    """Elemental starts on the standardised co-array: every 2-subset if there are at most
    LTS_N_SAMPLES of them, else LTS_N_SAMPLES LCG-random ones; rank-deficient subsets are
    extended until they have rank 2.  (S, 4) int32, -1 padded."""
    P = xs.shape[0]
    if P * (P - 1) // 2 <= LTS_N_SAMPLES:
        subs = _all_pairs(int(P))
    else:
        subs = uniran_subsets(P)
    out = -np.ones((len(subs), 4), dtype=np.int32)
    out[:, :2] = subs
    scale = np.max(np.abs(xs)) ** 2
    # Gram determinant of every 2-subset at once; only the (rare) rank-deficient ones take the repair loop
    a, b = xs[subs[:, 0]], xs[subs[:, 1]]
    g00 = a[:, 0] * a[:, 0] + b[:, 0] * b[:, 0]
    g01 = a[:, 0] * a[:, 1] + b[:, 0] * b[:, 1]
    g11 = a[:, 1] * a[:, 1] + b[:, 1] * b[:, 1]
    suspect = np.nonzero(~(g00 * g11 - g01 * g01 > 1e-9 * scale * scale))[0]      # generous margin over the 1e-12 test below
    for s in suspect.tolist():
        sub = list(subs[s])
        nxt = 0
        while True:
            g = xs[sub].T @ xs[sub]
            det = g[0, 0] * g[1, 1] - g[0, 1] * g[1, 0]
            if det > 1e-12 * scale * scale or len(sub) >= 4:
                break
            while nxt in sub:
                nxt += 1
            if nxt >= P:
                break
            sub.append(nxt)
        out[s, :len(sub)] = sub
    return out


def _consfactor(m, n):
    if m >= n or m <= 0:
        return 1.0
    q = norm.ppf((m + n) / (2.0 * n))
    return 1.0 / math.sqrt(1.0 - (2.0 * n) / (m / q) * norm.pdf(q))


def _consfactor_table(n):
    """_consfactor(m, n) for m = 1..n-1 in one vectorised pass (same IEEE operations per element)."""
    m = np.arange(1, n, dtype=np.float64)
    q = norm.ppf((m + n) / (2.0 * n))
    return 1.0 / np.sqrt(1.0 - (2.0 * n) / (m / q) * norm.pdf(q))


def _cnp2(p, n, alpha, c500, c875):
    c500 = np.asarray(c500, dtype=float)
    c875 = np.asarray(c875, dtype=float)
    y500 = np.log(-c500[0] / p ** c500[1])
    y875 = np.log(-c875[0] / p ** c875[1])
    k500 = np.linalg.solve(np.column_stack((np.ones(2), -np.log(c500[2] * p ** 2))), y500)
    k875 = np.linalg.solve(np.column_stack((np.ones(2), -np.log(c875[2] * p ** 2))), y875)
    fp500 = 1 - math.exp(k500[0]) / n ** k500[1]
    fp875 = 1 - math.exp(k875[0]) / n ** k875[1]
    if alpha <= 0.875:
        fp = fp500 + (fp875 - fp500) / 0.375 * (alpha - 0.5)
    else:
        fp = fp875 + (1 - fp875) / 0.125 * (alpha - 0.875)
    return 1.0 / fp


# robustbase LTScnp2 / LTScnp2.rew coefficient tables, no-intercept, p >= 2 [R]
_RAW_500 = [[-0.487338281979106, -0.340762058011], [0.405511279418594, 0.37972360544988], [3, 5]]
_RAW_875 = [[-0.251778730491252, -0.146660023184295], [0.883966931611758, 0.86292940340761], [3, 5]]
_REW_500 = [[-0.417574780492848, -0.175753709374146], [1.83958876341367, 1.8313809497999], [3, 5]]
_REW_875 = [[-0.267522855927958, -0.161200683014406], [1.17559984533974, 1.21675019853961], [3, 5]]


@functools.lru_cache(maxsize=64)
def _lts_factors(P, alpha):
    """Consistency and small-sample factors of the raw and the reweighted scale: pure functions of the pair count and
    alpha (like the LCG subsets above), computed once per (P, alpha) and kept."""
    h = lts_h(P, alpha)
    raw = _consfactor(h, P) * _cnp2(LTS_DIM, P, alpha, _RAW_500, _RAW_875)
    rew = np.ones(P + 1)
    cor = _cnp2(LTS_DIM, P, alpha, _REW_500, _REW_875)
    rew[1:P] = _consfactor_table(P) * cor
    rew.flags.writeable = False
    return raw, rew


def lts_plan(xij, alpha):
    """Everything the LTS kernel needs besides the lags (see ``nbls_lts_params``)."""
    if not (0.5 <= alpha < 1.0):
        raise ValueError('LTS needs 0.5 <= ALPHA < 1.0')
    P = xij.shape[0]
    h = lts_h(P, alpha)
    xij_mad = MAD_CONST * np.median(np.abs(xij), axis=0)
    if not np.all(xij_mad > 0):
        raise RuntimeError('Co-array MAD is zero along an axis; cannot standardise for LTS.')
    starts = lts_starts(xij / xij_mad)
    raw, rew = _lts_factors(int(P), float(alpha))
    rew = rew.copy()
    return dict(alpha=alpha, h=h, starts=starts, csteps=LTS_CSTEPS, csteps2=LTS_CSTEPS2,
                ncand=LTS_CANDIDATES, xij_mad=xij_mad, raw_factor=raw, rew_table=rew,
                quantile=LTS_QUANTILE, zero_scale=LTS_ZERO_SCALE)


def sosfreqz_bands(sos_list, worN, fs):
    """``scipy.signal.sosfreqz(sos, worN, fs=fs)`` for every band of a call (narrow_band_least_squares.py:78-80) ->
    (w (F,), h rows (B, F) complex).  The same NumPy operations in the same order on arrays of the same shape as
    SciPy's ``freqz_sos`` -> ``freqz`` -> ``numpy.polynomial.polynomial.polyval`` chain (``zm1 = exp(-1j w)``; Horner in
    ``zm1`` per section; ``h *= num / den``), so every value has SciPy's bits — but ``zm1`` is computed once per call
    instead of once per section and band, and the per-call argument checks are gone (48 bands: 2.7 -> 1.2 ms).
    Falls back to SciPy for anything but an array of frequencies and (S, 6) float sections."""
    if worN is None or np.ndim(worN) == 0:          # a point count (or SciPy's default): its own branches
        return None
    w_in = np.atleast_1d(worN)
    if w_in.ndim != 1 or w_in.dtype.kind not in 'fiu' or not (np.isscalar(fs) and fs > 0):
        return None
    w = 2 * np.pi * w_in / fs
    zm1 = np.exp(-1j * w)
    x0 = zm1 * 0
    rows = np.empty((len(sos_list), len(w)), dtype=complex)
    for n, sos in enumerate(sos_list):
        sos = np.asarray(sos)
        if sos.ndim != 2 or sos.shape[1] != 6 or sos.shape[0] == 0 or sos.dtype != np.float64:
            return None
        h = 1.
        for row in sos:
            num = row[2] + x0
            num = row[1] + num * zm1
            num = row[0] + num * zm1
            den = row[5] + x0
            den = row[4] + den * zm1
            den = row[3] + den * zm1
            h *= num / den
        rows[n] = h
    return w * (fs / (2 * np.pi)), rows


def uncertainty_frame(xij):
    """(lambda_0, lambda_1, R00, R01, R10, R11): eigenvalues (ascending, ``numpy.linalg.eigh``) of X^T X of the co-array
    and the rotation into its eigen-frame as lts_array builds it [R: source absent] — ``ang = arccos(evecs[0, 0])``,
    ``R = [[cos, sin], [-sin, cos]]`` — for the confidence intervals the GPU computes behind the solve
    (``nbls_set_uncertainty``; 7th / 8th returns of ``ltsva``, narrow_band_least_squares.py:91)."""
    xij = np.asarray(xij, dtype=np.float64)
    evals, evecs = np.linalg.eigh(xij.T @ xij)
    ang = np.arccos(np.clip(evecs[0, 0], -1.0, 1.0))
    return np.array([evals[0], evals[1], np.cos(ang), np.sin(ang), -np.sin(ang), np.cos(ang)])


def check_min_velocity(min_velocity):
    """``min_velocity`` (km/s) of the bounded lag search -> float; ``ValueError`` unless it is a finite real > 0 (not a bool)."""
    if isinstance(min_velocity, (bool, np.bool_)) or not isinstance(min_velocity, (int, float, np.integer, np.floating)):
        raise ValueError('min_velocity must be a finite number of km/s above 0, not %r' % (min_velocity,))
    v = float(min_velocity)
    if not np.isfinite(v) or v <= 0.0:
        raise ValueError('min_velocity must be a finite number of km/s above 0, not %r' % (min_velocity,))
    return v


MAX_GRID_POINTS = 65536      # grid points of one slowness-grid search (NBLS_BEAM_GRID_MAX)


def slowness_grid(max_slowness, n):
    """The ``n`` x ``n`` Cartesian grid of slowness vectors over ``+-max_slowness`` s/km (``n`` odd, so s = 0 is a point;
    ``numpy.meshgrid(..., indexing='ij')`` order), the points with ``|s| > max_slowness`` dropped -> (G, 2) float64, the
    table ``ltsva_grid`` and ``nbls_set_beam_grid`` take.  ``slowness_grid(4.0, 41)`` has 1257 points."""
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)) or n < 1 or n % 2 == 0:
        raise ValueError('n must be an odd number of grid points per axis, not %r' % (n,))
    s = float(max_slowness)
    if not np.isfinite(s) or s <= 0.0:
        raise ValueError('max_slowness must be a finite number of s/km above 0, not %r' % (max_slowness,))
    ax = np.linspace(-s, s, int(n)) if n > 1 else np.zeros(1)           # (one point per axis: the centre)
    g0, g1 = np.meshgrid(ax, ax, indexing='ij')
    grid = np.stack([g0.ravel(), g1.ravel()], axis=1)
    return np.ascontiguousarray(grid[np.hypot(grid[:, 0], grid[:, 1]) <= s])


def check_slowness_grid(grid):
    """``slowness_grid`` of the grid search -> C-contiguous (G, 2) float64; ``ValueError`` (before any GPU work) unless it
    is a real array of that shape with 1 <= G <= ``MAX_GRID_POINTS`` and finite entries."""
    try:
        g = np.asarray(grid)
    except Exception:
        raise ValueError('slowness_grid must be a (G, 2) array of slowness vectors in s/km')
    if g.dtype == object or g.dtype.kind not in 'iuf':
        raise ValueError('slowness_grid must hold real numbers (s/km), not dtype %s' % g.dtype)
    if g.ndim != 2 or g.shape[1] != 2:
        raise ValueError('slowness_grid must be (G, 2), not %r' % (g.shape,))
    if not (1 <= g.shape[0] <= MAX_GRID_POINTS):
        raise ValueError('slowness_grid has %d points: 1 to %d are supported' % (g.shape[0], MAX_GRID_POINTS))
    g = np.ascontiguousarray(g, dtype=np.float64)
    if not np.all(np.isfinite(g)):
        raise ValueError('slowness_grid holds entries that are not finite')
    return g


STEER_TAPS = (4, 6, 8)    # Lagrange taps of the fractional-sample steering (nbls_set_beam_interpolation); 0 switches it off


def check_steering(taps):
    """``taps`` of the fractional-sample steering (``nbls_set_beam_interpolation``) -> int;
    ``ValueError`` (before any GPU work) unless it is the integer 0 (off), 4, 6 or 8."""
    if isinstance(taps, (bool, np.bool_)) or not isinstance(taps, (int, np.integer)) or int(taps) not in (0,) + STEER_TAPS:
        raise ValueError('taps must be 0 (whole-sample delays), 4, 6 or 8, not %r' % (taps,))
    return int(taps)


def steering_coefficients(taps, mu):
    """The Lagrange coefficients ``c_k(mu)``, k = -K+1 .. K, K = taps / 2, of the fractional delay ``mu`` in [0, 1) ->
    (..., taps) float64, in the operation order of the library (csrc/steer.h): the factors ``mu - j`` multiplied for j
    ascending without k, one division by ``D_k = prod_{j != k} (k - j)``."""
    taps = check_steering(taps)
    if not taps:
        raise ValueError('taps must be 4, 6 or 8')
    mu = np.asarray(mu, dtype=np.float64)
    K = taps // 2
    out = np.empty(mu.shape + (taps,))
    for k in range(-K + 1, K + 1):
        p, D = np.ones_like(mu), 1
        for j in range(-K + 1, K + 1):
            if j != k:
                p = p * (mu - np.float64(j))
                D *= k - j
        out[..., k + K - 1] = p / np.float64(D)
    return out


def steering_error(taps, f_over_fs):
    """Worst-case error of the ``taps``-point Lagrange interpolator on a unit sinusoid of frequency ``f_over_fs`` cycles per
    sample: ``max_mu |sum_k c_k(mu) exp(2 pi i f/fs (k - mu)) - 1|`` over the 101 values mu = 0, 0.01, ..., 1 (DESIGN.md
    section 22 has the table: 8 taps stay below 2.4e-5 up to a tenth of the sampling rate)."""
    taps = check_steering(taps)
    if not taps:
        raise ValueError('taps must be 4, 6 or 8')
    K = taps // 2
    mu = np.arange(101) / 100.0
    c = steering_coefficients(taps, mu)
    k = np.arange(-K + 1, K + 1)
    h = np.sum(c * np.exp(2j * np.pi * float(f_over_fs) * (k[None, :] - mu[:, None])), axis=1)
    return float(np.max(np.abs(h - 1.0)))


def seed_halfwidths(fmax_list, fs, period_fraction=0.5):
    """Per-band half-widths of the seeded lag search (``nbls_set_lag_seed``) -> int32 (nbands,):
    ``K_b = max(1, int(floor(period_fraction * fs / fmax_b)))`` samples — by default half a period of the band's upper edge,
    so that the neighbouring cycle, one period away from the delay the grid maximum predicts, stays outside the range
    (18 samples for 1.1 Hz at 40 Hz).  ``ValueError`` unless every ``fmax_b`` and ``fs`` is a finite real > 0 and
    ``period_fraction`` a finite real in (0, 1]."""
    def real(v):
        return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))
    if not real(fs) or not np.isfinite(float(fs)) or float(fs) <= 0.0:
        raise ValueError('fs must be a finite sampling rate in Hz above 0, not %r' % (fs,))
    if not real(period_fraction) or not (0.0 < float(period_fraction) <= 1.0):
        raise ValueError('period_fraction must be a number in (0, 1], not %r' % (period_fraction,))
    try:
        f = np.asarray(fmax_list)
    except Exception:
        raise ValueError('fmax_list must be a list of upper band edges in Hz')
    if f.dtype == object or f.dtype.kind not in 'iuf' or f.ndim != 1 or f.size < 1:
        raise ValueError('fmax_list must be a non-empty list of upper band edges in Hz, not %r' % (fmax_list,))
    f = f.astype(np.float64)
    if not np.all(np.isfinite(f)) or np.any(f <= 0.0):
        raise ValueError('fmax_list must hold finite frequencies above 0 Hz')
    K = np.floor(float(period_fraction) * float(fs) / f)
    return np.maximum(1.0, np.minimum(K, 2.0 ** 31 - 1)).astype(np.int32)


def check_seed_halfwidths(halfwidth, nbands):
    """``halfwidth`` of the seeded lag search (samples; one integer for every band, or ``nbands`` of them) -> int32
    (nbands,); ``ValueError`` (before any GPU work) unless the entries are integers in 0 .. 2^31-1 and their number fits."""
    try:
        k = np.asarray(halfwidth)
    except Exception:
        raise ValueError('halfwidth must be an integer number of samples or one per band')
    if k.dtype == object or k.dtype.kind not in 'iu' or k.ndim > 1:
        raise ValueError('halfwidth must be an integer number of samples (or one per band), not %r' % (halfwidth,))
    k = np.atleast_1d(k).astype(np.int64)
    if k.size == 1 and nbands > 1:
        k = np.repeat(k, nbands)
    if k.size != nbands:
        raise ValueError('halfwidth has %d entries for %d bands' % (k.size, nbands))
    if np.any(k < 0) or np.any(k > 2 ** 31 - 1):
        raise ValueError('halfwidth must be 0 .. 2^31-1 samples, not %r' % (halfwidth,))
    return np.ascontiguousarray(k, dtype=np.int32)


def lag_limits(xij, fs, min_velocity):
    """Per-pair lag limits of the bounded search (``nbls_set_lag_limits``) -> int32 (P,):
    ``L_k = int(ceil(fs * hypot(xij[k, 0], xij[k, 1]) / min_velocity)) + 1`` samples — the delay a plane wave no slower
    than ``min_velocity`` km/s can put between the two elements of pair k, plus one sample of guard for the lag's own
    quantisation.  A sub-array needs no table of its own: its pairs are a subset of the full array's with the same ``xij``."""
    v = check_min_velocity(min_velocity)
    xij = np.asarray(xij, dtype=np.float64)
    L = np.ceil(float(fs) * np.hypot(xij[:, 0], xij[:, 1]) / v) + 1.0
    return np.minimum(L, 2.0 ** 31 - 1).astype(np.int32)


MAX_CAPON_ELEMENTS = 32      # array elements of a plan with Capon spectra (NBLS_CAPON_MAX_ELEMENTS)
MAX_CAPON_STEER_BYTES = 1 << 30      # the steering table nbands * G * N * 16 bytes of one plan


def _real(v):
    return not isinstance(v, (bool, np.bool_)) and isinstance(v, (int, float, np.integer, np.floating))


def capon_frequencies(band_edges):
    """The frequency at which the Capon spectra of every band are formed (``nbls_set_capon``) ->
    float64 (nbands,): the geometric centre ``sqrt(f_lo * f_hi)`` of the band.  ``ValueError`` unless every edge is a finite
    real > 0."""
    try:
        e = np.asarray(band_edges, dtype=np.float64)
    except Exception:
        raise ValueError('band_edges must be a list of (f_lo, f_hi) in Hz')
    if e.ndim != 2 or e.shape[1] != 2 or e.shape[0] < 1:
        raise ValueError('band_edges must be a non-empty list of (f_lo, f_hi) in Hz, not %r' % (band_edges,))
    if not np.all(np.isfinite(e)) or np.any(e <= 0.0):
        raise ValueError('band_edges must hold finite frequencies above 0 Hz')
    return np.sqrt(e[:, 0] * e[:, 1])


def capon_snapshots(xij, grid, fs, freqs, W_list):
    """Per-band snapshot length and hop of the Capon spectra -> (Ls int32 (nbands,), Hs int32 (nbands,)):
    ``Ls = min(W, max(ceil(2 fs / f), ceil(2 fs tau_max)))`` samples, ``tau_max`` the largest ``|xij[i-1] . s_g|`` over the
    pairs (0, i) and the grid — the narrow-band condition: the snapshot's frequency bin (two bins of the Hann taper, 2 fs / Ls)
    must be narrower than ``1 / tau_max``, and hold two periods — and ``Hs = max(1, Ls // 2)``, the half overlap of a Hann
    taper.  ``xij`` is the co-array (``co_array``), whose first N-1 rows are the pairs (0, i)."""
    g = check_slowness_grid(grid)
    xij = np.asarray(xij, dtype=np.float64)
    f = np.atleast_1d(np.asarray(freqs, dtype=np.float64))
    W = np.atleast_1d(np.asarray(W_list)).astype(np.int64)
    if f.shape != W.shape:
        raise ValueError('one window length per frequency')
    if not _real(fs) or not np.isfinite(float(fs)) or float(fs) <= 0.0:
        raise ValueError('fs must be a finite sampling rate in Hz above 0, not %r' % (fs,))
    if not np.all(np.isfinite(f)) or np.any(f <= 0.0):
        raise ValueError('freqs must hold finite frequencies above 0 Hz')
    N = int(round((1.0 + math.sqrt(1.0 + 8.0 * len(xij))) / 2.0))
    tau_max = float(np.abs(xij[:N - 1] @ g.T).max()) if N > 1 else 0.0
    Ls = np.maximum(np.ceil(2.0 * float(fs) / f), math.ceil(2.0 * float(fs) * tau_max))
    Ls = np.maximum(1, np.minimum(W, Ls)).astype(np.int32)
    return Ls, np.maximum(1, Ls // 2).astype(np.int32)


def check_capon(nchans, grid, freqs, snapshots, loading, W_list, maps=False, csdm=False):
    """Everything ``nbls_set_capon`` and the plan behind it refuse, as ``ValueError`` before any GPU work -> (grid (G, 2)
    float64, freqs float64 (nbands,), Ls int32, Hs int32, loading float).  ``snapshots``: (Ls, Hs), each one integer or one
    per band; ``W_list``: the window length of every band in samples."""
    g = check_slowness_grid(grid)
    for name, v in (('maps', maps), ('csdm', csdm)):
        if not isinstance(v, (bool, np.bool_)):
            raise ValueError('%s must be True or False, not %r' % (name, v))
    W = np.atleast_1d(np.asarray(W_list)).astype(np.int64)
    nb = len(W)
    try:
        f = np.atleast_1d(np.asarray(freqs))
    except Exception:
        raise ValueError('capon_freqs must be one frequency in Hz per band')
    if f.dtype == object or f.dtype.kind not in 'iuf' or f.ndim != 1:
        raise ValueError('capon_freqs must be one frequency in Hz per band, not %r' % (freqs,))
    f = f.astype(np.float64)
    if len(f) != nb:
        raise ValueError('capon_freqs has %d entries for %d bands' % (len(f), nb))
    if not np.all(np.isfinite(f)) or np.any(f <= 0.0):
        raise ValueError('capon_freqs must hold finite frequencies above 0 Hz')
    try:
        ls, hs = snapshots
        ls, hs = np.asarray(ls), np.asarray(hs)
    except Exception:
        raise ValueError('capon_snapshots must be (lengths, hops) in samples')
    out = []
    for name, v in (('length', ls), ('hop', hs)):
        if v.dtype == object or v.dtype.kind not in 'iu' or v.ndim > 1:
            raise ValueError('the snapshot %s must be an integer number of samples (or one per band), not %r' % (name, v))
        v = np.atleast_1d(v).astype(np.int64)
        if v.size == 1 and nb > 1:
            v = np.repeat(v, nb)
        if v.size != nb:
            raise ValueError('the snapshot %s has %d entries for %d bands' % (name, v.size, nb))
        if np.any(v < 1) or np.any(v > 2 ** 31 - 1):
            raise ValueError('the snapshot %s must be at least 1 sample' % name)
        out.append(v)
    ls, hs = out
    if np.any(ls > W):
        raise ValueError('a snapshot of %d samples is longer than its window of %d' % (int(ls[np.argmax(ls > W)]), int(W[np.argmax(ls > W)])))
    if not _real(loading) or not np.isfinite(float(loading)) or float(loading) < 0.0:
        raise ValueError('the loading must be a finite number that is not negative, not %r' % (loading,))
    if not (3 <= int(nchans) <= MAX_CAPON_ELEMENTS):
        raise ValueError('%d array elements: the Capon spectra support 3 to %d' % (nchans, MAX_CAPON_ELEMENTS))
    K = 1 + (W - ls) // hs
    if float(loading) == 0.0 and np.any(K < nchans):
        raise ValueError('loading 0 with %d snapshots of %d elements: the matrix is singular by construction' % (int(K.min()), nchans))
    if nb * len(g) * int(nchans) * 16 > MAX_CAPON_STEER_BYTES:
        raise ValueError('the steering table of %d bands x %d grid points x %d elements exceeds 1 GiB' % (nb, len(g), nchans))
    return g, f, ls.astype(np.int32), hs.astype(np.int32), float(loading)


MAX_CAPON_PEAKS = 8          # ranks of a peak request (NBLS_CAPON_PEAKS_MAX)
MAX_CAPON_CELL = 32768       # lattice coordinates of a peak request lie below this


def grid_cells(grid):
    """The lattice coordinates of a slowness grid, as a peak request takes them (``nbls_set_capon_peaks``, DESIGN.md section
    19) -> (cells int32 (G, 2), steps float64 (2,)).  Per axis the step is the smallest positive difference between distinct
    coordinates (values within 1e-9 of the axis' span count as equal; an axis with one value has step 0 and cells 0) and
    ``cell = rint((v - min) / step)``.  ``ValueError`` if a point lies more than 1e-6 step off its lattice point, if two points
    share a cell, or if a coordinate reaches 32768.  ``grid_cells(slowness_grid(s, n))`` gives the meshgrid indices."""
    g = check_slowness_grid(grid)
    cells = np.zeros(g.shape, dtype=np.int64)
    steps = np.zeros(2)
    for ax in (0, 1):
        v = g[:, ax]
        u = np.unique(v)
        d = np.diff(u)
        d = d[d > 1e-9 * (u[-1] - u[0])] if len(u) > 1 else d
        if len(d) == 0:
            continue
        steps[ax] = d.min()
        q = (v - u[0]) / steps[ax]
        c = np.rint(q)
        if np.any(np.abs(q - c) > 1e-6):
            raise ValueError('slowness_grid is no lattice on axis %d: point %d lies %.3g steps off its lattice point'
                             % (ax, int(np.argmax(np.abs(q - c))), float(np.abs(q - c).max())))
        if c.max() >= MAX_CAPON_CELL:
            raise ValueError('slowness_grid spans %d lattice steps on axis %d: fewer than %d are supported'
                             % (int(c.max()), ax, MAX_CAPON_CELL))
        cells[:, ax] = c.astype(np.int64)
    if len(np.unique(cells[:, 0] * MAX_CAPON_CELL + cells[:, 1])) != len(cells):
        raise ValueError('two points of slowness_grid share one lattice cell')
    return np.ascontiguousarray(cells, dtype=np.int32), steps


MAX_GRID_REFINE_LEVELS = 12      # NBLS_BEAM_GRID_REFINE_MAX_LEVELS


def check_grid_refinement(levels, step, grid, taps, has_seed=False):
    """Everything ``nbls_set_beam_grid_refinement`` and the plan behind it refuse, as ``ValueError`` before any GPU work ->
    (levels int, step float64 (2,)).  ``levels``: an integer in 1..12; ``step``: (h0, h1) s/km, finite and > 0, or None: the
    lattice step of ``grid`` (``grid_cells(grid)[1]``; ``ValueError`` where an axis of the grid has a single value); ``grid``:
    the slowness grid of the call (None: there is none); ``taps``: its steering, which must be 4, 6 or 8 — the whole-sample
    F is piecewise constant in the slowness —; ``has_seed``: the call seeds its lag search by the grid maximum, which does not
    combine."""
    if isinstance(levels, (bool, np.bool_)) or not isinstance(levels, (int, np.integer)) or not (1 <= int(levels) <= MAX_GRID_REFINE_LEVELS):
        raise ValueError('the refinement levels must be an integer in 1..%d, not %r' % (MAX_GRID_REFINE_LEVELS, levels))
    if grid is None:
        raise ValueError('the refinement of the grid maximum needs slowness_grid')
    if check_steering(taps) == 0:
        raise ValueError('the refinement of the grid maximum needs fractional-sample steering (taps 4, 6 or 8): with whole-sample '
                         'delays F is piecewise constant in the slowness')
    if has_seed:
        raise ValueError('the refinement of the grid maximum does not combine with the seeded lag search: the seed keeps the '
                         'unrefined maximum')
    if step is None:
        step = grid_cells(grid)[1]
        if not np.all(step > 0.0):
            raise ValueError('slowness_grid has a single value on axis %d: it has no lattice step there, give step=(h0, h1)'
                             % int(np.argmin(step)))
    try:
        s = np.array(step, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('the refinement step must be two numbers (h0, h1) in s/km, not %r' % (step,))
    if s.shape != (2,) or not np.all(np.isfinite(s)) or not np.all(s > 0.0):
        raise ValueError('the refinement step must be two finite numbers > 0 (h0, h1) in s/km, not %r' % (step,))
    return int(levels), s


def check_capon_peaks(grid_len, cells, K, floor):
    """Everything ``nbls_set_capon_peaks`` and the plan behind it refuse, as ``ValueError`` before any GPU work -> (cells int32
    (G, 2), K int, floor float).  ``grid_len``: the G of the Capon spectra the request goes with."""
    if isinstance(K, (bool, np.bool_)) or not isinstance(K, (int, np.integer)) or not (1 <= int(K) <= MAX_CAPON_PEAKS):
        raise ValueError('the number of peaks must be an integer in 1..%d, not %r' % (MAX_CAPON_PEAKS, K))
    if not _real(floor) or not (0.0 <= float(floor) <= 1.0):
        raise ValueError('the peak floor must be a number in [0, 1], not %r' % (floor,))
    try:
        c = np.asarray(cells)
    except Exception:
        raise ValueError('the cells must be a (G, 2) array of lattice coordinates')
    if c.dtype == object or c.dtype.kind not in 'iu':
        raise ValueError('the cells must hold integers, not dtype %s' % c.dtype)
    if c.ndim != 2 or c.shape[1] != 2:
        raise ValueError('the cells must be (G, 2), not %r' % (c.shape,))
    if c.shape[0] != int(grid_len):
        raise ValueError('%d cells for Capon spectra of %d grid points' % (c.shape[0], int(grid_len)))
    c = c.astype(np.int64)
    if np.any(c < 0) or np.any(c >= MAX_CAPON_CELL):
        raise ValueError('the cells must lie in 0..%d' % (MAX_CAPON_CELL - 1))
    if len(np.unique(c[:, 0] * MAX_CAPON_CELL + c[:, 1])) != len(c):
        raise ValueError('two points share one lattice cell')
    return np.ascontiguousarray(c, dtype=np.int32), int(K), float(floor)


MAX_CAPON_CLEAN = 32      # iterations of a CLEAN request (NBLS_CAPON_CLEAN_MAX)


def check_capon_clean(iterations, gain=0.5, floor=0.02, residual=False, has_capon=True):
    """Everything ``nbls_set_capon_clean`` and the plan behind it refuse, as ``ValueError`` before any GPU work -> (iterations
    int, gain float, floor float, residual bool): an integer number of iterations in 1..32, a gain in (0, 1], a floor in
    [0, 1), ``residual`` a bool; ``has_capon``: the call computes the Capon spectra the request works on."""
    if isinstance(iterations, (bool, np.bool_)) or not isinstance(iterations, (int, np.integer)) or not (1 <= int(iterations) <= MAX_CAPON_CLEAN):
        raise ValueError('the CLEAN iterations must be an integer in 1..%d, not %r' % (MAX_CAPON_CLEAN, iterations))
    if not _real(gain) or not (0.0 < float(gain) <= 1.0):
        raise ValueError('the CLEAN gain must be a number in (0, 1], not %r' % (gain,))
    if not _real(floor) or not (0.0 <= float(floor) < 1.0):
        raise ValueError('the CLEAN floor must be a number in [0, 1), not %r' % (floor,))
    if not isinstance(residual, (bool, np.bool_)):
        raise ValueError('residual must be True or False, not %r' % (residual,))
    if not has_capon:
        raise ValueError('a CLEAN request needs the Capon spectra (capon_grid)')
    return int(iterations), float(gain), float(floor), bool(residual)


def check_capon_music(nchans, sources=0, eig_floor=0.05, maps=False, vectors=False, peaks=False, peak_floor=0.0, has_capon=True,
                      has_peaks=True, kept_capon=False, estimators=False, comm=False, segmented=False):
    """Everything ``nbls_set_capon_music`` and the plan behind it refuse, as ``ValueError`` before any GPU work -> (sources int,
    eig_floor float, maps bool, vectors bool, peaks bool, peak_floor float): an array of 3..32 elements, an integer ``sources`` in 0..nchans-1 (0: by the
    floor), with ``sources=0`` an ``eig_floor`` in (0, 1), ``maps``, ``vectors`` and ``peaks`` bools, a ``peak_floor`` in [0, 1);
    ``has_capon``: the call computes the Capon spectra the request works on; ``has_peaks``: and their peaks, whose K and cells
    ``peaks`` uses; ``kept_capon``, ``estimators``, ``comm``, ``segmented``: the call also asks for the
    spectra of the kept elements, further estimators, an RCCL communicator or the time-segmented path, none of which a MUSIC
    request combines with."""
    if isinstance(nchans, (bool, np.bool_)) or not isinstance(nchans, (int, np.integer)) or not (3 <= int(nchans) <= MAX_CAPON_ELEMENTS):
        raise ValueError('a MUSIC request needs an array of 3..%d elements, not %r' % (MAX_CAPON_ELEMENTS, nchans))
    if isinstance(sources, (bool, np.bool_)) or not isinstance(sources, (int, np.integer)) or not (0 <= int(sources) <= int(nchans) - 1):
        raise ValueError('the MUSIC sources must be an integer in 0..%d (0: by eig_floor), not %r' % (int(nchans) - 1, sources))
    if not _real(eig_floor) or (int(sources) == 0 and not (0.0 < float(eig_floor) < 1.0)):
        raise ValueError('the MUSIC eig_floor must be a number in (0, 1), not %r' % (eig_floor,))
    for name, flag in (('maps', maps), ('vectors', vectors), ('peaks', peaks)):
        if not isinstance(flag, (bool, np.bool_)):
            raise ValueError('%s must be True or False, not %r' % (name, flag))
    if not _real(peak_floor) or not (0.0 <= float(peak_floor) < 1.0):
        raise ValueError('the MUSIC peak_floor must be a number in [0, 1), not %r' % (peak_floor,))
    if not has_capon:
        raise ValueError('a MUSIC request needs the Capon spectra (capon_grid)')
    if peaks and not has_peaks:
        raise ValueError('the peaks of a MUSIC request need K and the cells of a peak request (capon_peaks, capon_cells)')
    if kept_capon:
        raise ValueError('a MUSIC request works on the full array: not with the Capon spectra of the kept elements')
    if estimators:
        raise ValueError('a MUSIC request is not supported with further estimators')
    if comm:
        raise ValueError('a MUSIC request is not supported with an RCCL communicator')
    if segmented:
        raise ValueError('a MUSIC request is not supported on the time-segmented path')
    return int(sources), float(eig_floor), bool(maps), bool(vectors), bool(peaks), float(peak_floor)


MAX_KEPT_ELEMENTS = 32    # elements of a plan that names the dropped ones: one bit each of a uint32 (csrc/kept.hip)


def check_kept(nchans, min_pairs=None, beam=True, capon=False):
    """Everything ``nbls_set_kept_elements`` and the plan behind it refuse, as ``ValueError`` before any GPU work -> (min_pairs
    int, beam bool, capon bool).  ``nchans``: the elements N of the array; ``min_pairs`` q: an element counts as dropped by
    LTS when at least q of its N - 1 pairs have lost their weight, None: N - 1, all of them.  ``beam`` /
    ``capon``: the beam results / the Capon spectra are formed over the kept elements."""
    if isinstance(nchans, (bool, np.bool_)) or not isinstance(nchans, (int, np.integer)):
        raise ValueError('the element count must be an integer, not %r' % (nchans,))
    n = int(nchans)
    if n < 3 or n > MAX_KEPT_ELEMENTS:
        raise ValueError('%d array elements: the kept elements are worked out for 3..%d' % (n, MAX_KEPT_ELEMENTS))
    for name, flag in (('beam', beam), ('capon', capon)):
        if not isinstance(flag, (bool, np.bool_)):
            raise ValueError('%s must be True or False, not %r' % (name, flag))
    if min_pairs is None:
        min_pairs = n - 1
    if isinstance(min_pairs, (bool, np.bool_)) or not isinstance(min_pairs, (int, np.integer)):
        raise ValueError('min_pairs must be an integer in 1..%d, not %r' % (n - 1, min_pairs))
    if not (1 <= int(min_pairs) <= n - 1):
        raise ValueError('min_pairs must lie in 1..%d (an element of %d has %d pairs), not %r' % (n - 1, n, n - 1, min_pairs))
    return int(min_pairs), bool(beam), bool(capon)


def beam_trace_window(W, kind='hann'):
    """The synthesis window (W,) that stitches the windows of a beam trace (``nbls_set_beam_trace``):
    ``'hann'``: sin^2(pi (t + 1/2) / W), strictly positive, so every sample a usable window covers has a positive
    denominator; ``'boxcar'``: ones (the plain average of the windows that cover a sample)."""
    if isinstance(W, (bool, np.bool_)) or not isinstance(W, (int, np.integer)) or int(W) < 1:
        raise ValueError('the window length must be a positive integer, not %r' % (W,))
    if kind == 'boxcar':
        return np.ones(int(W))
    if kind == 'hann':
        return np.sin(np.pi * (np.arange(int(W)) + 0.5) / int(W)) ** 2
    raise ValueError("kind must be 'hann' or 'boxcar', not %r" % (kind,))


def check_beam_trace(W, window='hann', mdccm_min=None, kept=False, has_kept=False, window_slice=None, estimators=None,
                     comm=False):
    """Everything ``nbls_set_beam_trace`` and the plan behind it refuse, as ``ValueError`` before any GPU work -> (table,
    mdccm_min, kept): the synthesis windows of the bands one after the other (float64, sum of ``W`` entries), the MdCCM gate
    as a float (NaN: off) and the kept flag.  ``W``: the window length of every band; ``window``: ``'hann'`` / ``'boxcar'``
    (``beam_trace_window``) or the table itself, flat or one array per band; ``mdccm_min``: None or NaN (no gate) or a number —
    only windows with MdCCM >= it enter the trace; ``kept``: sum each window over the elements LTS kept in it, which needs a
    plan that names them (``has_kept``: the call also passes ``kept=``, ``check_kept``).  A window slice, further estimators
    and an RCCL communicator are refused."""
    W = np.asarray(W)
    if W.ndim != 1 or len(W) < 1 or W.dtype.kind not in 'iu' or (W < 1).any():
        raise ValueError('the window lengths must be positive integers, one per band')
    if not isinstance(kept, (bool, np.bool_)):
        raise ValueError('kept must be True or False, not %r' % (kept,))
    if kept and not has_kept:
        raise ValueError('the beam trace of the kept elements needs a plan that names them (kept=, planner.check_kept)')
    if window_slice is not None:
        raise ValueError('the beam trace is not available for a slice of the windows (window_slice): it would not cover the trace')
    if estimators:
        raise ValueError('the beam trace is not available with further estimators')
    if comm:
        raise ValueError('the beam trace is not available with an RCCL communicator (the gathered block does not carry it)')
    if mdccm_min is None:
        gate = float('nan')
    else:
        if isinstance(mdccm_min, (bool, np.bool_)) or not isinstance(mdccm_min, (int, float, np.integer, np.floating)):
            raise ValueError('mdccm_min must be a number or None, not %r' % (mdccm_min,))
        gate = float(mdccm_min)                    # (NaN: the gate is off, as in the C ABI)
    if isinstance(window, str):
        table = np.concatenate([beam_trace_window(int(w), window) for w in W])
    else:
        try:                                       # the table itself: flat, or one array per band
            table = np.concatenate([np.asarray(p, dtype=np.float64).reshape(-1) for p in window])
        except (TypeError, ValueError):
            raise ValueError("window must be 'hann', 'boxcar' or the synthesis windows of the bands")
    if table.size != int(W.sum()):
        raise ValueError('%d synthesis-window entries for bands whose window lengths add up to %d' % (table.size, int(W.sum())))
    if not np.isfinite(table).all() or (table < 0).any():
        raise ValueError('the synthesis window must be finite and not negative')
    o = 0
    for b, w in enumerate(W):
        if not (table[o:o + int(w)] > 0).any():
            raise ValueError('the synthesis window of band %d is all zero' % b)
        o += int(w)
    return np.ascontiguousarray(table, dtype=np.float64), gate, bool(kept)


ELEMENT_DELAY_MAX_SHIFT = 256      # NBLS_ELEMENT_DELAY_MAX_SHIFT


def element_shifts(fmax_list, fs, period_fraction=0.5):
    """Per-band shift ranges of the element delays (``nbls_set_element_delays``) -> int32 (nbands,):
    ``min(seed_halfwidths(fmax_list, fs, period_fraction), 256)`` samples — by default half a period of the band's upper
    edge either side of the modelled delay, so that the neighbouring cycle stays outside the range."""
    return np.minimum(seed_halfwidths(fmax_list, fs, period_fraction), ELEMENT_DELAY_MAX_SHIFT).astype(np.int32)


def check_element_shifts(max_shift, nbands):
    """``max_shift`` of the element delays (samples; one integer for every band, or ``nbands`` of them) -> int32
    (nbands,); ``ValueError`` (before any GPU work) unless the entries are integers in 0 .. 256 and their number fits."""
    if isinstance(nbands, (bool, np.bool_)) or not isinstance(nbands, (int, np.integer)) or int(nbands) < 1:
        raise ValueError('nbands must be a positive integer, not %r' % (nbands,))
    try:
        k = np.asarray(max_shift)
    except Exception:
        raise ValueError('max_shift must be an integer or a list of integers, one per band')
    if k.dtype == object or k.dtype.kind not in 'iu' or k.ndim > 1 or k.size < 1:
        raise ValueError('max_shift must be an integer or a list of integers, one per band, not %r' % (max_shift,))
    if k.ndim == 0:
        k = np.full(int(nbands), int(k))
    if k.size != int(nbands):
        raise ValueError('%d shift ranges for %d bands' % (k.size, int(nbands)))
    if (k < 0).any() or (k > ELEMENT_DELAY_MAX_SHIFT).any():
        raise ValueError('max_shift must lie in 0..%d samples, not %r' % (ELEMENT_DELAY_MAX_SHIFT, max_shift))
    return np.ascontiguousarray(k, dtype=np.int32)


FAMILY_MAX_REACH = 8      # largest band_reach / time_reach of a family request (NBLS_FAMILY_MAX_REACH)
# the columns of a family table row (include/nbls.h), in order
FAMILY_FIELDS = ('count', 'first_cell', 'peak_cell', 'band_lo', 'band_hi', 'segment', 'sample_first', 'sample_end')


def _family_real(name, x):
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, float, np.integer, np.floating)):
        raise ValueError('%s must be a number, not %r' % (name, x))
    return float(x)


def _family_whole(name, x):
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
        raise ValueError('%s must be an integer, not %r' % (name, x))
    return int(x)


def check_families(mdccm_min, baz_tol, vel_tol, vel_min, vel_max, sigma_tau_max=None, band_reach=1, time_reach=1, min_pixels=1,
                   window_slice=None, estimators=None, comm=False):
    """Everything ``nbls_set_families`` and the plan behind it refuse, as ``ValueError`` before any GPU work -> the request as
    a dict of ``mdccm_min``, ``vel_min``, ``vel_max``, ``sigma_tau_max`` (None: that gate is off), ``baz_tol`` (degrees),
    ``vel_tol`` (km/s), ``band_reach``, ``time_reach`` and ``min_pixels``.  ``mdccm_min`` finite;
    ``vel_min <= vel_max``, both finite; ``sigma_tau_max`` None, NaN (both: no gate) or finite; ``baz_tol`` in [0, 180];
    ``vel_tol`` >= 0 and finite; ``band_reach`` in 0..8; ``time_reach`` in 1..8; ``min_pixels`` >= 1.  A window slice, further
    estimators and an RCCL communicator are refused for the in-pass request (``label_families`` covers them)."""
    p = dict(mdccm_min=_family_real('mdccm_min', mdccm_min), vel_min=_family_real('vel_min', vel_min), vel_max=_family_real('vel_max', vel_max),
             sigma_tau_max=None if sigma_tau_max is None else _family_real('sigma_tau_max', sigma_tau_max),
             baz_tol=_family_real('baz_tol', baz_tol), vel_tol=_family_real('vel_tol', vel_tol), band_reach=_family_whole('band_reach', band_reach),
             time_reach=_family_whole('time_reach', time_reach), min_pixels=_family_whole('min_pixels', min_pixels))
    if not np.isfinite(p['mdccm_min']):
        raise ValueError('mdccm_min must be finite')
    if not (np.isfinite(p['vel_min']) and np.isfinite(p['vel_max']) and p['vel_min'] <= p['vel_max']):
        raise ValueError('vel_min <= vel_max, both finite')
    if p['sigma_tau_max'] is not None:
        if np.isnan(p['sigma_tau_max']):
            p['sigma_tau_max'] = None
        elif np.isinf(p['sigma_tau_max']):
            raise ValueError('sigma_tau_max must be finite, or None for no gate')
    if not (0.0 <= p['baz_tol'] <= 180.0):
        raise ValueError('baz_tol must lie in [0, 180] degrees')
    if not (p['vel_tol'] >= 0.0) or np.isinf(p['vel_tol']):
        raise ValueError('vel_tol must be finite and not negative')
    if not (0 <= p['band_reach'] <= FAMILY_MAX_REACH):
        raise ValueError('band_reach must lie in 0..%d' % FAMILY_MAX_REACH)
    if not (1 <= p['time_reach'] <= FAMILY_MAX_REACH):
        raise ValueError('time_reach must lie in 1..%d' % FAMILY_MAX_REACH)
    if p['min_pixels'] < 1 or p['min_pixels'] >= 2 ** 31:
        raise ValueError('min_pixels must be at least 1')
    if window_slice is not None:
        raise ValueError('families are not available for a slice of the windows (window_slice): it would not cover the lattice')
    if estimators:
        raise ValueError('families are not available with further estimators')
    if comm:
        raise ValueError('families are not available with an RCCL communicator (the gathered block does not carry them)')
    return p


def check_family_lattice(nseg, winlens, incs, nwin, vel, baz, mdccm, sigma_tau, gate):
    """The arrays of ``label_families`` as ``nbls_label_families`` takes them -> (nseg, winlens, incs, nwin, vel, baz, mdccm,
    sigma_tau), contiguous int32 / float64; ``ValueError`` for what the library refuses: grids that are not 2-D of one shape
    with ``len(winlens) * nseg`` rows, 2^31 cells or more, a window length or hop below 1, ``nwin`` outside [0, vector_len],
    a ``sigma_tau`` that does not match the gate."""
    nseg = _family_whole('nseg', nseg)
    winlens, incs, nwin = (np.asarray(a) for a in (winlens, incs, nwin))
    for name, a in (('winlens', winlens), ('incs', incs), ('nwin', nwin)):
        if a.ndim != 1 or a.dtype.kind not in 'iu':
            raise ValueError('%s must be a 1-D array of integers' % name)
    vel, baz, mdccm = (np.ascontiguousarray(g, dtype=np.float64) for g in (vel, baz, mdccm))
    if nseg < 1 or len(winlens) < 1 or len(incs) != len(winlens):
        raise ValueError('one window length and one hop per band, and at least one recording')
    rows = len(winlens) * nseg
    if vel.ndim != 2 or vel.shape[0] != rows or vel.shape[1] < 1 or baz.shape != vel.shape or mdccm.shape != vel.shape:
        raise ValueError('vel, baz and mdccm must be (%d, vector_len) arrays of one shape' % rows)
    if vel.size >= 2 ** 31:
        raise ValueError('fewer than 2^31 cells are taken')
    if (winlens < 1).any() or (incs < 1).any() or (winlens >= 2 ** 31).any() or (incs >= 2 ** 31).any():
        raise ValueError('window lengths and hops must be positive')
    if len(nwin) != rows or (nwin < 0).any() or (nwin > vel.shape[1]).any():
        raise ValueError('nwin must have one entry per row, in 0..vector_len')
    if gate != (sigma_tau is not None):
        raise ValueError('sigma_tau is given exactly when sigma_tau_max sets a gate')
    if sigma_tau is not None:
        sigma_tau = np.ascontiguousarray(sigma_tau, dtype=np.float64)
        if sigma_tau.shape != vel.shape:
            raise ValueError('sigma_tau must have the shape of vel')
    return (nseg, winlens.astype(np.int32), incs.astype(np.int32), nwin.astype(np.int32), vel, baz, mdccm, sigma_tau)


def family_table(family, table, vel, baz, mdccm, sigma_tau, band_edges, winlens, incs, fs, starttime):
    """The per-family summary of a labelling, on the host -> dict of arrays with one entry per family.

    ``family`` (rows, vector_len) and ``table`` (F, 8) as ``label_families`` / a families call return them, the four grids of
    the same lattice (``sigma_tau`` may be None), ``band_edges`` [(fmin, fmax)] and ``winlens`` / ``incs`` (samples) per band,
    ``fs`` in Hz, ``starttime`` the recording's start as a date number (days, as ``res.t``), one for all or one per recording.
    Members come in ascending cell order from a stable sort and every sum is ``np.add.reduceat`` over them.  Keys: ``count``;
    ``t_start`` / ``t_end`` (seconds from the start: ``sample_first / fs``, ``sample_end / fs``) and ``t_start_datenum`` /
    ``t_end_datenum``; ``f_lo`` / ``f_hi`` (the lower edge of ``band_lo``, the upper of ``band_hi``); ``baz_mean`` /
    ``baz_std`` (circular, degrees: R = |mean e^{i baz}|, std = sqrt(-2 ln R)); ``vel_mean`` / ``vel_std`` (population);
    ``mdccm_median`` / ``mdccm_peak``; ``peak_band`` / ``peak_window`` / ``peak_baz`` / ``peak_vel``; ``sigma_tau_median``
    (NaN without ``sigma_tau``); and the table's own columns under their names (``FAMILY_FIELDS``)."""
    family = np.asarray(family)
    table = np.asarray(table, dtype=np.int64).reshape(-1, len(FAMILY_FIELDS))
    rows, vl = family.shape
    F = len(table)
    flat = family.reshape(-1)
    cells = np.flatnonzero(flat >= 0)
    mem = cells[np.argsort(flat[cells], kind='stable')]
    count = np.bincount(flat[cells], minlength=F)[:F] if F else np.zeros(0, dtype=np.int64)
    if F and (len(mem) != count.sum() or (count != table[:, 0]).any() or (count < 1).any()):
        raise ValueError('family and table do not describe the same labelling')
    start = np.r_[0, np.cumsum(count)[:-1]].astype(np.int64) if F else np.zeros(0, dtype=np.int64)
    g = lambda a: np.asarray(a, dtype=np.float64).reshape(-1)[mem]
    mean = lambda x: np.add.reduceat(x, start) / count if F else np.zeros(0)

    def median(x):
        out = np.full(F, np.nan)
        for k in range(F):
            out[k] = np.median(x[start[k]:start[k] + count[k]])
        return out
    rad = np.deg2rad(g(baz))
    c, s = mean(np.cos(rad)), mean(np.sin(rad))
    R = np.minimum(np.hypot(c, s), 1.0)
    v = g(vel)
    vm = mean(v)
    with np.errstate(divide='ignore'):
        baz_std = np.rad2deg(np.sqrt(np.abs(-2.0 * np.log(R))))
    edges = np.asarray(band_edges, dtype=np.float64).reshape(-1, 2)
    t0 = np.broadcast_to(np.asarray(starttime, dtype=np.float64).reshape(-1), (max(1, rows // len(edges)),))
    seg = table[:, 5]
    peak = table[:, 2]
    flatten = lambda a: np.asarray(a, dtype=np.float64).reshape(-1)
    out = dict(count=table[:, 0].copy(), t_start=table[:, 6] / float(fs), t_end=table[:, 7] / float(fs),
               f_lo=edges[table[:, 3], 0], f_hi=edges[table[:, 4], 1], baz_mean=np.rad2deg(np.arctan2(s, c)) % 360.0, baz_std=baz_std,
               vel_mean=vm, vel_std=np.sqrt(np.maximum(mean((v - np.repeat(vm, count)) ** 2), 0.0)),
               mdccm_median=median(g(mdccm)), mdccm_peak=flatten(mdccm)[peak], peak_band=(peak // vl) // (rows // len(edges)),
               peak_window=peak % vl, peak_baz=flatten(baz)[peak], peak_vel=flatten(vel)[peak],
               sigma_tau_median=median(g(sigma_tau)) if sigma_tau is not None else np.full(F, np.nan),
               band_lo=table[:, 3].copy(), band_hi=table[:, 4].copy(), segment=seg.copy())
    for k, name in enumerate(FAMILY_FIELDS):               # the table's own columns beside the summary
        out.setdefault(name, table[:, k].copy())
    out['t_start_datenum'] = t0[seg] + out['t_start'] / 86400.0
    out['t_end_datenum'] = t0[seg] + out['t_end'] / 86400.0
    return out
