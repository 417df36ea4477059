"""The sub-sample refinement of the picked lags (``nbls_set_lag_refinement``, csrc/refine.hip), stated
literally in ``np.longdouble`` on given windows and given lags.  CPU only: nothing here imports the GPU library.

For a pair of windows a, b of W samples with picked lag l:

    R(m) = sum_n a[n - m] b[n]   over the n for which both indices are in [0, W)   (np.correlate(a, b, 'full')[W-1-m])
    Nn = R(l-1) - R(l+1),  D = R(l-1) - 2 R(l) + R(l+1),  frac = 1/2 Nn / D clamped to [-1/2, 1/2]
    frac = 0 if |l| >= W-1, if D >= 0, or if one of the three values or the quotient is not finite

**Rounding bound of a float64 implementation.**  Whatever the order of its un-fused sums, a float64 R(m) is within
gamma_W sum |a||b| <= W 2^-53 |a| |b| (Cauchy-Schwarz) of the true value.  With E = 2 W 2^-53 |a| |b| the numerator is
within E of Nn (two sums and one subtraction), the denominator within 4 E of D, and for |D| > 4 E

    |frac' - frac| <= (E + 2 |frac| E) / (|D| - 4 E) + 4 * 2^-53

(the quotient, the halving and the clamp round a value of at most 1/2).  Not a measured number."""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53


def corr3(a, b, lag):
    """R(l-1), R(l), R(l+1) in long double for windows a, b (W,) -> list of three np.longdouble."""
    W = len(a)
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    out = []
    for m in (lag - 1, lag, lag + 1):
        lo, hi = max(0, m), min(W, W + m)                       # n and n - m both in [0, W)
        out.append(np.sum(a[lo - m:hi - m] * b[lo:hi], dtype=LD) if hi > lo else LD(0))
    return out


def refine_pair(a, b, lag):
    """One pair -> dict(frac float64, frac_ld, Nn, D (long double; None where |l| >= W-1 decides), E, bound)."""
    W = len(a)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        E = 2.0 * W * U53 * float(np.sqrt(np.sum(np.square(a, dtype=LD)))) * float(np.sqrt(np.sum(np.square(b, dtype=LD))))
        if abs(int(lag)) >= W - 1:
            return dict(frac=0.0, frac_ld=LD(0), Nn=None, D=None, E=E, bound=4 * U53)
        rm, r0, rp = corr3(a, b, int(lag))
        nn, dd = rm - rp, rm - 2 * r0 + rp
        ok = bool(np.isfinite(rm) and np.isfinite(r0) and np.isfinite(rp) and dd < 0)
        f = LD(0)
        if ok:
            f = LD(0.5) * nn / dd
            f = LD(0) if not np.isfinite(f) else min(max(f, LD(-0.5)), LD(0.5))
        margin = abs(float(dd)) - 4 * E if np.isfinite(dd) else -1.0
        bound = (E + 2 * abs(float(f)) * E) / margin + 4 * U53 if margin > 0 else np.inf
    return dict(frac=float(f), frac_ld=f, Nn=nn, D=dd, E=E, bound=bound)


def refine_windows(data, W, starts, pairs, lag):
    """``data`` (N, npts), windows of W samples at ``starts``, ``lag`` (nwin, P) integers of ``pairs`` ->
    dict(frac, bound, D, E: each (nwin, P) float64; D is NaN where |l| >= W-1 decided)."""
    n, P = len(starts), len(pairs)
    out = {k: np.zeros((n, P)) for k in ('frac', 'bound', 'D', 'E')}
    for w, s in enumerate(starts):
        win = data[:, s:s + W]
        for k, (i, j) in enumerate(pairs):
            r = refine_pair(win[i], win[j], lag[w, k])
            out['frac'][w, k], out['bound'][w, k], out['E'][w, k] = r['frac'], r['bound'], r['E']
            out['D'][w, k] = np.nan if r['D'] is None else float(r['D'])
    return out


def pick_lags(data, W, starts, pairs):
    """lag = W-1-argmax of the normalised full correlation, first maximum wins (oracle.correlate_windows) -> (nwin, P)."""
    lag = np.zeros((len(starts), len(pairs)), dtype=np.int64)
    with np.errstate(invalid='ignore', divide='ignore'):
        for w, s in enumerate(starts):
            for k, (i, j) in enumerate(pairs):
                a, b = data[i, s:s + W], data[j, s:s + W]
                c = np.correlate(a, b, 'full') / np.sqrt(np.sum(a * a) * np.sum(b * b))
                lag[w, k] = W - 1 - int(np.argmax(c))
    return lag


def pair_table(N):
    return [(i, j) for i in range(N - 1) for j in range(i + 1, N)]


def sinusoid_wave(N, npts, fs, seed, max_delay=None, noise=0.0, nsin=40, f0=0.4, f1=2.0, r0=0.05, r1=0.3, vel=0.34,
                  timing_error_s=0.0):
    """A plane wave of ``nsin`` sinusoids at f0 .. f1 Hz, evaluated analytically at the fractional delays d_i = -r_i . z
    (element i records s(t - d_i): tau_ij = d_j - d_i = x_ij . z, the sign convention of the measured lags), over an
    array of radii r0 .. r1 km, plus ``noise`` times the signal's rms of incoherent white noise -> (data (N, npts),
    rij (2, N) km, z (2,) s/km).  ``max_delay`` (samples): the geometry is scaled so that no |d_i| exceeds it.
    ``timing_error_s``: the last element records that much later (a mistimed element: its pairs are what LTS drops)."""
    rng = np.random.default_rng(seed)
    rad = rng.uniform(r0, r1, N)
    az = rng.uniform(0.0, 2.0 * np.pi, N)
    rij = np.stack([rad * np.sin(az), rad * np.cos(az)])
    baz = rng.uniform(0.0, 2.0 * np.pi)
    z = np.array([np.sin(baz), np.cos(baz)]) / vel
    d = -(z @ rij)
    if max_delay is not None and np.max(np.abs(d)) * fs > max_delay:
        s = max_delay / (np.max(np.abs(d)) * fs)
        rij, d = rij * s, d * s
    d[-1] += timing_error_s
    f = rng.uniform(f0, f1, nsin)
    ph = rng.uniform(0.0, 2.0 * np.pi, nsin)
    amp = rng.uniform(0.5, 1.0, nsin)
    t = np.arange(npts) / fs
    data = np.stack([np.sum(amp[:, None] * np.sin(2.0 * np.pi * f[:, None] * (t[None, :] - d[i]) + ph[:, None]), axis=0)
                     for i in range(N)])
    if noise:
        data = data + noise * np.sqrt(np.mean(data ** 2)) * rng.standard_normal(data.shape)
    return np.ascontiguousarray(data), np.ascontiguousarray(rij), z
