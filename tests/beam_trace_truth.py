"""CPU truths of the beam trace (``nbls_set_beam_trace``; the definition is in include/nbls.h).

For ONE result row: ``filt`` (N, npts) the filtered band, ``z`` (VL, 2) the solved slowness of every window, ``mdccm`` (VL,),
``nwin`` its window count, ``dropped_mask`` (VL,) uint32 or None (None: every window sums all N elements), ``xij`` (P, 2) the
co-array whose row m - 1 is pair (0, m), ``fs``, window length ``W``, hop ``inc``, synthesis window ``g`` (W,), and the gate
``mdccm_min`` (None or NaN: off).

(a) ``restate``: the definition's own sequence of IEEE float64 operations, in NumPy — what the kernel must give bit for bit.
(b) ``reference``: the same delays and windows, every sum, product and the division in long double, with a per-sample
    bound on |(a) - (b)| derived below from the operation count.

The bound.  u = 2^-53, gamma_k = k u / (1 - k u).  For one output sample let C be the number of usable windows that cover
it and N the element count (a window of the kept set adds M_w <= N terms).
  s_w   is N terms added to 0.0 from the left: the first addition is exact, N - 1 round.
  g s_w is one rounded product; the C products are added to 0.0 from the left: C - 1 rounded additions.
        Every term g x_m of acc therefore carries at most (N - 1) + 1 + (C - 1) = N + C - 1 factors (1 + delta).
  den   g M_w is one rounded product (M_w is a small integer, exact), C - 1 rounded additions of non-negative terms:
        den_hat = den (1 + theta), |theta| <= gamma_C.
  The quotient rounds once.
So trace_hat = sum g x_m (1 + theta_wm) / den with each theta_wm a product of at most (N + C - 1) + C + 1 = N + 2 C factors
(1 + delta)^(+-1), i.e. |theta_wm| <= gamma_(N + 2C) (Higham, Accuracy and Stability, Lemma 3.1), and

    |trace_hat - trace| <= gamma_(N + 2C) * A / den,    A = sum_w g[n - s0] * sum_m |x_m|.

The long-double reference has the same structure with u_l = 2^-64 (x87 extended) or smaller: its own error,
gamma^l_(N + 2C) A / den, is added to the bound.  Nothing here was fitted to GPU output."""
import numpy as np

U = 2.0 ** -53
MAX_DELAY = 2.0 ** 30


def kept_bits(dropped, N):
    """The kept elements of a window from its dropped mask -> (bool (N,), M): the complement, or everything where fewer
    than 3 would remain (nbls_set_kept_elements)."""
    keep = np.array([not (int(dropped) >> m) & 1 for m in range(N)])
    if keep.sum() < 3:
        keep[:] = True
    return keep, int(keep.sum())


def window_delays(xij, fs, z, N):
    """-> the delays d (N,) int64 of a window with slowness ``z``, or None where the window is unusable for its slowness:
    d_0 = 0, d_m = rint(fs * (xij[m-1][0] * z0 + xij[m-1][1] * z1)), plain float64 operations, ties to even."""
    z0, z1 = np.float64(z[0]), np.float64(z[1])
    if not (np.isfinite(z0) and np.isfinite(z1)):
        return None
    d = np.zeros(N, dtype=np.int64)
    for m in range(1, N):
        tau = np.float64(fs) * (np.float64(xij[m - 1][0]) * z0 + np.float64(xij[m - 1][1]) * z1)
        if not (abs(tau) < MAX_DELAY):
            return None
        d[m] = int(np.rint(tau))
    return d


def usable_windows(z, mdccm, nwin, xij, fs, N, mdccm_min=None):
    """-> [(w, d)] of the usable windows of a row, ascending."""
    gate = mdccm_min is not None and mdccm_min == mdccm_min
    out = []
    for w in range(int(nwin)):
        if gate and not (mdccm[w] >= mdccm_min):
            continue
        d = window_delays(xij, fs, z[w], N)
        if d is not None:
            out.append((w, d))
    return out


def _shifted(x, i0, W, dtype):
    """x[i0 : i0 + W] with 0.0 where the index is outside [0, len(x))."""
    npts = len(x)
    out = np.zeros(W, dtype=dtype)
    a, b = max(i0, 0), min(i0 + W, npts)
    if b > a:
        out[a - i0:b - i0] = x[a:b]
    return out


def _run(filt, z, mdccm, nwin, dropped_mask, xij, fs, W, inc, g, mdccm_min, dtype):
    filt = np.asarray(filt, dtype=np.float64)
    N, npts = filt.shape
    W, inc = int(W), int(inc)
    gq = np.asarray(g, dtype=np.float64).astype(dtype)
    acc, den, A = np.zeros(npts, dtype=dtype), np.zeros(npts, dtype=dtype), np.zeros(npts, dtype=dtype)
    cover = np.zeros(npts, dtype=np.int64)
    for w, d in usable_windows(z, mdccm, nwin, xij, fs, N, mdccm_min):
        s0 = w * inc
        keep, M = (np.ones(N, dtype=bool), N) if dropped_mask is None else kept_bits(dropped_mask[w], N)
        s, sa = np.zeros(W, dtype=dtype), np.zeros(W, dtype=dtype)
        for m in range(N):
            if keep[m]:
                x = _shifted(filt[m], s0 + int(d[m]), W, dtype)
                s = s + x
                sa = sa + np.abs(x)
        n1 = min(s0 + W, npts)
        k = n1 - s0
        if k <= 0:
            continue
        acc[s0:n1] = acc[s0:n1] + gq[:k] * s[:k]
        den[s0:n1] = den[s0:n1] + gq[:k] * dtype(M)
        A[s0:n1] = A[s0:n1] + gq[:k] * sa[:k]
        cover[s0:n1] += 1
    pos = den > 0
    out = np.zeros(npts, dtype=dtype)
    with np.errstate(invalid='ignore', over='ignore'):
        out[pos] = acc[pos] / den[pos]
    return out, den, A, cover


def restate(filt, z, mdccm, nwin, dropped_mask, xij, fs, W, inc, g, mdccm_min=None):
    """(a) -> trace (npts,) float64, the definition restated operation by operation."""
    return _run(filt, z, mdccm, nwin, dropped_mask, xij, fs, W, inc, g, mdccm_min, np.float64)[0]


def bound_constant(N, C):
    """The count of (1 + delta) factors a term of the quotient carries: N + 2 C (module docstring)."""
    return N + 2 * C


def reference(filt, z, mdccm, nwin, dropped_mask, xij, fs, W, inc, g, mdccm_min=None):
    """(b) -> (trace (npts,) long double, bound (npts,) float64 on |(a) - (b)|, cover (npts,) the usable windows over every
    sample)."""
    N = np.asarray(filt).shape[0]
    out, den, A, cover = _run(filt, z, mdccm, nwin, dropped_mask, xij, fs, W, inc, g, mdccm_min, np.longdouble)
    ul = float(np.finfo(np.longdouble).eps) / 2.0
    k = bound_constant(N, cover).astype(np.float64)
    gamma = k * U / (1.0 - k * U) + k * ul / (1.0 - k * ul)
    bound = np.zeros(len(out))
    pos = den > 0
    with np.errstate(invalid='ignore', over='ignore'):
        bound[pos] = gamma[pos] * (A[pos] / den[pos]).astype(np.float64)
    return out, bound, cover
