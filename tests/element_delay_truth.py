"""CPU reference of the element delays (``nbls_set_element_delays``), written from the definition in
``include/nbls.h`` and nothing else: (a) a float64 restatement, operation by operation, and (b) the same in
``np.longdouble`` with the rounding bounds the GPU's float64 results are held to.

For one unit (the N element rows ``filt`` (N, npts), the co-array ``xij`` whose first N-1 rows are the pairs (0, m), the
slowness ``z`` AS FETCHED FROM THE GPU, window start s0, length W, shift range K, the kept bits of the set S):

    tau_0 = 0, tau_m = fs * (xij[m-1, 0] * z0 + xij[m-1, 1] * z1), d_m = rint(tau_m)          float64, ties to even
    y_m(k)[t] = filt[m, s0 + t + d_m + k], 0.0 outside [0, npts)                              k in [-K, K]
    b[t] = ((0.0 + y_a(0)[t]) + y_b(0)[t]) + ... over S ascending;  b_m = b - y_m(0) for m in S, b otherwise
    E_b,m = sum b_m^2,  E_m(k) = sum y_m(k)^2,  C_m(k) = sum y_m(k) b_m,  c_m(k) = C_m(k) / sqrt(E_m(k) * E_b,m)
    k* under "c descending, |k| ascending, k ascending" (NaN no candidate; none: shift 0, cc NaN, delay NaN)
    frac = parabola of (c(k*-1), c(k*), c(k*+1)) by the rule of refine_fraction.h, 0 where |k*| == K
    delay = ((((double)(d_m + k*)) + frac) - tau_m) / fs

The definition leaves the order of the sums over t open; (a) adds in plain t order.

Tolerances of (b), per value — derived, not fitted.  u = 2^-53.  The samples are exact.  The long-double sums carry 2^-64
relative: noise here.  Each of C, E_m, E_b is a W-term float64 sum of rounded products in some order: 64 ulps of slack per
term, as section 12 charges (64 W u times the sum of the terms' magnitudes).  The float64 b_m carries |S| additions and one
subtraction:

    e_b[t]  = (|S| + 1) u sum_{i in S} |y_i(0)[t]|                              |b_m,GPU[t] - b_m[t]| <= e_b[t]
    e_C(k)  = 64 W u sum_t |y| (|b_m| + e_b) + sum_t |y| e_b
    e_E(k)  = 64 W u E_m(k)
    e_Eb    = 64 W u sum_t (|b_m| + e_b)^2 + sum_t (2 |b_m| e_b + e_b^2)
    P = E_m E_b:   e_P = (E_m + e_E)(E_b + e_Eb) (1 + u) - P
    R = sqrt(P):   e_R = sqrt(P) - sqrt(P - e_P) + u sqrt(P + e_P)              infinite unless P > e_P
    c = C / R:     e_c = (|C| + e_C) / (R - e_R) (1 + u) - |C| / R              infinite unless R > e_R
    parabola nn = rm - rp, dd = (rm - 2 r0) + rp, f = 0.5 nn / dd:
        e_nn = e_m + e_p + u (|nn| + e_m + e_p)
        e_dd = e_m + 2 e_0 + e_p + 2 u (|rm| + 2 |r0| + |rp| + e_m + 2 e_0 + e_p)
        e_f  = 0.5 ((|nn| + e_nn) / (|dd| - e_dd) (1 + u) - |nn| / |dd|)        infinite where |dd| <= e_dd; the clamp to
                                                                                [-1/2, 1/2] does not widen it
    e_delay = (e_f + u (|d_m + k*| + 1 + K + 1)) / fs + u |delay|               two rounded additions and a division

Cells whose parabola bound is infinite are compared on ``shift`` and ``cc`` only.  A ``shift`` that differs from (b)'s is
accepted (``check_element``) only where (b)'s c at the two shifts differ by less than the sum of their bounds; ``cc`` and
``delay`` are then held to (b) at the shift the GPU took."""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
MAX_DELAY = 2.0 ** 30
MAX_SHIFT = 256
SLACK = 64


def taus(xij, z, fs, N):
    """-> (tau (N,) float64, d (N,) int64), or None where the unit is bad by definition."""
    xij = np.asarray(xij, dtype=np.float64)[:N - 1]
    z0, z1 = np.float64(z[0]), np.float64(z[1])
    if not (np.isfinite(z0) and np.isfinite(z1)):
        return None
    tau = np.concatenate(([0.0], np.float64(fs) * (xij[:, 0] * z0 + xij[:, 1] * z1)))
    if not np.all(np.abs(tau) < MAX_DELAY):
        return None
    return tau, np.rint(tau).astype(np.int64)


def kept_bits(dropped, N):
    """The set S from a dropped mask: its clear bits, the whole array where fewer than 3 would remain -> bool (N,)."""
    keep = np.array([not ((int(dropped) >> m) & 1) for m in range(N)])
    return keep if keep.sum() >= 3 else np.ones(N, dtype=bool)


def shifted(row, s0, W, d, K, dtype):
    """y(k)[t] = row[s0 + t + d + k] for k in [-K, K], 0.0 outside the trace -> (2K + 1, W) of ``dtype``."""
    n = np.arange(W + 2 * K, dtype=np.int64) + (int(s0) + int(d) - K)
    ok = (n >= 0) & (n < len(row))
    seg = np.zeros(W + 2 * K, dtype=dtype)
    seg[ok] = np.asarray(row)[n[ok]].astype(dtype)
    return np.lib.stride_tricks.sliding_window_view(seg, W)


def fraction(rm, r0, rp):
    """The rule of refine_fraction.h in float64."""
    rm, r0, rp = np.float64(rm), np.float64(r0), np.float64(rp)
    with np.errstate(all='ignore'):
        nn = rm - rp
        dd = (rm - 2.0 * r0) + rp
        f = 0.5 * nn / dd
    if not (np.isfinite(rm) and np.isfinite(r0) and np.isfinite(rp) and dd < 0.0 and np.isfinite(f)) or f == 0.0:
        return 0.0
    return float(min(0.5, max(-0.5, f)))


def pick(c, K):
    """k* of the quotients c (2K + 1,) under "c descending, |k| ascending, k ascending"; None without a candidate."""
    best = None
    for i in range(2 * K + 1):
        v, k = c[i], i - K
        if v != v:
            continue
        if best is None or v > c[best + K] or (v == c[best + K] and (abs(k), k) < (abs(best), best)):
            best = k
    return best


def unit64(filt, fs, xij, z, s0, W, K, keep=None):
    """(a): one unit in float64 -> (delay (N,), cc (N,), shift (N,) int32, c (N, 2K + 1))."""
    filt = np.asarray(filt, dtype=np.float64)
    N = filt.shape[0]
    delay, cc, shift = np.full(N, np.nan), np.full(N, np.nan), np.zeros(N, dtype=np.int32)
    call = np.full((N, 2 * K + 1), np.nan)
    td = taus(xij, z, fs, N)
    if td is None:
        return delay, cc, shift, call
    tau, d = td
    keep = np.ones(N, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    y = [shifted(filt[m], s0, W, d[m], K, np.float64) for m in range(N)]
    b = np.zeros(W)
    for m in range(N):
        if keep[m]:
            b = b + y[m][K]
    with np.errstate(all='ignore'):
        for m in range(N):
            bm = b - y[m][K] if keep[m] else b
            Eb = np.cumsum(bm * bm)[-1]
            E = np.cumsum(y[m] * y[m], axis=1)[:, -1]
            C = np.cumsum(y[m] * bm[None, :], axis=1)[:, -1]
            c = C / np.sqrt(E * Eb)
            call[m] = c
            ks = pick(c, K)
            if ks is None:
                continue
            fr = 0.0 if abs(ks) == K else fraction(c[ks - 1 + K], c[ks + K], c[ks + 1 + K])
            shift[m], cc[m] = ks, c[ks + K]
            delay[m] = ((np.float64(d[m] + ks) + fr) - tau[m]) / np.float64(fs)
    return delay, cc, shift, call


def _fraction_ld(rm, r0, rp, em, e0, ep):
    """The parabola in long double and its bound -> (frac, e_f)."""
    if not (np.isfinite(rm) and np.isfinite(r0) and np.isfinite(rp)):
        return LD(0), LD(0)            # (a NaN quotient is NaN in float64 too — 0/0 or a NaN sample —: the rule gives 0)
    nn = rm - rp
    dd = (rm - 2 * r0) + rp
    e_nn = em + ep + U * (abs(nn) + em + ep)
    e_dd = em + 2 * e0 + ep + 2 * U * (abs(rm) + 2 * abs(r0) + abs(rp) + em + 2 * e0 + ep)
    if not (np.isfinite(e_dd) and np.isfinite(e_nn)) or abs(dd) <= e_dd:
        return LD(0), np.inf
    if dd >= 0:
        return LD(0), np.inf           # (no strict maximum: only at an edge of the order, never bounded here)
    f = LD(0.5) * nn / dd
    e_f = LD(0.5) * ((abs(nn) + e_nn) / (abs(dd) - e_dd) * (1 + U) - abs(nn) / abs(dd))
    return min(LD(0.5), max(LD(-0.5), f)), e_f


def unit(filt, fs, xij, z, s0, W, K, keep=None):
    """(b): one unit in long double -> dict: ``bad``; ``tau``, ``d``; ``c`` (N, 2K + 1) long double and its bound ``e_c``;
    ``shift`` (N,) (None: no candidate).  ``at(m, k)`` gives (cc, e_cc, delay, e_delay) at a shift."""
    filt = np.asarray(filt, dtype=np.float64)
    N = filt.shape[0]
    td = taus(xij, z, fs, N)
    if td is None:
        return dict(bad=True, N=N, K=K)
    tau, d = td
    keep = np.ones(N, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    nS = int(keep.sum())
    y = [shifted(filt[m], s0, W, d[m], K, LD) for m in range(N)]
    b = np.zeros(W, dtype=LD)
    mag = np.zeros(W, dtype=LD)
    for m in range(N):
        if keep[m]:
            b = b + y[m][K]
            mag = mag + np.abs(y[m][K])
    eb = (nS + 1) * U * mag
    c = np.full((N, 2 * K + 1), np.nan, dtype=LD)
    e_c = np.full((N, 2 * K + 1), np.inf, dtype=LD)
    with np.errstate(all='ignore'):
        for m in range(N):
            bm = b - y[m][K] if keep[m] else b
            ab = np.abs(bm)
            Eb = (bm * bm).sum()
            e_Eb = SLACK * W * U * ((ab + eb) ** 2).sum() + (2 * ab * eb + eb * eb).sum()
            ay = np.abs(y[m])
            E = (y[m] * y[m]).sum(axis=1)
            C = (y[m] * bm[None, :]).sum(axis=1)
            e_C = SLACK * W * U * (ay * (ab + eb)[None, :]).sum(axis=1) + (ay * eb[None, :]).sum(axis=1)
            e_E = SLACK * W * U * E
            P = E * Eb
            e_P = (E + e_E) * (Eb + e_Eb) * (1 + U) - P
            R = np.sqrt(P)
            c[m] = C / R
            for i in range(2 * K + 1):
                if not np.isfinite(c[m, i]) or not (P[i] > e_P[i]):
                    continue
                e_R = R[i] - np.sqrt(P[i] - e_P[i]) + U * np.sqrt(P[i] + e_P[i])
                if R[i] > e_R:
                    e_c[m, i] = (abs(C[i]) + e_C[i]) / (R[i] - e_R) * (1 + U) - abs(C[i]) / R[i]
    shift = [pick(c[m], K) for m in range(N)]
    out = dict(bad=False, N=N, K=K, tau=tau, d=d, c=c, e_c=e_c, shift=shift, fs=float(fs))

    def at(m, k):
        i = k + K
        if abs(k) == K:
            f, e_f = LD(0), LD(0)
        else:
            f, e_f = _fraction_ld(c[m, i - 1], c[m, i], c[m, i + 1], e_c[m, i - 1], e_c[m, i], e_c[m, i + 1])
        dl = ((LD(int(d[m]) + k) + f) - LD(tau[m])) / LD(fs)
        e_d = (e_f + U * (abs(int(d[m]) + k) + K + 2)) / LD(fs) + U * abs(dl)
        return c[m, i], e_c[m, i], dl, e_d
    out['at'] = at
    return out


def check_element(ref, m, got_delay, got_cc, got_shift):
    """Judge the GPU's (or (a)'s) three values of element ``m`` against (b)'s unit ``ref`` -> (accepted through a near-tie,
    worst fraction of a bound reached).  Raises AssertionError on a miss."""
    got_delay, got_cc, got_shift = float(got_delay), float(got_cc), int(got_shift)
    if ref['bad'] or ref['shift'][m] is None:
        assert got_shift == 0 and np.isnan(got_cc) and np.isnan(got_delay), (m, got_shift, got_cc, got_delay)
        return False, 0.0
    K, ks = ref['K'], ref['shift'][m]
    assert -K <= got_shift <= K, (m, got_shift)
    tie = got_shift != ks
    if tie:
        c, e = ref['c'][m], ref['e_c'][m]
        assert np.isfinite(c[got_shift + K]), (m, got_shift, ks)
        gap, room = abs(c[got_shift + K] - c[ks + K]), e[got_shift + K] + e[ks + K]
        assert gap < room, 'element %d: shift %d where the truth has %d, c differ by %g, bounds %g' % (m, got_shift, ks, gap, room)
    cc, e_cc, dl, e_d = ref['at'](m, got_shift)
    assert np.isfinite(e_cc), (m, got_shift, 'no bound for cc')
    assert abs(LD(got_cc) - cc) <= e_cc, 'element %d: cc %r, truth %r, bound %g' % (m, got_cc, float(cc), e_cc)
    worst = float(abs(LD(got_cc) - cc) / e_cc) if e_cc > 0 else 0.0
    if np.isfinite(e_d):
        assert abs(LD(got_delay) - dl) <= e_d, 'element %d: delay %r, truth %r, bound %g' % (m, got_delay, float(dl), e_d)
        worst = max(worst, float(abs(LD(got_delay) - dl) / e_d))
    else:
        assert np.isfinite(got_delay), (m, got_delay)
    return tie, worst


def check_units(refs, delay, cc, shift, cap=0.01):
    """``check_element`` over the units ``refs`` and the rows ``delay`` / ``cc`` / ``shift`` (len(refs), N) -> (values,
    accepted through a near-tie, worst fraction of a bound).  At most ``cap`` of the values may be accepted that way."""
    n = ties = 0
    worst = 0.0
    for w, ref in enumerate(refs):
        for m in range(ref['N']):
            t, f = check_element(ref, m, delay[w][m], cc[w][m], shift[w][m])
            n, ties, worst = n + 1, ties + int(t), max(worst, f)
    assert ties <= cap * n, '%d of %d values were accepted through a near-tie: change the input' % (ties, n)
    return n, ties, worst


def row_reference(filt, fs, xij, z, W, inc, nwin, K, dropped=None, first=0):
    """(b) for the windows [first, first + nwin) of one result row -> list of units; ``z`` (>= first + nwin, 2) as fetched,
    ``dropped`` (>= first + nwin,) the dropped masks of a KEPT plan or None."""
    N = np.asarray(filt).shape[0]
    return [unit(filt, fs, xij, z[first + k], (first + k) * int(inc), int(W), int(K),
                 None if dropped is None else kept_bits(dropped[first + k], N)) for k in range(nwin)]


def row64(filt, fs, xij, z, W, inc, nwin, K, dropped=None, first=0):
    """(a) for the same windows -> (delay, cc, shift), (nwin, N) each."""
    N = np.asarray(filt).shape[0]
    out = [unit64(filt, fs, xij, z[first + k], (first + k) * int(inc), int(W), int(K),
                  None if dropped is None else kept_bits(dropped[first + k], N))[:3] for k in range(nwin)]
    return tuple(np.array([o[j] for o in out]) for j in range(3))


def demonstration_statements(kept, full, clean, bad=7, late=0.25, fs=20.0):
    """The statements of DESIGN.md section 23 on the per-element medians (N,) of the three runs (seconds): with KEPT the late
    element within one sample of its lateness and every other |median| below half a sample; without KEPT the others all
    negative, their mean within half a sample of -late / (N - 1); on the clean trace no |median| above half a sample."""
    N = len(kept)
    others = [m for m in range(N) if m != bad]
    assert abs(kept[bad] - late) <= 1.0 / fs, kept[bad]
    assert all(abs(kept[m]) < 0.5 / fs for m in others), kept
    assert all(full[m] < 0.0 for m in others), full
    assert abs(np.mean([full[m] for m in others]) + late / (N - 1)) <= 0.5 / fs, full
    assert all(abs(clean[m]) <= 0.5 / fs for m in range(N)), clean
