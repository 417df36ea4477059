"""References of the CLEAN-SC components (``nbls_set_capon_clean``, csrc/capon_clean.hip; the definition is
in include/nbls.h).

(a) ``clean_reference``: the definition restated in float64, operation by operation and in the kernel's order, the scan
    vectorised over the grid.  Where the definition says fma(x, y, z), (a) forms x * y + z in long double and rounds that to
    float64: the product carries 64 bits instead of all 106, so a result can differ from the fused one in its last bit in
    rare cases.  (a) is held to (b)'s bounds, not to the GPU's bits.
(b) ``clean_step``: ONE iteration in long double from a given R_i, so that no error of an earlier iteration enters a later
    bound: the Bartlett spectrum with capon_truth's stage B bound on that R_i, its arg-max, p_i, and R_{i+1} along a given
    g with a bound per entry and component.  With u = 2^-53, |a_k| = 1, A_j = sum_k |R_jk| and c = 2.01 N u >= gamma_2N:
      v    either component of v_j is a real dot product of 2 N terms, accumulated by fma, of |Rr||ar| + |Ri||ai| <=
           |R_jk| each:                                  dv_j <= c A_j            and |v_j| <= A_j
      q    a dot product of 2 N terms of |ar||vr| + |ai||vi| <= |v_j|, plus what dv carries in, (|ar| + |ai|) dv_j <=
           sqrt(2) dv_j:                                 dq <= c sum_j (|v_j| + sqrt(2) dv_j) + sqrt(2) sum_j dv_j
      s    one division:                                 ds <= s u + phi dq / (q (q - dq))
      w    w = v_j conj(v_k), two roundings per component on terms of at most |v_j||v_k| together, plus the inputs' errors:
                                                         dw <= 2 u |v_j||v_k| + sqrt(2) (dv_j |v_k| + dv_k |v_j|) + 2 dv_j dv_k
      R'   one rounding of fma(-w, s, R):                dR'_jk <= u |R'_jk| + |w| ds + dw (s + ds)
    with the moduli of the long-double values and a factor 1.01 on the whole for the second-order terms dropped (dv in |v|
    under c, the long-double arithmetic's own 2^-64).  The constants are derived, not fitted: a ratio above 1 means that
    the kernel or the derivation is wrong.
An index is judged as capon_truth.check_spectrum judges one; a stop decision may differ from (b)'s only where p_i and
f p_0 (or p_i and 0) lie within their bounds of each other (``stop_is_admissible``)."""
import numpy as np

import capon_truth as ct

LD, CLD, U = ct.LD, ct.CLD, ct.U


def _fma(x, y, z):
    return (np.asarray(x, dtype=LD) * np.asarray(y, dtype=LD) + np.asarray(z, dtype=LD)).astype(np.float64)


def kept_rows(dropped, N):
    """``nbls_kept_bits_of``: the kept elements of a unit from its dropped mask, the whole array where fewer than 3 remain."""
    kept = [m for m in range(N) if not (int(dropped) >> m) & 1]
    return kept if len(kept) >= 3 else list(range(N))


def degenerate(R):
    R = np.asarray(R)
    t = 0.0
    for i in range(R.shape[0]):
        t += float(R[i, i].real)
    return bool(np.isnan(R.real).any() or np.isnan(R.imag).any() or t == 0.0 or t != t)


def bartlett_float64(R, steer):
    """P_B(g) of capon_bartlett_point (csrc/capon_point.h) in its order, float64, all g at once."""
    R = np.asarray(R, dtype=np.complex128)
    N = R.shape[0]
    ar, ai = np.ascontiguousarray(steer.real), np.ascontiguousarray(steer.imag)      # (G, N)
    pb = np.zeros(steer.shape[0])
    for i in range(N):
        ur, ui = np.zeros(steer.shape[0]), np.zeros(steer.shape[0])
        for j in range(i):
            rx, ry = R[i, j].real, R[i, j].imag
            ur = _fma(rx, ar[:, j], ur)
            ur = _fma(-ry, ai[:, j], ur)
            ui = _fma(rx, ai[:, j], ui)
            ui = _fma(ry, ar[:, j], ui)
        pb = pb + R[i, i].real * (ar[:, i] * ar[:, i] + ai[:, i] * ai[:, i])
        pb = pb + 2.0 * (ar[:, i] * ur + ai[:, i] * ui)
    return pb / (float(N) * float(N))


def update_float64(R, a, gain):
    """The update of the definition for the steering vector ``a`` (N,) -> (R_{i+1}, q); R_{i+1} None where q stops the loop."""
    N = R.shape[0]
    vr, vi = np.zeros(N), np.zeros(N)
    for k in range(N):
        vr = _fma(R[:, k].real, a[k].real, vr)
        vr = _fma(-R[:, k].imag, a[k].imag, vr)
        vi = _fma(R[:, k].real, a[k].imag, vi)
        vi = _fma(R[:, k].imag, a[k].real, vi)
    q = np.float64(0.0)
    for j in range(N):
        q = _fma(a[j].real, vr[j], q)
        q = _fma(a[j].imag, vi[j], q)
    q = float(q)
    if not q > 0.0 or not np.isfinite(q):
        return None, q
    s = gain / q
    wr = _fma(vi[:, None], vi[None, :], vr[:, None] * vr[None, :])
    wi = _fma(vi[:, None], vr[None, :], -(vr[:, None] * vi[None, :]))
    re, im = _fma(-wr, s, R.real), _fma(-wi, s, R.imag)
    low = np.tril(np.ones((N, N), dtype=bool), -1)
    out = np.where(low, re + 1j * im, 0.0)
    out = out + np.conj(out.T) + np.diag(np.diag(re))
    return out, q


def clean_reference(R, steer, iterations, gain, floor, dropped=0, history=False):
    """(a) for one unit: R (N, N) complex128, steer (G, N) the plan's table -> dict ``count``, ``index`` (I,), ``power`` (I,),
    ``total``, ``residual``, ``R`` (N, N) (scattered back with the kept elements) and, with ``history``, ``steps``: the
    (R_i, P_i, g_i) of every scan."""
    R = np.asarray(R, dtype=np.complex128)
    N, I = R.shape[0], int(iterations)
    rows = kept_rows(dropped, N)
    M = len(rows)
    Rk = R[np.ix_(rows, rows)].copy()
    a = np.asarray(steer)[:, rows]
    out = dict(count=0, index=np.full(I, -1, dtype=np.int32), power=np.full(I, np.nan), total=np.nan, residual=np.nan, R=R.copy(),
               steps=[])
    if degenerate(Rk):
        return out
    t = 0.0
    for i in range(M):
        t += Rk[i, i].real
    out['total'] = t / M
    count, p0 = I, 0.0
    for it in range(I):
        P = bartlett_float64(Rk, a)
        g = ct.argmax_total(P)
        if history:
            out['steps'].append((Rk.copy(), P, g))
        if g < 0 or not P[g] > 0.0:
            count = it
            break
        if it == 0:
            p0 = P[g]
        elif P[g] < floor * p0:
            count = it
            break
        Rn, _ = update_float64(Rk, a[g], gain)
        if Rn is None:
            count = it
            break
        Rk = Rn
        out['index'][it], out['power'][it] = g, gain * P[g]
    tr = 0.0
    for i in range(M):
        tr += Rk[i, i].real
    full = np.zeros((N, N), dtype=np.complex128)
    full[np.ix_(rows, rows)] = Rk
    out.update(count=count, residual=tr / M, R=full)
    return out


def bartlett_longdouble(R, steer):
    """-> (P_B long double (G,), bound float64 (G,)): capon_truth's stage B for the Bartlett spectrum alone."""
    Rl, a = np.asarray(R).astype(CLD), np.asarray(steer).astype(CLD)
    N = Rl.shape[0]
    v = np.zeros(a.shape, dtype=CLD)
    for j in range(N):
        v += a[:, j][:, None] * Rl[:, j][None, :]
    P = (np.conj(a) * v).real.sum(axis=1) / LD(N * N)
    return P, np.full(a.shape[0], ct.TOL_B * N * N * U * float(np.abs(np.asarray(R)).sum()) / (N * N))


def clean_step(R, steer, gain, g=None):
    """(b) one iteration from R (N, N) (already the kept rows) -> dict ``P`` (long double), ``tolP``, ``index`` (the truth's
    arg-max), and along ``g`` (default: the truth's) ``q``, ``R_next`` (clongdouble) and ``tolR`` (float64, per component)."""
    R = np.asarray(R)
    N = R.shape[0]
    P, tolP = bartlett_longdouble(R, steer)
    idx = ct.argmax_total(P)
    out = dict(P=P, tolP=tolP, index=idx, R_next=None, tolR=None, q=None)
    g = idx if g is None else int(g)
    if g < 0:
        return out
    Rl, a = R.astype(CLD), np.asarray(steer)[g].astype(CLD)
    v = Rl @ a
    q = LD((np.conj(a) * v).real.sum())
    out['q'] = q
    if not q > 0:
        return out
    s = LD(gain) / q
    w = v[:, None] * np.conj(v)[None, :]
    out['R_next'] = Rl - w * s
    c = 2.01 * N * U
    A = np.abs(Rl).sum(axis=1).astype(np.float64)
    va = np.abs(v).astype(np.float64)
    dv = c * A
    dq = c * float((va + np.sqrt(2.0) * dv).sum()) + np.sqrt(2.0) * float(dv.sum())
    qf, sf = float(q), float(s)
    ds = sf * U + gain * dq / (qf * (qf - dq)) if qf > dq else np.inf
    dw = 2.0 * U * va[:, None] * va[None, :] + np.sqrt(2.0) * (dv[:, None] * va[None, :] + dv[None, :] * va[:, None]) \
        + 2.0 * dv[:, None] * dv[None, :]
    out['tolR'] = 1.01 * (U * np.abs(out['R_next']).astype(np.float64) + np.abs(w).astype(np.float64) * ds + dw * (sf + ds))
    return out


def stop_is_admissible(i, p, tol, p0, tol0, floor):
    """A stop decision that differs from (b)'s at iteration ``i``: p_i within its bounds of 0, or of f p_0."""
    near_zero = abs(float(p)) <= tol
    near_floor = i > 0 and abs(float(p) - floor * float(p0)) <= tol + floor * tol0
    return bool(near_zero or near_floor)


def check_step(label, R, steer, gain, floor, i, p0, tol0, gpu_stopped, gpu_index, gpu_power, gpu_R_next):
    """One unit, iteration ``i``, from the GPU's own R_i (kept rows): the scan's index and power against (b), the stop decision,
    and R_{i+1} along the GPU's own g within the bound -> dict ``worst`` (ratio of R_{i+1}), ``p`` and ``tol`` (p_i along the
    GPU's path and its bound), ``waived`` (the stop decision differed admissibly; where the GPU went on, its index and its
    update are checked along its own g all the same) and ``tolR`` (None where the GPU stopped)."""
    st = clean_step(R, steer, gain, g=None if gpu_stopped else gpu_index)
    P, tolP, idx = st['P'], st['tolP'], st['index']
    pi = float(P[idx]) if idx >= 0 else np.nan
    truth_stops = idx < 0 or not pi > 0 or (i > 0 and pi < floor * float(p0))
    if gpu_stopped != truth_stops:
        g = idx if gpu_stopped else gpu_index
        assert g >= 0 and stop_is_admissible(i, P[g], tolP[g], p0, tol0, floor), \
            '%s: the GPU %s at iteration %d, p = %r, f p0 = %r' % (label, 'stops' if gpu_stopped else 'goes on', i, pi, floor * float(p0 if p0 is not None else np.nan))
    waived = gpu_stopped != truth_stops
    if gpu_stopped:
        return dict(worst=0.0, p=pi, tol=float(tolP[0]), waived=waived, tolR=None)
    ct.check_spectrum(label, P, tolP, idx, int(gpu_index), float(gpu_power) / gain)
    assert st['R_next'] is not None, '%s: q = %r' % (label, st['q'])
    d = np.asarray(gpu_R_next).astype(CLD) - st['R_next']
    err = np.maximum(np.abs(d.real), np.abs(d.imag)).astype(np.float64)
    ok = st['tolR'] > 0
    worst = float(np.max(err[ok] / st['tolR'][ok])) if ok.any() else 0.0
    assert np.all(err <= st['tolR']), '%s: |R_next - truth| / bound = %.3g' % (label, worst)
    return dict(worst=worst, p=float(P[gpu_index]), tol=float(tolP[gpu_index]), waived=waived, tolR=st['tolR'])


def invariants(label, R_prev, R_next, tolR, eig_bound):
    """Trace non-increasing up to the step's bound, and the smallest eigenvalue >= -``eig_bound``: the entry bounds (both
    components) of every step so far, summed by the caller (a perturbation E moves an eigenvalue by at most ||E||_F <=
    sum |E_jk|), plus N u ||R|| for the eigenvalue routine's own error."""
    tr0, tr1 = float(np.trace(R_prev).real), float(np.trace(R_next).real)
    assert tr1 <= tr0 + float(np.trace(tolR)), '%s: the trace grew from %r to %r' % (label, tr0, tr1)
    ev = np.linalg.eigvalsh(np.asarray(R_next, dtype=np.complex128))
    own = 4 * len(ev) * 2.0 ** -52 * max(abs(ev[0]), abs(ev[-1]))
    assert ev[0] >= -eig_bound - own, '%s: smallest eigenvalue %r below -%r' % (label, ev[0], eig_bound)
