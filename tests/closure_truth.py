"""The closure (consistency) of a lag table, by the definition of DESIGN.md section 17 / include/nbls.h, for the tests of
``nbls_set_closure`` (csrc/closure.hip).  CPU only: nothing here imports the GPU library.

Per unit, for N elements and the lexicographic pair list, k(i,j) the index of pair (i, j), i < j:

    c_ijk = (t_ij + t_jk) - t_ik   for i < j < k,        T = N (N-1)(N-2) / 6,   T_m = (N-1)(N-2) / 2
    Q = sum c^2,  E_m = sum over the triplets that contain m of c^2
    consistency = sqrt(Q / T) / fs,  closure_max = max |c| / fs,  element_consistency[m] = sqrt(E_m / T_m) / fs

``closure_int``: t = lag, Python integers, exact.  ``closure_refined``: t = lag + frac in ``np.longdouble`` (64-bit mantissa
on x86: every t, of magnitude below 2^31 with a 53-bit fraction part, and every c is far more accurate than the float64
arithmetic it judges), triplet by triplet in loop order — not the kernel's order.

**Bound of the refined form.**  With u = 2^-53 the kernel's c_ijk is ``fl(fl(t_ij + t_jk) - t_ik)`` on float64 t: two
roundings, the first on a value of magnitude <= 2W, the second <= 3W, so ``|c - c*| <= delta = 5 W u``.  Then
``|c^2 - c*^2| <= 2 |c*| delta + delta^2``, the product's own rounding and the T - 1 additions of the sum, in any order,
are within ``2 T u Q`` (gamma_{T+1} Q with room):

    E_Q  = sum_t (2 |c_t| delta + delta^2) + 2 T u Q_ref        (E_m likewise, with T_m in place of T)
    tol  = (sqrt((Q + E_Q) / T) - sqrt(max(Q - E_Q, 0) / T)) / fs + 4 * 2^-52 * value

the last term for the division, the root and the division by fs (three roundings, one halved by the root).  closure_max
is one c: ``tol = delta / fs + 4 * 2^-52 * value``.  None of these is a measured number."""
import itertools

import numpy as np

U = 2.0 ** -53
REL = 4 * 2.0 ** -52


def pair_index(N):
    return {p: k for k, p in enumerate((i, j) for i in range(N - 1) for j in range(i + 1, N))}


def triplets(N):
    return list(itertools.combinations(range(N), 3))


def closure_int(lag_row, N):
    """One unit's integer lags (P,) -> (Q, cmax, [E_m]) as Python integers, exact."""
    idx = pair_index(N)
    assert len(lag_row) == len(idx)
    Q, cmax, E = 0, 0, [0] * N
    for i, j, k in triplets(N):
        c = (int(lag_row[idx[(i, j)]]) + int(lag_row[idx[(j, k)]])) - int(lag_row[idx[(i, k)]])
        Q += c * c
        cmax = max(cmax, abs(c))
        for m in (i, j, k):
            E[m] += c * c
    return Q, cmax, E


def counts(N):
    return N * (N - 1) * (N - 2) // 6, (N - 1) * (N - 2) // 2


def outputs_int(lag_row, N, fs):
    """The float64 expression of the whole-sample form from the exact integers: (consistency, closure_max, element (N,))
    and the exact Q (for the caller's Q < 2^48 check)."""
    Q, cmax, E = closure_int(lag_row, N)
    T, Tm = counts(N)
    cons = np.sqrt(np.float64(Q) / np.float64(T)) / np.float64(fs)
    el = np.array([np.sqrt(np.float64(e) / np.float64(Tm)) / np.float64(fs) for e in E])
    return cons, np.float64(cmax) / np.float64(fs), el, Q


def outputs_refined(lag_row, frac_row, N, fs, W):
    """The refined form in long double -> dict(cons, cmax, el (N,), tol_cons, tol_cmax, tol_el (N,)) as float64."""
    ld = np.longdouble
    idx = pair_index(N)
    t = np.asarray(lag_row, dtype=ld) + np.asarray(frac_row, dtype=ld)
    delta = ld(5.0 * W * U)
    T, Tm = counts(N)
    Q, EQ, cmax = ld(0), ld(0), ld(0)
    E, EE = [ld(0)] * N, [ld(0)] * N
    for i, j, k in triplets(N):
        c = (t[idx[(i, j)]] + t[idx[(j, k)]]) - t[idx[(i, k)]]
        c2, e = c * c, 2 * abs(c) * delta + delta * delta
        Q, EQ, cmax = Q + c2, EQ + e, max(cmax, abs(c))
        for m in (i, j, k):
            E[m], EE[m] = E[m] + c2, EE[m] + e
    EQ = EQ + 2 * T * ld(U) * Q
    EE = [ee + 2 * Tm * ld(U) * e for ee, e in zip(EE, E)]
    fsl = ld(fs)

    def val_tol(q, eq, n):
        v = np.sqrt(q / n) / fsl
        lo = q - eq if q > eq else ld(0)
        return float(v), float((np.sqrt((q + eq) / n) - np.sqrt(lo / n)) / fsl + REL * v)

    cons, tol_cons = val_tol(Q, EQ, ld(T))
    el, tol_el = zip(*[val_tol(E[m], EE[m], ld(Tm)) for m in range(N)])
    cm = cmax / fsl
    return dict(cons=cons, cmax=float(cm), el=np.array(el), tol_cons=tol_cons, tol_cmax=float(delta / fsl + REL * cm),
                tol_el=np.array(tol_el))


def numpy_lags(win):
    """Full-lag picks of one window (N, W) as the library defines them: lag = W-1-argmax of np.correlate(a, b, 'full')
    -> (P,) int64 in list order."""
    N, W = win.shape
    return np.array([(W - 1) - int(np.argmax(np.correlate(win[i], win[j], 'full')))
                     for i in range(N - 1) for j in range(i + 1, N)], dtype=np.int64)
