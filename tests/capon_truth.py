"""Long-double reference of the Capon / Bartlett slowness spectra (``nbls_set_capon``, csrc/capon.hip):
a literal restatement of the definition in ``np.longdouble`` / ``np.clongdouble`` with its own Cholesky and substitution
loops (no LAPACK), in two stages, and the rounding bounds the GPU's float64 results are held to.

Stage A   tables and filtered samples -> R.  With A_i[k] = sum_n |c[n]| |x_i[s0 + k Hs + n]| (|c| the complex modulus):
          either component of a snapshot's X_i[k] is a real dot product of Ls terms, so its error is at most Ls u A_i[k]
          (u = 2^-53, any summation order), the complex error at most sqrt(2) Ls u A_i[k], and |X_i[k]| <= A_i[k]; a product
          X_i conj(X_j) is then off by at most 2 sqrt(2) Ls u A_i A_j, and the 2 K products of a component of R_ij, their
          sum and the division by K add (2 K + 2) u sum_k A_i A_j.  2 sqrt(2) < 4 and 2 K + 2 <= 4 K:
              |dR_ij| <= TOL_A (Ls + K) u (1 / K) sum_k A_i[k] A_j[k]   per component,  TOL_A = 4.
Stage B   the GPU's OWN R -> both spectra, so that the first stage's error does not enter.
          Bartlett: Re(a^H R a) is a sum over the N^2 entries of products of three numbers, |a_i| = 1; no path from an
          entry to the result has more than 4 N + 6 roundings, and taking components for moduli costs a factor 2:
          |dP_B| <= 2 (4 N + 6) u sum |R_ij| / N^2 <= TOL_B N^2 u sum |R_ij| / N^2 for every N >= 3, TOL_B = 4.
          Capon: the computed factor and solve are exact for a perturbed matrix (Higham, Accuracy and Stability, thms 10.3
          and 8.5): y^H y = a^H (R' + E)^-1 a with |E| <= (gamma_{N+1} + 2 gamma_N) |L| |L^H| in real arithmetic, 2 sqrt(2)
          times that in complex, and || |L| |L^H| ||_2 <= N ||R'||_2; the relative change of a^H R'^-1 a is at most
          kappa_2(R') ||E|| / ||R'||: 2 sqrt(2) (3 N + 1) N kappa u <= 275 N kappa u at N <= 32.  The loading's own
          rounding, the reciprocal diagonal, |y|^2 and the final reciprocal add a few u each:
              |dP_C| / P_C <= TOL_C N kappa_2(R') u,  TOL_C = 300.
          R'^-1 is never formed on the GPU; a kernel that formed it would need kappa^2 here.
The constants are derived, not fitted: a ratio |difference| / bound above 1 means that the kernel or the derivation is wrong.
An index is accepted if its power can be the largest within the bounds, and must be the reference's where that one leads by
more than both bounds (grid_truth.check_window's rule)."""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble
U = 2.0 ** -53
TOL_A, TOL_B, TOL_C = 4.0, 4.0, 300.0
TABLE_TOL = 4 * 2.0 ** -52


def tables(xij, grid, fs, freq, Ls, N):
    """The plan's tables as NumPy's float64 expression -> (coef complex128 (Ls,), steer complex128 (G, N))."""
    n = np.arange(int(Ls), dtype=np.float64)
    wf = 2.0 * np.pi * float(freq)
    hann = 0.5 - 0.5 * np.cos((2.0 * np.pi * (n + 0.5)) / float(Ls))
    p = -((wf * n) / float(fs))
    coef = hann * np.cos(p) + 1j * (hann * np.sin(p))
    xij, grid = np.asarray(xij, dtype=np.float64), np.asarray(grid, dtype=np.float64)
    tau = xij[:N - 1, 0][None, :] * grid[:, 0][:, None] + xij[:N - 1, 1][None, :] * grid[:, 1][:, None]
    q = -(wf * tau)
    steer = np.ones((len(grid), N), dtype=np.complex128)
    steer[:, 1:] = np.cos(q) + 1j * np.sin(q)
    return coef, steer


def snapshot_count(W, Ls, Hs):
    return 1 + (int(W) - int(Ls)) // int(Hs)


def csdm_reference(filt, coef, W, inc, nwin, Hs, first=0):
    """Stage A -> (R clongdouble (nwin, N, N), tol float64 (nwin, N, N) per component).  ``coef``: the plan's own table."""
    filt = np.asarray(filt, dtype=np.float64)
    N, Ls = filt.shape[0], len(coef)
    K = snapshot_count(W, Ls, Hs)
    c = np.asarray(coef).astype(CLD)
    cabs = np.abs(c).astype(LD)
    R = np.zeros((nwin, N, N), dtype=CLD)
    tol = np.zeros((nwin, N, N))
    for w in range(nwin):
        s0 = (first + w) * int(inc)
        X = np.zeros((K, N), dtype=CLD)
        A = np.zeros((K, N), dtype=LD)
        for k in range(K):
            seg = filt[:, s0 + k * Hs:s0 + k * Hs + Ls].astype(LD)
            assert seg.shape[1] == Ls and s0 + k * Hs + Ls <= s0 + W
            X[k] = (seg * c[None, :]).sum(axis=1)
            A[k] = (np.abs(seg) * cabs[None, :]).sum(axis=1)
        R[w] = np.einsum('ki,kj->ij', X, np.conj(X)) / LD(K)
        tol[w] = (TOL_A * (Ls + K) * U * (np.einsum('ki,kj->ij', A, A) / LD(K))).astype(np.float64)
    return R, tol


def cholesky(A):
    """Lower Cholesky factor of a Hermitian matrix, long double, plain loops -> (L, ok); ok False: a pivot was not > 0."""
    N = A.shape[0]
    L = np.zeros((N, N), dtype=CLD)
    for j in range(N):
        d = LD(A[j, j].real)
        for k in range(j):
            d -= LD(L[j, k].real) ** 2 + LD(L[j, k].imag) ** 2
        if not d > 0:
            return L, False
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, N):
            s = CLD(A[i, j])
            for k in range(j):
                s -= L[i, k] * np.conj(L[j, k])
            L[i, j] = s / L[j, j]
    return L, True


def spectra_reference(R, steer, loading):
    """Stage B for one window: R (N, N) complex (the GPU's own), steer (G, N) the plan's own table -> dict with
    ``PB``, ``PC`` (G,) long double as float64 views kept in LD, ``tolB``, ``tolC`` (absolute, float64), ``kappa``,
    ``degenerate`` (every result NaN / -1), ``chol_ok``."""
    R = np.asarray(R)
    N, G = R.shape[0], steer.shape[0]
    out = dict(degenerate=False, chol_ok=True, kappa=np.inf)
    Rl = R.astype(CLD)
    t = LD(0)
    for i in range(N):
        t += LD(Rl[i, i].real)
    nan = np.full(G, np.nan)
    if np.isnan(R.real).any() or np.isnan(R.imag).any() or t == 0 or np.isnan(t):
        out.update(degenerate=True, chol_ok=False, PB=nan, PC=nan, tolB=nan, tolC=nan, index_B=-1, index_C=-1)
        return out
    a = np.asarray(steer).astype(CLD)                                # (G, N)
    v = np.zeros((G, N), dtype=CLD)
    for i in range(N):
        for j in range(N):
            v[:, i] += Rl[i, j] * a[:, j]
    PB = np.zeros(G, dtype=LD)
    for i in range(N):
        PB += (np.conj(a[:, i]) * v[:, i]).real
    PB = PB / LD(N * N)
    tolB = np.full(G, TOL_B * N * N * U * float(np.abs(R).sum()) / (N * N))
    Rp = Rl.copy()
    lam = LD(loading) * (t / LD(N))
    for i in range(N):
        Rp[i, i] += lam
    L, ok = cholesky(Rp)
    out['chol_ok'] = ok
    if ok:
        y = np.zeros((G, N), dtype=CLD)
        q = np.zeros(G, dtype=LD)
        for i in range(N):
            s = a[:, i].copy()
            for j in range(i):
                s -= L[i, j] * y[:, j]
            y[:, i] = s / L[i, i]
            q += y[:, i].real ** 2 + y[:, i].imag ** 2
        PC = LD(1) / q
        ev = np.linalg.eigvalsh(Rp.astype(np.complex128))
        kappa = float(ev[-1] / ev[0]) if ev[0] > 0 else np.inf
        out['kappa'] = kappa
        tolC = TOL_C * N * kappa * U * PC.astype(np.float64)
    else:
        PC, tolC = nan, nan
    out.update(PB=PB, PC=PC, tolB=tolB, tolC=tolC, index_B=argmax_total(PB), index_C=argmax_total(PC) if ok else -1)
    return out


def argmax_total(P):
    """The g with the largest P under "P descending, g ascending"; NaN is no candidate; -1 if there is none."""
    P = np.asarray(P, dtype=LD)
    ok = ~np.isnan(P)
    if not ok.any():
        return -1
    return int(np.flatnonzero(ok & (P == P[ok].max()))[0])


def check_spectrum(label, ref_P, tol, ref_index, gpu_index, gpu_power, gpu_map=None):
    """One window, one spectrum: the map within the bound, the power the map's entry, the index admissible -> worst ratio."""
    ref = np.asarray(ref_P, dtype=np.float64)
    worst = 0.0
    if ref_index < 0:
        assert gpu_index == -1 and np.isnan(gpu_power), '%s: %d / %r where the reference has no maximum' % (label, gpu_index, gpu_power)
        if gpu_map is not None:
            assert np.isnan(gpu_map).all(), label
        return worst
    assert 0 <= gpu_index < len(ref), '%s: index %d' % (label, gpu_index)
    if gpu_map is not None:
        diff = np.abs(np.asarray(gpu_map, dtype=LD) - np.asarray(ref_P, dtype=LD)).astype(np.float64)
        worst = float(np.max(diff / tol))
        assert worst <= 1.0, '%s: |map - reference| / bound = %.3g' % (label, worst)
        assert gpu_map[gpu_index] == gpu_power, '%s: the power is not the map\'s entry at the index' % label
    else:
        d = abs(float(gpu_power) - ref[gpu_index]) / tol[gpu_index]
        worst = float(d)
        assert d <= 1.0, '%s: |power - reference| / bound = %.3g' % (label, d)
    # admissible: P(g) can be the largest within the bounds; and the reference's own where that one leads by more
    assert ref[gpu_index] + tol[gpu_index] >= np.max(ref - tol), '%s: index %d cannot be the maximum' % (label, gpu_index)
    others = np.delete(ref + tol, ref_index)
    if len(others) == 0 or ref[ref_index] - tol[ref_index] > others.max():
        assert gpu_index == ref_index, '%s: index %d, the reference leads with %d' % (label, gpu_index, ref_index)
    return worst


# ---- the two-source demonstration ----

def local_maxima(P, shape):
    """Indices (flat, descending power) of the strict-or-equal local maxima of a map on a full Cartesian grid ``shape``
    (8 neighbours; the border compares with what it has)."""
    M = np.asarray(P, dtype=np.float64).reshape(shape)
    pad = np.full((shape[0] + 2, shape[1] + 2), -np.inf)
    pad[1:-1, 1:-1] = M
    peak = np.ones(shape, dtype=bool)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            if di or dj:
                nb = pad[1 + di:1 + di + shape[0], 1 + dj:1 + dj + shape[1]]
                peak &= (M > nb) | ((M == nb) & (di * shape[1] + dj > 0))
    idx = np.flatnonzero(peak.ravel())
    return idx[np.argsort(-M.ravel()[idx], kind='stable')]


def grid_baz(grid, idx):
    s = np.asarray(grid)[idx]
    return np.mod(np.degrees(np.arctan2(s[..., 0], s[..., 1])), 360.0)


def both_found(P, grid, shape, baz_pair, floor=0.25):
    """The two largest local maxima of the map are the two sources: each within a third of their separation in
    back-azimuth of a different source, the second at least ``floor`` of the first."""
    pk = local_maxima(P, shape)
    if len(pk) < 2:
        return False
    P = np.asarray(P, dtype=np.float64)
    if not P[pk[1]] >= floor * P[pk[0]]:
        return False
    sep = abs((baz_pair[0] - baz_pair[1] + 180.0) % 360.0 - 180.0)
    b = grid_baz(grid, pk[:2])

    def near(x, y):
        return abs((x - y + 180.0) % 360.0 - 180.0) <= sep / 3.0
    return (near(b[0], baz_pair[0]) and near(b[1], baz_pair[1])) or (near(b[0], baz_pair[1]) and near(b[1], baz_pair[0]))
