"""Truth of the eigenvalues and the MUSIC pseudo-spectrum (``nbls_set_capon_music``, csrc/capon_music.hip; DESIGN.md section 25;
the definition is in include/nbls.h).

``jacobi`` is a row-cyclic Jacobi method in long double (x86 80-bit, u_l = 2^-64), written from the definition's rotation and
run to off(A) <= 2^-60 ||R||_F; there is no LAPACK in it.  ``music`` makes of it the eigenvalues, the noise projector, D(g)
over the grid, M by the rho rule and the arg-max.  The truth's own error, at 2^-64 per rounding, is 2^-11 of the kernel's and
is ignored.

The bounds (derived, none fitted; u = 2^-53, S = NBLS_MUSIC_SWEEP_CAP):
  Jacobi       one computed rotation applied to a pair of rows or columns x gives J~ (x + e) with J~ exactly unitary: every
               component is a chain of three fma (3 u of the moduli, 4 real components: 8 u |x| with the moduli's sqrt(2)
               taken in) and c, sigma carry 10 u between them (g 3, tau 3, t 3, c 3, s 1, sigma 2 roundings, each half or
               less of a relative u in c or sigma): 18 u |x|.  A two-sided rotation touches two rows and two columns, at most
               2 * 18 u ||A||_F, and the closed form of its own block is the same rotation with fewer roundings: c_J = 40
               covers both.  ||A||_F = ||R||_F throughout, to first order.  The diagonal is read when off(A) <= 2^-46 ||R||_F:
                   ||E||_F <= (c_J S N (N - 1) / 2 u + 2^-46) ||R||_F         lambda^ and E^ are exact for R + E
  eigenvalues  Weyl: |lambda^_k - lambda_k| <= ||E||_2 <= ||E||_F.
  vectors      E^ is a product of rotations applied from the right alone, 18 u on two columns of norm sqrt(2) (1 + ...):
                   ||dE||_F <= 1.01 * 18 sqrt(2) S N (N - 1) / 2 u;   ||E^H E - I||_F <= 2.01 ||dE||_F;
                   ||R E^ - E^ L^||_F <= ||E||_F + 2 ||R||_F ||dE||_F
  projector    Davis-Kahan: ||P^_n - P_n||_2 <= 2 ||E||_2 / gap, gap = lambda_M - lambda_{M+1}, plus 2.01 ||dE||_F for the
               columns' own departure from orthonormal.  a^H a = N, so |D^ - D| <= that, plus the scan's own
               (N - M) (4 N + 8) u: z is two real dot products of 2 N terms by fma on |e_ik| each, |z_k| <= sqrt(N), sum
               |e_ik| <= sqrt(N), and 2 (N - M) + 2 roundings of the sum and the division on D <= 1.
D = 1 / P is compared, never P: P's relative error is |dD| / D and has no bound at a source."""
import numpy as np

import capon_truth as ct

LD, CLD, U = ct.LD, ct.CLD, ct.U
SWEEP_CAP = 24
STOP = 2.0 ** -46
C_J = 40.0


def degenerate(R):
    R = np.asarray(R)
    t = 0.0
    for i in range(R.shape[0]):
        t += float(R[i, i].real)
    return bool(np.isnan(R.real).any() or np.isnan(R.imag).any() or t == 0.0 or t != t)


def _off(A):
    return np.sqrt((np.abs(A - np.diag(np.diag(A))) ** 2).sum())


def jacobi(R, stop=LD(2.0) ** -60, cap=60):
    """R (N, N) Hermitian -> (lambda long double (N,) descending, E clongdouble (N, N) with column k beside lambda_k, sweeps).
    Row-cyclic, the stable rotation t = sign(tau) / (|tau| + sqrt(1 + tau^2))."""
    A = np.asarray(R).astype(CLD)
    N = A.shape[0]
    A = (A + np.conj(A.T)) / LD(2)
    E = np.eye(N, dtype=CLD)
    nrm = np.sqrt((np.abs(A) ** 2).sum())
    sweeps = 0
    while _off(A) > stop * nrm:
        assert sweeps < cap, 'the truth did not converge'
        for p in range(N - 1):
            for q in range(p + 1, N):
                x = A[p, q]
                g = np.abs(x)
                if g == 0:
                    continue
                tau = (A[q, q].real - A[p, p].real) / (LD(2) * g)
                t = (LD(1) if tau >= 0 else LD(-1)) / (np.abs(tau) + np.sqrt(LD(1) + tau * tau))
                c = LD(1) / np.sqrt(LD(1) + t * t)
                sg = (t * c) * (x / g)
                Ap, Aq = A[:, p].copy(), A[:, q].copy()              # A J
                A[:, p], A[:, q] = c * Ap - np.conj(sg) * Aq, sg * Ap + c * Aq
                Ap, Aq = A[p, :].copy(), A[q, :].copy()              # J^H (A J)
                A[p, :], A[q, :] = c * Ap - sg * Aq, np.conj(sg) * Ap + c * Aq
                A[p, q] = A[q, p] = 0
                A[p, p], A[q, q] = A[p, p].real, A[q, q].real
                Ep, Eq = E[:, p].copy(), E[:, q].copy()
                E[:, p], E[:, q] = c * Ep - np.conj(sg) * Eq, sg * Ep + c * Eq
        sweeps += 1
    lam = np.diag(A).real.astype(LD)
    order = sorted(range(N), key=lambda i: (-lam[i], i))
    return lam[order], E[:, order], sweeps


def sources_by_floor(lam, rho):
    """The rho rule on float64 eigenvalues, the kernel's one multiplication: clamp(#{k : lambda_k >= rho lambda_1}, 1, N - 1)."""
    lam = np.asarray(lam, dtype=np.float64)
    return int(min(max(int(np.sum(lam >= np.float64(rho) * lam[0])), 1), len(lam) - 1))


def argmin_total(D):
    """The arg-max of P = 1 / D under "P descending, g ascending": the smallest D, of equal ones the lowest g; NaN is none."""
    D = np.asarray(D)
    ok = ~np.isnan(D)
    if not ok.any():
        return -1
    return int(np.flatnonzero(ok & (D == D[ok].min()))[0])


def music(R, steer, sources, eig_floor=0.05):
    """One unit: R (N, N), steer (G, N) the plan's table -> dict ``lam`` (N,), ``E`` (N, N), ``sweeps``, ``M``, ``gap``
    (lambda_M - lambda_{M+1}, float), ``Pn`` (the noise projector), ``D`` long double (G,), ``index``."""
    lam, E, sweeps = jacobi(R)
    N = len(lam)
    M = int(sources) if sources else sources_by_floor(lam.astype(np.float64), eig_floor)
    return dict(lam=lam, E=E, sweeps=sweeps, **spectrum(lam, E, steer, M))


def spectrum(lam, E, steer, M):
    """D(g) = a^H P_n a / N with the noise projector of the columns beyond M -> dict ``M``, ``gap``, ``Pn``, ``D``, ``index``."""
    N = len(lam)
    En = E[:, M:]
    a = np.asarray(steer).astype(CLD)
    z = a @ np.conj(En)                                              # (G, N - M): e_k^H a
    D = (np.abs(z) ** 2).sum(axis=1) / LD(N)
    return dict(M=M, gap=float(lam[M - 1] - lam[M]), Pn=En @ np.conj(En.T), D=D, index=argmin_total(D))


def bounds(R, M=None, gap=None):
    """-> dict ``E`` (||E||_F), ``lam`` (per eigenvalue), ``dE`` (||dE||_F), ``orth`` (||E^H E - I||_F), ``resid``
    (||R E^ - E^ L^||_F) and, given M and the truth's gap, ``D``."""
    R = np.asarray(R)
    N = R.shape[0]
    nrm = float(np.sqrt((np.abs(R.astype(CLD)) ** 2).sum()))
    rot = SWEEP_CAP * N * (N - 1) / 2.0
    eE = (C_J * rot * U + STOP) * nrm
    dE = 1.01 * 18.0 * np.sqrt(2.0) * rot * U
    out = dict(E=eE, lam=eE, dE=dE, orth=2.01 * dE, resid=eE + 2.0 * nrm * dE)
    if M is not None:
        out['D'] = 2.0 * eE / gap + 2.01 * dE + (N - M) * (4.0 * N + 8.0) * U if gap > 0 else np.inf
    return out
