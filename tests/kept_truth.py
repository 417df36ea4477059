"""CPU reference of the kept-element results (``nbls_set_kept_elements``, csrc/kept.hip), written from
the definition in ``include/nbls.h`` and nothing else.

The rule, for one window of an array of N elements with the full lexicographic pair list, k(a, b) the index of pair (a, b),
a < b, and the weights w_k as ``nbls_fetch`` returns them:

    c_m = #{k : pair k holds m and w_k == 0};   m is dropped iff c_m >= q;   dropped_mask: bit m
    kept set: the complement, ascending; the whole array where fewer than 3 elements would remain;  kept_count = M

The kept beam is ``beam_truth`` on the rows e_i with the co-array rows k(e_0, e_i); the kept spectra are
``capon_truth.spectra_reference`` on R[K][:, K] and steer[:, K].  Both inherit those modules' bounds unchanged: the sums are
the same sums over fewer terms."""
import numpy as np

import beam_truth
import capon_truth


def pair_index(N, a, b):
    """k(a, b) of the full lexicographic pair list of N elements, a < b."""
    assert 0 <= a < b < N
    return a * (2 * N - a - 1) // 2 + (b - a - 1)


def pair_list(N):
    return [(a, b) for a in range(N) for b in range(a + 1, N)]


def zero_counts(weights, N):
    """c_m of one window's weights (P,) -> (N,) int."""
    w = np.asarray(weights)
    assert w.shape == (N * (N - 1) // 2,)
    c = np.zeros(N, dtype=np.int64)
    for k, (a, b) in enumerate(pair_list(N)):
        if w[k] == 0:
            c[a] += 1
            c[b] += 1
    return c


def rule(weights, N, q):
    """One window -> (dropped_mask int, kept (M,) ascending int array, M)."""
    assert 1 <= q <= N - 1
    c = zero_counts(weights, N)
    dropped = [m for m in range(N) if c[m] >= q]
    mask = 0
    for m in dropped:
        mask |= 1 << m
    kept = np.array([m for m in range(N) if m not in dropped], dtype=np.int64)
    if len(kept) < 3:
        kept = np.arange(N, dtype=np.int64)
    return mask, kept, len(kept)


def rule_table(weights, N, q):
    """``rule`` over a table of weights (..., P) -> (dropped_mask uint32 (...), kept_count int32 (...))."""
    w = np.asarray(weights)
    lead = w.shape[:-1]
    flat = w.reshape(-1, w.shape[-1])
    mask = np.zeros(len(flat), dtype=np.uint32)
    count = np.zeros(len(flat), dtype=np.int32)
    for i, row in enumerate(flat):
        m, _, M = rule(row, N, q)
        mask[i], count[i] = m, M
    return mask.reshape(lead), count.reshape(lead)


def kept_of_mask(mask, N):
    """The kept set of a dropped mask (the fallback included) -> ascending int array."""
    kept = np.array([m for m in range(N) if not (int(mask) >> m) & 1], dtype=np.int64)
    return kept if len(kept) >= 3 else np.arange(N, dtype=np.int64)


def kept_coarray(xij, N, kept):
    """The co-array rows of the pairs (e_0, e_i), i = 1 .. M-1, of the full array's co-array ``xij`` (P, 2)."""
    xij = np.asarray(xij, dtype=np.float64)
    return np.array([xij[pair_index(N, int(kept[0]), int(e))] for e in kept[1:]]).reshape(len(kept) - 1, 2)


def beam_reference(filt, fs, xij, z, W, inc, w, kept):
    """Window ``w`` of one result row on the kept elements -> ``beam_truth.beam_reference``'s dict of (1,) arrays.
    ``filt`` (N, npts) the full array's rows, ``xij`` its co-array, ``z`` (>= w + 1, 2) the GPU's own slowness."""
    filt = np.asarray(filt, dtype=np.float64)
    return beam_truth.beam_reference(filt[np.asarray(kept)], fs, kept_coarray(xij, filt.shape[0], kept), z, W, inc, 1, first=w)


def spectra_reference(R, steer, loading, kept):
    """One window's spectra on the kept elements: R (N, N) the GPU's own matrix of the full array, steer (G, N) the plan's
    own table -> ``capon_truth.spectra_reference``'s dict."""
    K = np.asarray(kept)
    return capon_truth.spectra_reference(np.asarray(R)[K][:, K], np.asarray(steer)[:, K], loading)
