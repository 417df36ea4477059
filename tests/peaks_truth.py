"""Plain NumPy restatement of the peak request of the Capon / Bartlett spectra (``nbls_set_capon_peaks``, include/nbls.h;
DESIGN.md section 19): the neighbour table, the peak test, the floor, the ranks and the parabolic offsets, one map at a time,
in the float64 operations the definition names, un-fused.  The GPU's peaks are an exact function of the GPU's own maps, so
everything here is compared with ``==``."""
import numpy as np

DIRS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))


def neighbours(cells):
    """cells (G, 2) int, distinct -> (8, G) int32: the index of the point at ``cells[g] + DIRS[d]``, -1 where there is none."""
    cells = np.asarray(cells, dtype=np.int64)
    where = {(int(i), int(j)): g for g, (i, j) in enumerate(cells)}
    assert len(where) == len(cells), 'two points share a cell'
    nbr = np.full((8, len(cells)), -1, dtype=np.int32)
    for g, (i, j) in enumerate(cells):
        for d, (di, dj) in enumerate(DIRS):
            nbr[d, g] = where.get((int(i) + di, int(j) + dj), -1)
    return nbr


def better(p, g, q, n):
    """"P descending, g ascending" of two candidates (neither NaN)."""
    return p > q or (p == q and g < n)


def fraction(pm, p0, pp):
    """``refine_fraction`` of csrc/refine_fraction.h, float64."""
    pm, p0, pp = np.float64(pm), np.float64(p0), np.float64(pp)
    with np.errstate(all='ignore'):
        nn = pm - pp
        dd = (pm - np.float64(2.0) * p0) + pp
        f = np.float64(0.5) * nn / dd
    if not (np.isfinite(pm) and np.isfinite(p0) and np.isfinite(pp) and dd < 0.0 and np.isfinite(f)) or f == 0.0:
        return 0.0
    return float(min(max(f, -0.5), 0.5))


def peaks(P, cells, K, floor, nbr=None):
    """One map P (G,) on the lattice ``cells`` -> (count, index int32 (K,), power (K,), offset (K, 2))."""
    P = np.asarray(P, dtype=np.float64)
    G = len(P)
    nbr = neighbours(cells) if nbr is None else nbr
    g = np.arange(G)
    peak = ~np.isnan(P)
    for d in range(8):                                               # (the rule of ``better``, all points at once)
        n = nbr[d]
        q = P[np.maximum(n, 0)]
        competes = (n >= 0) & ~np.isnan(q)
        with np.errstate(invalid='ignore'):
            peak &= ~competes | (P > q) | ((P == q) & (g < n))
    found = sorted((int(k) for k in np.flatnonzero(peak)), key=lambda k: (-P[k], k))
    index = np.full(K, -1, dtype=np.int32)
    power = np.full(K, np.nan)
    offset = np.full((K, 2), np.nan)
    if not found:
        return 0, index, power, offset
    top = found[0]
    thr = np.float64(floor) * P[top]
    kept = [g for g in found if g == top or floor == 0 or P[g] >= thr]
    for k, g in enumerate(kept[:K]):
        index[k], power[k] = g, P[g]
        for ax in (0, 1):
            m, p = nbr[2 * ax, g], nbr[2 * ax + 1, g]
            offset[k, ax] = 0.0 if (m < 0 or p < 0) else fraction(P[m], P[g], P[p])
    return len(kept), index, power, offset


def peaks_of_maps(maps, cells, K, floor):
    """maps (n, G) -> (count (n,) int32, index (n, K) int32, power (n, K), offset (n, K, 2))."""
    nbr = neighbours(cells)
    out = [peaks(m, cells, K, floor, nbr) for m in maps]
    return (np.array([o[0] for o in out], dtype=np.int32), np.array([o[1] for o in out], dtype=np.int32).reshape(len(out), K),
            np.array([o[2] for o in out]).reshape(len(out), K), np.array([o[3] for o in out]).reshape(len(out), K, 2))


def same_bits(a, b):
    """Equal as bit patterns (NaN == NaN; 0.0 != -0.0)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
