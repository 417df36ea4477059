"""The families of a lattice, from the definition (include/nbls.h), in Python and NumPy.

Shares no code with the package.  Candidates come from a binary search over the other row's doubled centres (not from the
integer division the kernel uses), every candidate pair is put to the four link conditions as they are written, and the
components come from a union-find over the sorted edge list whose representative is the smallest cell.  Everything is
exact: integers, and float64 subtract / abs / compare.
"""
import numpy as np

FIELDS = ('count', 'first_cell', 'peak_cell', 'band_lo', 'band_hi', 'segment', 'sample_first', 'sample_end')


def eligible_cells(par, nwin, vel, baz, mdccm, sigma_tau=None):
    """-> bool (rows, vector_len)."""
    rows, vl = vel.shape
    with np.errstate(invalid='ignore'):
        ok = np.arange(vl)[None, :] < np.asarray(nwin).reshape(rows, 1)
        ok &= np.isfinite(vel) & np.isfinite(baz) & np.isfinite(mdccm)
        ok &= mdccm >= par['mdccm_min']
        ok &= (par['vel_min'] <= vel) & (vel <= par['vel_max'])
        if par.get('sigma_tau_max') is not None:
            ok &= sigma_tau <= par['sigma_tau_max']
    return ok


def values_agree(par, baz_a, vel_a, baz_b, vel_b):
    with np.errstate(invalid='ignore'):                 # (cells that are not eligible may hold anything)
        d = np.abs(baz_a - baz_b)
        d = np.where(d > 180.0, 360.0 - d, d)
        return (d <= par['baz_tol']) & (np.abs(vel_a - vel_b) <= par['vel_tol'])


def edges(par, nseg, winlen, wininc, nwin, vel, baz, mdccm, sigma_tau=None):
    """-> (eligible, edge list int64 (E, 2) with edge[:, 0] > edge[:, 1]), every linked pair once."""
    rows, vl = vel.shape
    nb = rows // nseg
    W = np.asarray(winlen, dtype=np.int64)
    inc = np.asarray(wininc, dtype=np.int64)
    ok = eligible_cells(par, nwin, vel, baz, mdccm, sigma_tau)
    w = np.arange(vl, dtype=np.int64)
    out = []
    for r in range(rows):
        b, s = divmod(r, nseg)
        c2 = 2 * w * inc[b] + W[b]
        for b2 in range(max(0, b - par['band_reach']), b + 1):          # the partner of smaller cell index
            r2 = b2 * nseg + s
            c2o = 2 * w * inc[b2] + W[b2]
            T = 2 * par['time_reach'] * max(inc[b], inc[b2])
            lo = np.searchsorted(c2o, c2 - T, 'left')
            hi = np.searchsorted(c2o, c2 + T, 'right')
            for k in range(int((hi - lo).max()) if vl else 0):
                w2 = lo + k
                m = (w2 < hi) & ok[r]
                w2 = np.minimum(w2, vl - 1)
                m &= ok[r2, w2]
                if r2 == r:
                    m &= w2 < w
                m &= np.abs(c2 - c2o[w2]) <= T
                m &= values_agree(par, baz[r], vel[r], baz[r2, w2], vel[r2, w2])
                if m.any():
                    out.append(np.stack([r * vl + w[m], r2 * vl + w2[m]], axis=1))
    e = np.concatenate(out) if out else np.zeros((0, 2), dtype=np.int64)
    return ok, e


def components(ncells, edge):
    """Union-find over the edges; -> root (ncells,), the smallest cell of every cell's component."""
    parent = list(range(ncells))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b in edge.tolist():
        ra, rb = find(a), find(b)
        if ra != rb:
            if ra < rb:
                parent[rb] = ra
            else:
                parent[ra] = rb
    return np.array([find(x) for x in range(ncells)], dtype=np.int64)


def label(par, nseg, winlen, wininc, nwin, vel, baz, mdccm, sigma_tau=None):
    """-> (family int32 (rows, vector_len), nfamilies, table int64 (nfamilies, 8))."""
    vel, baz, mdccm = (np.asarray(g, dtype=np.float64) for g in (vel, baz, mdccm))
    rows, vl = vel.shape
    ok, e = edges(par, nseg, winlen, wininc, nwin, vel, baz, mdccm, sigma_tau)
    root = components(rows * vl, e)
    cells = np.flatnonzero(ok.reshape(-1))
    family = np.full(rows * vl, -1, dtype=np.int32)
    if cells.size == 0:
        return family.reshape(rows, vl), 0, np.zeros((0, 8), dtype=np.int64)
    order = np.argsort(root[cells], kind='stable')
    mem = cells[order]                                  # members, family after family in ascending root, ascending inside
    rt = root[mem]
    start = np.flatnonzero(np.r_[True, rt[1:] != rt[:-1]])
    count = np.diff(np.r_[start, mem.size])
    keep = count >= par['min_pixels']
    fid = np.where(keep, np.cumsum(keep) - 1, -2)
    family[mem] = np.repeat(fid, count)
    r = mem // vl
    band = r // nseg
    s0 = (mem % vl) * np.asarray(wininc, dtype=np.int64)[band]
    end = s0 + np.asarray(winlen, dtype=np.int64)[band]
    md = mdccm.reshape(-1)[mem]
    top = np.repeat(np.maximum.reduceat(md, start), count)
    peak = np.minimum.reduceat(np.where(md == top, mem, rows * vl), start)
    table = np.stack([count, mem[start], peak, np.minimum.reduceat(band, start), np.maximum.reduceat(band, start), r[start] % nseg,
                      np.minimum.reduceat(s0, start), np.maximum.reduceat(end, start)], axis=1).astype(np.int64)
    return family.reshape(rows, vl), int(keep.sum()), table[keep]
