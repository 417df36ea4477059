"""The cost of the peak request of the Capon / Bartlett spectra (nbls_set_capon_peaks, csrc/capon.hip) in
the cfg-3 pass (8 elements, 48 bands, W = 1200, 69 024 units, LTS 0.5) over the 41 x 41 grid over +-4 s/km (1257 points), K = 4,
floor 0.25, against what a caller did before it existed:

    capon        the spectra alone (peaks off: the kernel instance of the parent commit)
    peaks_lds    with the peaks, the unit's maps in LDS               (option capon_peak_route 1)
    peaks_hbm    with the peaks, the unit's maps in a slab of HBM     (capon_peak_route 2; the default slabs: 4096 here)
    peaks_hbm_256    the same with 256 slabs: one workgroup per CU and launch
    peaks_auto   with the peaks, the route the library chooses
    host         the spectra with both maps kept, the fetch of both maps, and a NumPy pick of the same peaks on the host

    python tools/capon_peaks_time.py [reps]

The forms alternate rep by rep after a warm-up.  solve_ms / total_ms are the handle's events (set_profiling): the device pass,
which for `host` holds neither the fetch nor the pick; wall_ms is the whole call on the host's clock, for `host` up to the
picked peaks.  One JSON line with medians, minima and maxima; the host's pick is checked against the GPU's once."""
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from narrow_band_least_squares_amd import engine, planner, synthetic  # noqa: E402

K, FLOOR = 4, 0.25
DIRS = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (-1, 1), (1, -1), (1, 1))


def neighbours(cells):
    where = {(int(i), int(j)): g for g, (i, j) in enumerate(cells)}
    return np.array([[where.get((int(i) + di, int(j) + dj), -1) for i, j in cells] for di, dj in DIRS])


def host_pick(m, nbr):
    """The K strongest kept peaks of the maps m (n, G), all rows at once -> (count (n,), index (n, K))."""
    g = np.arange(m.shape[1])
    peak = ~np.isnan(m)
    with np.errstate(invalid='ignore'):
        for n in nbr:
            q = m[:, np.maximum(n, 0)]
            peak &= ~((n >= 0)[None, :] & ~np.isnan(q)) | (m > q) | ((m == q) & (g < n)[None, :])
        v = np.where(peak, m, -np.inf)
        top = v.argmax(axis=1)
        kept = peak & ((v >= FLOOR * v.max(axis=1)[:, None]) | (g[None, :] == top[:, None]))
    v = np.where(kept, m, -np.inf)
    index = np.argsort(-v, axis=1, kind='stable')[:, :K]
    count = kept.sum(axis=1)
    return count, np.where(np.arange(K)[None, :] < count[:, None], index, -1)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    c = synthetic.build_config('cfg3', 1.0)
    data, fs, t0 = engine.stream_rows(c['st'])
    edges = [(c['freqlist'][b], c['freqlist'][b + 1]) for b in range(c['NBANDS'])]
    grid = planner.slowness_grid(4.0, 41)
    cells = planner.grid_cells(grid)[0]
    nbr = neighbours(cells)
    xij = planner.co_array(c['rij'])[0]
    W = engine.plan_windows(len(data[0]), fs, c['WINLEN_list'], c['overlap'])[0]
    freqs = planner.capon_frequencies(edges)
    Ls, Hs = planner.capon_snapshots(xij, grid, fs, freqs, W)
    h = engine.get_handle()
    capon = dict(capon_grid=grid, capon_freqs=freqs, capon_snapshots=(Ls, Hs))
    peaks = dict(capon, capon_peaks=K, capon_peak_floor=FLOOR)
    forms = dict(capon=(capon, 0, 0), peaks_lds=(peaks, 1, 0), peaks_hbm_256=(peaks, 2, 256), peaks_hbm=(peaks, 2, 0),
                 peaks_auto=(peaks, 0, 0), host=(dict(capon, want_capon_maps=True), 0, 0))

    def run(form):
        kw, route, slabs = forms[form]
        h.set_option('capon_peak_route', route)
        h.set_option('capon_peak_slabs', slabs)
        t = time.perf_counter()
        res = engine.process(data, fs, t0, c['rij'], edges, c['WINLEN_list'], c['overlap'], c['alpha'], c['ftype'], c['order'],
                             c['ripple'], **kw)
        picked = None
        if form == 'host':
            picked = [[host_pick(m[b, :int(res.nwin[b])], nbr) for b in range(len(res.nwin))] for m in (res.capon_map, res.bartlett_map)]
        wall = (time.perf_counter() - t) * 1e3
        return res, h.timings(), wall, picked

    out = {k: [] for k in forms}
    with contextlib.redirect_stdout(io.StringIO()):
        for form in forms:
            res, _, _, picked = run(form)
            if form == 'peaks_lds':
                gpu = res
            if form == 'host':                           # the host's pick is the GPU's
                for which, name in enumerate(('capon', 'bartlett')):
                    for b in range(len(res.nwin)):
                        n = int(res.nwin[b])
                        assert np.array_equal(picked[which][b][0], getattr(gpu, name + '_peak_count')[b, :n]), (name, b)
                        assert np.array_equal(picked[which][b][1], getattr(gpu, name + '_peak_index')[b, :n]), (name, b)
            del res, picked
        h.set_profiling(True)
        for _ in range(reps):
            for form in forms:
                res, t, wall, _ = run(form)
                out[form].append((t['solve_ms'], t['total_ms'], wall))
                units = int(res.nwin.sum())
                del res
        h.set_profiling(False)
        h.set_option('capon_peak_route', 0)
        h.set_option('capon_peak_slabs', 0)
    rec = dict(shape='cfg3', reps=reps, units=units, elements=len(data), grid_points=len(grid), peaks=K, floor=FLOOR,
               map_bytes_per_spectrum=units * len(grid) * 8)
    for key in forms:
        a = np.array(out[key])
        rec[key] = {name: [float(np.median(a[:, i])), float(a[:, i].min()), float(a[:, i].max())]
                    for i, name in enumerate(('solve_ms', 'total_ms', 'wall_ms'))}
    for key in ('peaks_lds', 'peaks_hbm_256', 'peaks_hbm', 'peaks_auto'):
        rec[key + '_extra_ms'] = rec[key]['solve_ms'][0] - rec['capon']['solve_ms'][0]
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
