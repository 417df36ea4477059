"""The cost of the Capon / Bartlett spectra (nbls_set_capon, csrc/capon.hip) in a device pass: the cfg-3 pass (8 elements,
48 bands, W = 1200, 69 024 units, LTS 0.5) plain, with the spectra over the 41 x 41 grid over +-4 s/km (1257 points) at the
default frequencies and snapshots, and with the time-domain grid search (nbls_set_beam_grid) over the same grid for
comparison, from the handle's events (set_profiling).

    python tools/capon_time.py [reps]

capon_kernel and beam_grid_kernel run behind every unit range's solve, inside the solve interval of nbls_timings: a kernel's
time is the difference of its solve interval and the plain one.  The three forms alternate rep by rep after a warm-up; one
JSON line with the medians, minima and maxima, the FP64 multiply-adds of the spectra per pass (snapshots N K Ls x 2, the
matrix K N (N + 1) / 2 x 4, the grid G N (N - 1) / 2 x 4 for either spectrum) and the rate they were done at."""
import contextlib
import io
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from narrow_band_least_squares_amd import engine, planner, synthetic  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    c = synthetic.build_config('cfg3', 1.0)
    data, fs, t0 = engine.stream_rows(c['st'])
    edges = [(c['freqlist'][b], c['freqlist'][b + 1]) for b in range(c['NBANDS'])]
    grid = planner.slowness_grid(4.0, 41)
    xij = planner.co_array(c['rij'])[0]
    W = engine.plan_windows(len(data[0]), fs, c['WINLEN_list'], c['overlap'])[0]
    freqs = planner.capon_frequencies(edges)
    Ls, Hs = planner.capon_snapshots(xij, grid, fs, freqs, W)
    h = engine.get_handle()
    forms = dict(plain={}, capon=dict(capon_grid=grid, capon_freqs=freqs, capon_snapshots=(Ls, Hs)), grid=dict(slowness_grid=grid))

    def run(form):
        res = engine.process(data, fs, t0, c['rij'], edges, c['WINLEN_list'], c['overlap'], c['alpha'], c['ftype'], c['order'],
                             c['ripple'], **forms[form])
        return res, h.timings()

    out = {k: [] for k in forms}
    with contextlib.redirect_stdout(io.StringIO()):
        for form in list(forms) * 2:
            run(form)
        h.set_profiling(True)
        for _ in range(reps):
            for form in forms:
                res, t = run(form)
                out[form].append((t['solve_ms'], t['total_ms']))
                if form == 'capon':
                    found = float(np.mean(res.capon_index[res.capon_power != 0] >= 0))
        h.set_profiling(False)
    N, G = res.nchans, len(grid)
    K = 1 + (W - Ls) // Hs
    nwin = np.asarray(res.nwin, dtype=np.float64)
    fma = float(np.sum(nwin * (2.0 * N * K * Ls + 4.0 * K * N * (N + 1) / 2 + 2 * 4.0 * G * N * (N - 1) / 2)))
    rec = dict(shape='cfg3', reps=reps, units=int(res.nwin.sum()), elements=N, grid_points=G, snap_len=[int(Ls.min()), int(Ls.max())],
               snapshots=[int(K.min()), int(K.max())], fp64_fma=fma, index_found=found)
    for key in forms:
        a = np.array(out[key])
        rec[key] = dict(solve_ms=[float(np.median(a[:, 0])), float(a[:, 0].min()), float(a[:, 0].max())],
                        total_ms=[float(np.median(a[:, 1])), float(a[:, 1].min()), float(a[:, 1].max())])
    rec['capon_kernel_ms'] = rec['capon']['solve_ms'][0] - rec['plain']['solve_ms'][0]
    rec['grid_kernel_ms'] = rec['grid']['solve_ms'][0] - rec['plain']['solve_ms'][0]
    rec['capon_fp64_tflops'] = 2.0 * fma / (rec['capon_kernel_ms'] * 1e-3) / 1e12
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
