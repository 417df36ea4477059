"""The cost of a coarse slowness grid with refinement (nbls_set_beam_grid_refinement; csrc/beam_grid_refine.hip) against the
fine grid it replaces, in a device pass: the cfg-3 pass (8 elements, 48 bands, W = 1200, half overlap, 69 024 units, LTS 0.5)
steered through the 8-tap interpolator with the 1257-point grid ``slowness_grid(4.0, 41)`` alone, the 317-point grid
``slowness_grid(4.0, 21)`` alone, and the 317-point grid with 4 levels (317 + 32 evaluations per window), from the handle's
events (set_profiling), by the method of tools/steer_time.py.

    python tools/grid_refine_time.py [reps] [--parent]

What the refinement adds is reported as the difference of the median solve intervals of the 317-point pass with and without
it (the handle has no event pair around the kernel).
The forms alternate rep by rep after a warm-up; one JSON line with the medians, minima and maxima, the halo of the refining
plan and which form of the kernel ran.  ``--parent``: only the 1257-point grid, for a library without the refinement."""
import contextlib
import io
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from narrow_band_least_squares_amd import _hip, engine, planner, synthetic  # noqa: E402

LEVELS = 4


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    parent = '--parent' in sys.argv[1:]
    reps = int(args[0]) if args else 7
    c = synthetic.build_config('cfg3', 1.0)
    data, fs, t0 = engine.stream_rows(c['st'])
    N, npts = len(data), len(data[0])
    edges = [(c['freqlist'][b], c['freqlist'][b + 1]) for b in range(c['NBANDS'])]
    fine, coarse = planner.slowness_grid(4.0, 41), planner.slowness_grid(4.0, 21)
    h = engine.get_handle()
    forms = dict(grid1257=dict(slowness_grid=fine, beam_taps=8))
    if not parent:
        forms.update(grid317=dict(slowness_grid=coarse, beam_taps=8),
                     grid317_refined=dict(slowness_grid=coarse, beam_taps=8, grid_refine=LEVELS))

    def run(form):
        res = engine.process(data, fs, t0, c['rij'], edges, c['WINLEN_list'], c['overlap'], c['alpha'], c['ftype'], c['order'],
                             c['ripple'], **forms[form])
        return res, h.timings()

    out = {k: [] for k in forms}
    with contextlib.redirect_stdout(io.StringIO()):
        for form in forms:
            run(form)
        h.set_profiling(True)
        for _ in range(reps):
            for form in forms:
                res, t = run(form)
                out[form].append((t['solve_ms'], t['total_ms']))
        h.set_profiling(False)
    W = int(res.W[0])
    units = int(res.nwin.sum())
    rec = dict(shape='cfg3', reps=reps, units=units, elements=N, bands=len(edges), npts=npts, W=W, inc=int(res.inc[0]), taps=8,
               points=dict(grid1257=len(fine), grid317=len(coarse)), levels=LEVELS)
    for key in forms:
        a = np.array(out[key])
        rec[key] = dict(solve_ms=[float(np.median(a[:, 0])), float(a[:, 0].min()), float(a[:, 0].max())],
                        total_ms=[float(np.median(a[:, 1])), float(a[:, 1].min()), float(a[:, 1].max())])
    if not parent:
        # the halo of the last plan (the refining one): the grid's from the plan's own table n = floor(tau) and its taps, the
        # reach of the step by the expression of include/nbls.h
        step = planner.grid_cells(coarse)[1]
        xr = np.abs(np.asarray(res.xij)[:N - 1])
        n, K = h.fetch_beam_grid_delays().astype(np.int64), h.taps // 2
        grid_halo = int(max(np.abs(n - K + 1).max(), np.abs(n + K).max()))
        halo = grid_halo + int(np.ceil(fs * np.max(xr[:, 0] * step[0] + xr[:, 1] * step[1]))) + 1
        lds = _hip.load_library().nbls_beam_grid_refine_lds_bytes(N, W, halo)
        rec.update(refine_halo=halo, refine_lds_bytes=lds, refine_form='LDS' if lds > 0 else 'global',
                   refine_extra_solve_ms=rec['grid317_refined']['solve_ms'][0] - rec['grid317']['solve_ms'][0],
                   refined_against_fine_total_ms=rec['grid317_refined']['total_ms'][0] - rec['grid1257']['total_ms'][0])
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
