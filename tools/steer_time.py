"""The cost of fractional-sample steering (nbls_set_beam_interpolation; csrc/beam.hip, csrc/beam_grid.hip) in a device pass:
the cfg-3 pass (8 elements, 48 bands, W = 1200, half overlap, 69 024 units, LTS 0.5) with the beam and with a 1257-point
slowness grid, each steered by whole samples (taps 0) and through the 8-tap interpolator, from the handle's events
(set_profiling).

    python tools/steer_time.py [reps]

Per sample and element the interpolated instances issue 8 loads and 16 floating-point operations where the whole-sample
ones issue one and two; what that costs is the difference of the passes' solve and total intervals at taps 8 and taps 0 of
the same form.  The four forms alternate rep by rep after a warm-up; one JSON line with the medians, minima and maxima."""
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
    N, npts = len(data), len(data[0])
    edges = [(c['freqlist'][b], c['freqlist'][b + 1]) for b in range(c['NBANDS'])]
    grid = planner.slowness_grid(4.0, 41)
    h = engine.get_handle()
    forms = dict(beam_taps0=dict(want_beam=True), beam_taps8=dict(want_beam=True, beam_taps=8),
                 grid_taps0=dict(slowness_grid=grid), grid_taps8=dict(slowness_grid=grid, beam_taps=8))

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
    rec = dict(shape='cfg3', reps=reps, units=units, elements=N, bands=len(edges), npts=npts, W=W, inc=int(res.inc[0]),
               grid_points=len(grid), taps=8, beam_samples=units * N * W, grid_samples=units * N * W * len(grid))
    for key in forms:
        a = np.array(out[key])
        rec[key] = dict(solve_ms=[float(np.median(a[:, 0])), float(a[:, 0].min()), float(a[:, 0].max())],
                        total_ms=[float(np.median(a[:, 1])), float(a[:, 1].min()), float(a[:, 1].max())])
    for what in ('beam', 'grid'):
        rec[what + '_extra_total_ms'] = rec[what + '_taps8']['total_ms'][0] - rec[what + '_taps0']['total_ms'][0]
        rec[what + '_extra_solve_ms'] = rec[what + '_taps8']['solve_ms'][0] - rec[what + '_taps0']['solve_ms'][0]
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
