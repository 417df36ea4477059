"""The cost of the kept-element results (nbls_set_kept_elements, csrc/kept.hip and the KEPT instances of beam_fstat_kernel and
capon_kernel) in a device pass: the cfg-3 pass (8 elements, 48 bands, W = 1200, 69 024 units, LTS 0.5, element 7 mistimed)
with the beam, and with the Capon spectra over the 41 x 41 grid over +-4 s/km (1257 points) at the default frequencies and
snapshots, each with and without the kept flags, from the handle's events (set_profiling).

    python tools/kept_time.py [reps]

The kernels run behind every unit range's solve, inside the solve interval of nbls_timings: what the feature costs is the
difference of the solve intervals with and without it.  The four forms alternate rep by rep after a warm-up; one JSON line
with the medians, minima and maxima, the share of units with a dropped element and the mean kept count."""
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
    N = len(data)
    edges = [(c['freqlist'][b], c['freqlist'][b + 1]) for b in range(c['NBANDS'])]
    grid = planner.slowness_grid(4.0, 41)
    xij = planner.co_array(c['rij'])[0]
    W = engine.plan_windows(len(data[0]), fs, c['WINLEN_list'], c['overlap'])[0]
    freqs = planner.capon_frequencies(edges)
    Ls, Hs = planner.capon_snapshots(xij, grid, fs, freqs, W)
    capon = dict(capon_grid=grid, capon_freqs=freqs, capon_snapshots=(Ls, Hs))
    h = engine.get_handle()
    forms = dict(beam=dict(want_beam=True), beam_kept=dict(want_beam=True, kept=(N - 1, True, False)),
                 capon=dict(capon), capon_kept=dict(capon, kept=(N - 1, False, True)))

    def run(form):
        res = engine.process(data, fs, t0, c['rij'], edges, c['WINLEN_list'], c['overlap'], c['alpha'], c['ftype'], c['order'],
                             c['ripple'], **forms[form])
        return res, h.timings()

    out = {k: [] for k in forms}
    stats = {}
    with contextlib.redirect_stdout(io.StringIO()):
        for form in list(forms) * 2:
            run(form)
        h.set_profiling(True)
        for _ in range(reps):
            for form in forms:
                res, t = run(form)
                out[form].append((t['solve_ms'], t['total_ms']))
                if res.dropped_mask is not None:
                    computed = np.arange(res.kept_count.shape[1])[None, :] < np.asarray(res.nwin)[:, None]
                    stats[form] = dict(units_with_a_dropped_element=float(np.mean(res.dropped_mask[computed] != 0)),
                                       mean_kept_count=float(np.mean(res.kept_count[computed])))
        h.set_profiling(False)
    rec = dict(shape='cfg3', reps=reps, units=int(res.nwin.sum()), elements=N, grid_points=len(grid), min_pairs=N - 1)
    for key in forms:
        a = np.array(out[key])
        rec[key] = dict(solve_ms=[float(np.median(a[:, 0])), float(a[:, 0].min()), float(a[:, 0].max())],
                        total_ms=[float(np.median(a[:, 1])), float(a[:, 1].min()), float(a[:, 1].max())], **stats.get(key, {}))
    rec['beam_kept_extra_ms'] = rec['beam_kept']['solve_ms'][0] - rec['beam']['solve_ms'][0]
    rec['capon_kept_extra_ms'] = rec['capon_kept']['solve_ms'][0] - rec['capon']['solve_ms'][0]
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
