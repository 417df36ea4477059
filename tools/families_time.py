"""The cost of the family labelling (nbls_set_families / nbls_label_families, csrc/families.hip): two records.

    python tools/families_time.py [reps]

1. In a pass: the cfg-3 pass (8 elements, 48 bands, W = 1200, half overlap, 69 024 cells, LTS 0.5) as ONE pass (groups=1)
   without and with the request, from the handle's events (set_profiling).  The eight launches sit behind the pass's last
   solve, ahead of the closing event: what they cost is the difference of the passes' total intervals.  The two forms
   alternate rep by rep after a warm-up; medians, minima and maxima.
2. On a catalogue: nbls_label_families on the grid of 64 recordings of that shape (the pass's own rows repeated, 4.4 M cells):
   the wall time of the whole call — four grids up, eight launches, the labels and the table down — since the call is
   synchronous and carries no events of its own; medians of the same number of reps after a warm-up.
One JSON line."""
import contextlib
import io
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from narrow_band_least_squares_amd import _hip, engine, planner, synthetic  # noqa: E402

PAR = planner.check_families(mdccm_min=0.5, baz_tol=5.0, vel_tol=0.03, vel_min=0.25, vel_max=0.45, band_reach=1, time_reach=1, min_pixels=4)


def stats(a):
    return [float(np.median(a)), float(np.min(a)), float(np.max(a))]


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    c = synthetic.build_config('cfg3', 1.0)
    data, fs, t0 = engine.stream_rows(c['st'])
    edges = [(c['freqlist'][b], c['freqlist'][b + 1]) for b in range(c['NBANDS'])]
    h = engine.get_handle()
    forms = dict(plain={}, families=dict(families=PAR))

    def run(form):
        res = engine.process(data, fs, t0, c['rij'], edges, c['WINLEN_list'], c['overlap'], c['alpha'], c['ftype'], c['order'],
                             c['ripple'], groups=1, **forms[form])
        return res, h.timings()

    out = {k: [] for k in forms}
    with contextlib.redirect_stdout(io.StringIO()):
        for form in list(forms) * 2:
            run(form)
        h.set_profiling(True)
        for _ in range(reps):
            for form in forms:
                res, t = run(form)
                out[form].append(t['total_ms'])
        h.set_profiling(False)
    assert res.families_in_pass
    rec = dict(shape='cfg3', reps=reps, cells=int(res.nwin.sum()), lattice=list(res.vel.shape), families=int(len(res.family_table)),
               eligible=int((res.family != -1).sum()), request=PAR)
    for key in forms:
        rec[key + '_total_ms'] = stats(out[key])
    rec['families_extra_ms'] = rec['families_total_ms'][0] - rec['plain_total_ms'][0]
    S = 64
    grids = [np.ascontiguousarray(np.repeat(g, S, axis=0)) for g in (res.vel, res.baz, res.mdccm)]
    nwin = np.repeat(np.asarray(res.nwin, dtype=np.int32), S)
    p = _hip.family_params(**PAR)
    wall = []
    for k in range(reps + 1):
        t1 = time.perf_counter()
        fam, n, tab = h.label_families(p, S, res.W, res.inc, nwin, *grids)
        if k:
            wall.append(1e3 * (time.perf_counter() - t1))
    assert n == S * rec['families']
    rec['catalogue'] = dict(recordings=S, cells=int(nwin.sum()), lattice=list(grids[0].shape), families=int(n), call_wall_ms=stats(wall),
                            grid_upload_mb=3 * grids[0].nbytes / 1e6)
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
