"""The cost of the seeded lag search (nbls_set_lag_seed, csrc/xcorr_seeded.hip) in a device pass: the cfg-3 pass
(8 elements, 48 bands, W = 1200, 69 024 units, LTS 0.5) in three configurations — plain, with the 41 x 41 slowness grid over
+-4 s/km (1257 points), and with that grid plus the seed at K = 18 samples in every band — from the handle's events
(set_profiling), for cfg-3's own geometry (radius 1 km) and for the same coordinates scaled by 0.15.

    python tools/seeded_time.py [reps] [--halfwidth 18]

Without a seed the pass takes the int8 screening path and the grid kernel runs behind the solve, inside the solve interval;
with the seed every window group runs the grid kernel and then the seeded correlator in the correlation stage
(nbls_timings.xcorr_impl == 5): the grid kernel's time moves from the solve interval into xcorr_ms.  The three passes
alternate rep by rep after a warm-up; one JSON line per geometry with the medians, minima and maxima of the correlation
interval, the solve interval and the whole pass, the form, the correlator's own time (the seeded pass's xcorr_ms less the
grid kernel's, which is the difference of the other two solve intervals) and the two bounds of the staged form: two 8-byte
LDS reads per multiply-add at 256 B/clk/CU, and one FP64 FMA per multiply-add at 64 lanes/clk/CU, 256 CUs at 2.4 GHz."""
import contextlib
import io
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from narrow_band_least_squares_amd import engine, planner, synthetic, _hip  # noqa: E402
from narrow_band_least_squares_amd.helpers import get_freqlist, get_winlenlist  # noqa: E402

CUS, CLK = 256, 2.4e9


def main():
    argv = sys.argv[1:]
    K = 18
    if '--halfwidth' in argv:
        i = argv.index('--halfwidth')
        K = int(argv[i + 1])
        del argv[i:i + 2]
    reps = int(argv[0]) if argv else 9
    c = synthetic.CONFIGS['cfg3']
    npts = int(round(c['dur'] * c['fs']))
    freqlist, nbands, _ = get_freqlist(c['fmin'], c['fmax'], c['band_type'], c['B'])
    winlens = get_winlenlist('constant', nbands, c['winlen'], c['winlen'], c['winlen'])
    edges = [(freqlist[b], freqlist[b + 1]) for b in range(nbands)]
    grid = planner.slowness_grid(4.0, 41)
    h = engine.get_handle()
    keys = ('xcorr_ms', 'solve_ms', 'total_ms')
    names = ('plain', 'grid', 'seeded')
    for scale in (1.0, 0.15):
        rij0 = synthetic.array_geometry(c['N'], c['radius']) * scale
        data = synthetic.plane_wave(rij0, npts, c['fs'], c['fmin'], c['fmax'], timing_error_s=0.25, bad_element=c['N'] - 1)
        rows = list(data)
        rij = rij0 - rij0.mean(axis=1, keepdims=True)

        def run(name):
            res = engine.process(rows, c['fs'], 0.0, rij, edges, winlens, c['overlap'], c['alpha'], c['ftype'], c['order'],
                                 c['ripple'], slowness_grid=None if name == 'plain' else grid,
                                 seed_halfwidths=K if name == 'seeded' else None)
            return res, h.timings()

        out = {n: [] for n in names}
        impl = {}
        with contextlib.redirect_stdout(io.StringIO()):
            for n in names:
                run(n)
            h.set_profiling(True)
            for _ in range(reps):
                for n in names:
                    res, t = run(n)
                    out[n].append([t[k] for k in keys])
                    impl[n] = t['xcorr_impl']
            h.set_profiling(False)
        W, N, P = int(res.W[0]), c['N'], c['N'] * (c['N'] - 1) // 2
        units = int(res.nwin.sum())
        rec = dict(radius_km=c['radius'] * scale, halfwidth=K, reps=reps, units=units, elements=N, W=W, grid_points=len(grid),
                   form=_hip.lag_seed_form(N, W, K, 0))
        for n in names:
            a = np.array(out[n])
            rec[n] = {k: [float(np.median(a[:, i])), float(a[:, i].min()), float(a[:, i].max())] for i, k in enumerate(keys)}
            rec[n]['xcorr_impl'] = int(impl[n])
        grid_ms = rec['grid']['solve_ms'][0] - rec['plain']['solve_ms'][0]
        rec['grid_kernel_ms'] = grid_ms
        rec['seeded_correlator_ms'] = rec['seeded']['xcorr_ms'][0] - grid_ms
        # multiply-adds of the seeded correlator: at most (2K + 1) lags of about W terms per (unit, pair)
        fma = float(units) * P * (2 * K + 1) * W
        rec['multiply_adds'] = fma
        rec['lds_bound_ms'] = fma * 16 / (256.0 * CUS * CLK) * 1e3
        rec['fp64_bound_ms'] = fma / (64.0 * CUS * CLK) * 1e3
        rec['fraction_of_lds_bound'] = rec['lds_bound_ms'] / rec['seeded_correlator_ms']
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
