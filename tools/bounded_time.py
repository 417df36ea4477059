"""The cost of the bounded lag search (nbls_set_lag_limits, csrc/xcorr_bounded.hip) in a device pass: the cfg-3 pass
(8 elements, 48 bands, W = 1200, 69 024 units, LTS 0.5) with and without lag limits at v_min = 0.25 km/s, from the handle's
events (set_profiling), for cfg-3's own geometry (radius 1 km) and for the same coordinates scaled by 0.15.

    python tools/bounded_time.py [reps] [--min-velocity 0.25]

Without limits the pass takes the int8 screening path; with limits every window group runs the bounded-lag correlator
(nbls_timings.xcorr_impl == 4), whose work grows with the limits.  The two passes alternate rep by rep after a warm-up;
one JSON line per geometry with the medians, minima and maxima of the correlation interval and of the whole pass, the
limits (min / median / max), the form, and how many of the full search's picks lie outside the range."""
import contextlib
import io
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from narrow_band_least_squares_amd import engine, planner, synthetic, _hip  # noqa: E402
from narrow_band_least_squares_amd.helpers import get_freqlist, get_winlenlist  # noqa: E402


def main():
    argv = sys.argv[1:]
    vmin = 0.25
    if '--min-velocity' in argv:
        i = argv.index('--min-velocity')
        vmin = float(argv[i + 1])
        del argv[i:i + 2]
    reps = int(argv[0]) if argv else 9
    c = synthetic.CONFIGS['cfg3']
    npts = int(round(c['dur'] * c['fs']))
    freqlist, nbands, _ = get_freqlist(c['fmin'], c['fmax'], c['band_type'], c['B'])
    winlens = get_winlenlist('constant', nbands, c['winlen'], c['winlen'], c['winlen'])
    edges = [(freqlist[b], freqlist[b + 1]) for b in range(nbands)]
    h = engine.get_handle()
    keys = ('xcorr_ms', 'solve_ms', 'total_ms')
    for scale in (1.0, 0.15):
        rij0 = synthetic.array_geometry(c['N'], c['radius']) * scale
        data = synthetic.plane_wave(rij0, npts, c['fs'], c['fmin'], c['fmax'], timing_error_s=0.25, bad_element=c['N'] - 1)
        rows = list(data)
        rij = rij0 - rij0.mean(axis=1, keepdims=True)
        lim = planner.lag_limits(planner.co_array(rij)[0], c['fs'], vmin)

        def run(v, want_lag=False):
            res = engine.process(rows, c['fs'], 0.0, rij, edges, winlens, c['overlap'], c['alpha'], c['ftype'], c['order'],
                                 c['ripple'], min_velocity=v, want_lag=want_lag)
            return res, h.timings()

        out = {False: [], True: []}
        impl = {}
        with contextlib.redirect_stdout(io.StringIO()):
            for b in (False, True):
                run(vmin if b else None)
            h.set_profiling(True)
            for _ in range(reps):
                for b in (False, True):
                    res, t = run(vmin if b else None)
                    out[b].append([t[k] for k in keys])
                    impl[b] = t['xcorr_impl']
            h.set_profiling(False)
            plain = run(None, want_lag=True)[0]
        W = int(plain.W[0])
        computed = np.arange(plain.lag.shape[1])[None, :] < plain.nwin[:, None]
        outside = int(np.count_nonzero((np.abs(plain.lag) > lim[None, None, :]) & computed[:, :, None]))
        rec = dict(radius_km=c['radius'] * scale, min_velocity=vmin, reps=reps, units=int(plain.nwin.sum()), elements=c['N'], W=W,
                   limits_min_median_max=[int(lim.min()), int(np.median(lim)), int(lim.max())],
                   form=_hip.lag_limit_form(c['N'], W, int(lim.min())),
                   full_search_picks_outside_the_range=outside, picks=int(computed.sum()) * len(lim))
        for b, key in ((False, 'plain'), (True, 'bounded')):
            a = np.array(out[b])
            rec[key] = {k: [float(np.median(a[:, i])), float(a[:, i].min()), float(a[:, i].max())] for i, k in enumerate(keys)}
            rec[key]['xcorr_impl'] = int(impl[b])
        rec['bounded_over_plain_xcorr'] = rec['bounded']['xcorr_ms'][0] / rec['plain']['xcorr_ms'][0]
        print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
