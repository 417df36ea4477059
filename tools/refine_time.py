"""The cost of the sub-sample lag refinement (nbls_set_lag_refinement, csrc/refine.hip) in a device pass: the cfg-3 pass
(8 elements, 48 bands, W = 1200, 69 024 units, LTS 0.5) with and without it, from the handle's events (set_profiling).

    python tools/refine_time.py [reps] [--shape cfg3]

refine_lag_kernel runs behind every unit batch's verifier, inside the correlation interval of nbls_timings (and inside its
verify_ms on the screening path): its time is the difference of the two correlation intervals.  The two forms alternate
rep by rep after a warm-up; one JSON line with the medians, minima and maxima, the bytes a unit asks for, how many LTS
windows drop another set of pairs under refinement, and the medians of sigma_tau."""
import contextlib
import io
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from narrow_band_least_squares_amd import engine, synthetic  # noqa: E402


def main():
    argv = sys.argv[1:]
    name = 'cfg3'
    if '--shape' in argv:
        i = argv.index('--shape')
        name = argv[i + 1]
        del argv[i:i + 2]
    reps = int(argv[0]) if argv else 9
    c = synthetic.build_config(name, 1.0)
    data, fs, t0 = engine.stream_rows(c['st'])
    edges = [(c['freqlist'][b], c['freqlist'][b + 1]) for b in range(c['NBANDS'])]
    h = engine.get_handle()

    def run(sub):
        res = engine.process(data, fs, t0, c['rij'], edges, c['WINLEN_list'], c['overlap'], c['alpha'], c['ftype'], c['order'],
                             c['ripple'], want_subsample=sub)
        return res, h.timings()

    keys = ('xcorr_ms', 'verify_ms', 'solve_ms', 'total_ms')
    out = {False: [], True: []}
    last = {}
    with contextlib.redirect_stdout(io.StringIO()):
        for sub in (False, True, False, True):
            run(sub)
        h.set_profiling(True)
        for _ in range(reps):
            for sub in (False, True):
                res, t = run(sub)
                out[sub].append([t[k] for k in keys])
                last[sub] = res
        h.set_profiling(False)
    res = last[True]
    units, N, W = int(res.nwin.sum()), res.nchans, int(res.W[0])
    P = N * (N - 1) // 2
    rec = dict(shape=name, reps=reps, units=units, elements=N, pairs=P, W=W, bytes_asked_per_unit=2 * P * W * 8 + P * 4,
               bytes_unique_per_unit=8 * N * W + P * 4, bytes_written_per_unit=8 * P)
    for sub, key in ((False, 'plain'), (True, 'refined')):
        a = np.array(out[sub])
        rec[key] = {k: [float(np.median(a[:, i])), float(a[:, i].min()), float(a[:, i].max())] for i, k in enumerate(keys)}
    rec['kernel_ms'] = rec['refined']['xcorr_ms'][0] - rec['plain']['xcorr_ms'][0]
    computed = np.arange(res.mask.shape[1])[None, :] < res.nwin[:, None]
    if res.lts:
        changed = np.any(last[True].mask != last[False].mask, axis=-1) & computed
        rec['lts_windows_with_another_dropped_set'] = int(changed.sum())
    for sub, key in ((False, 'plain'), (True, 'refined')):
        s = last[sub].sigma_tau[computed]
        rec[key]['sigma_tau_median_s'] = float(np.nanmedian(s))
    rec['quantisation_floor_s'] = 1.0 / (fs * np.sqrt(12.0))
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
