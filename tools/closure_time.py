"""The cost of the closure results (nbls_set_closure, csrc/closure.hip) in a device pass: the cfg-3 pass (8 elements, 48
bands, W = 1200, 69 024 units, LTS 0.5) with and without them, from the handle's events (set_profiling), and the same once
on a cfg-5-shaped plan (32 elements: 4960 triplets per unit).

    python tools/closure_time.py [reps] [--shape cfg3] [--scale 1.0] [--subsample]

closure_kernel runs behind every unit range's solve, inside the solve interval of nbls_timings: its time is the difference
of the two solve intervals.  The two forms alternate rep by rep after a warm-up; one JSON line with the medians, minima and
maxima.  --subsample: both forms on a plan with lag refinement (the double instance of the kernel)."""
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
    name, scale = 'cfg3', 1.0
    if '--shape' in argv:
        i = argv.index('--shape')
        name = argv[i + 1]
        del argv[i:i + 2]
    if '--scale' in argv:
        i = argv.index('--scale')
        scale = float(argv[i + 1])
        del argv[i:i + 2]
    refined = '--subsample' in argv
    if refined:
        argv.remove('--subsample')
    reps = int(argv[0]) if argv else 9
    c = synthetic.build_config(name, scale)
    data, fs, t0 = engine.stream_rows(c['st'])
    edges = [(c['freqlist'][b], c['freqlist'][b + 1]) for b in range(c['NBANDS'])]
    h = engine.get_handle()

    def run(closure):
        res = engine.process(data, fs, t0, c['rij'], edges, c['WINLEN_list'], c['overlap'], c['alpha'], c['ftype'], c['order'],
                             c['ripple'], want_subsample=refined, want_consistency=closure)
        return res, h.timings()

    out = {False: [], True: []}
    with contextlib.redirect_stdout(io.StringIO()):
        for closure in (False, True, False, True):
            run(closure)
        h.set_profiling(True)
        for _ in range(reps):
            for closure in (False, True):
                res, t = run(closure)
                out[closure].append((t['solve_ms'], t['total_ms']))
        h.set_profiling(False)
    units, N = int(res.nwin.sum()), res.nchans
    P = N * (N - 1) // 2
    rec = dict(shape=name, scale=scale, refined=refined, reps=reps, units=units, elements=N, W=int(res.W[0]),
               triplets=N * (N - 1) * (N - 2) // 6, bytes_read_per_unit=(12 if refined else 4) * P,
               bytes_written_per_unit=16 + 8 * N,
               consistency_median_s=float(np.median(res.consistency[res.consistency != 0])) if res.consistency.any() else 0.0)
    for closure, key in ((False, 'plain'), (True, 'closure')):
        a = np.array(out[closure])
        rec[key] = dict(solve_ms=[float(np.median(a[:, 0])), float(a[:, 0].min()), float(a[:, 0].max())],
                        total_ms=[float(np.median(a[:, 1])), float(a[:, 1].min()), float(a[:, 1].max())])
    rec['kernel_ms'] = rec['closure']['solve_ms'][0] - rec['plain']['solve_ms'][0]
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
