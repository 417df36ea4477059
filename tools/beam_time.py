"""The cost of the beam results (nbls_set_beam, csrc/beam.hip) in a device pass: the cfg-3 pass (8 elements, 48 bands,
W = 1200, 69 024 units, LTS 0.5) with and without them, from the handle's events (set_profiling).

    python tools/beam_time.py [reps] [--shape cfg3]

beam_fstat_kernel runs behind every unit range's solve, inside the solve interval of nbls_timings: its time is the
difference of the two solve intervals.  The two forms alternate rep by rep after a warm-up; one JSON line with the
medians, minima and maxima."""
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
    reps = int(argv[0]) if argv else 7
    c = synthetic.build_config(name, 1.0)
    data, fs, t0 = engine.stream_rows(c['st'])
    edges = [(c['freqlist'][b], c['freqlist'][b + 1]) for b in range(c['NBANDS'])]
    h = engine.get_handle()

    def run(beam):
        res = engine.process(data, fs, t0, c['rij'], edges, c['WINLEN_list'], c['overlap'], c['alpha'], c['ftype'], c['order'],
                             c['ripple'], want_beam=beam)
        return res, h.timings()

    out = {False: [], True: []}
    with contextlib.redirect_stdout(io.StringIO()):
        for beam in (False, True, False, True):
            run(beam)
        h.set_profiling(True)
        for _ in range(reps):
            for beam in (False, True):
                res, t = run(beam)
                out[beam].append((t['solve_ms'], t['total_ms']))
        h.set_profiling(False)
    units, N, W = int(res.nwin.sum()), res.nchans, int(res.W[0])
    rec = dict(shape=name, reps=reps, units=units, elements=N, W=W, bytes_read_per_unit=8 * N * W, bytes_written_per_unit=16,
               fstat_median=float(np.nanmedian(res.fstat[res.fstat != 0])))
    for beam, key in ((False, 'plain'), (True, 'beam')):
        a = np.array(out[beam])
        rec[key] = dict(solve_ms=[float(np.median(a[:, 0])), float(a[:, 0].min()), float(a[:, 0].max())],
                        total_ms=[float(np.median(a[:, 1])), float(a[:, 1].min()), float(a[:, 1].max())])
    rec['kernel_ms'] = rec['beam']['solve_ms'][0] - rec['plain']['solve_ms'][0]
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
