"""Several estimators of one trace: ONE multi-estimator call (narrow_band_least_squares_multi) against the sum of the
corresponding single calls, for cfg-2 and cfg-3 at full size with ESTIMATORS = [0.5, 1.0] and [0.5, (1.0, (N-1,))].

    python tools/multi_time.py [reps] [--shapes cfg2,cfg3] [--singles-only] [--label TEXT] [--out FILE]

Per (shape, estimator list): the median whole-call ms of the multi call, the median, minimum and maximum of the sum of
the single calls (the sub-array's single call runs on the reduced stream), and the device pass of both from the
handle's events (set_profiling).  Both forms are warmed first and alternate rep by rep.  --singles-only measures the
single calls alone: that form also runs on a commit that has no multi call (the baseline of the comparison).  One
JSON line per (shape, list); --out appends them to FILE (default profiles/r06_multi_time.jsonl).  The time of
gather_pairs_kernel by itself comes from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python
tools/multi_time.py 3 --shapes cfg3)."""
import contextlib
import io
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit('/', 2)[0])
import narrow_band_least_squares_amd as nbls  # noqa: E402
from narrow_band_least_squares_amd import engine, synthetic  # noqa: E402


def shape(name):
    c = synthetic.build_config(name, 1.0)
    fr = np.logspace(-2, 1, 100)
    w = np.zeros(len(fr))
    args = [c['WINLEN_list'], c['overlap'], None, None, None, None, c['NBANDS'], w, w, c['freqlist'], c['band_type'], fr,
            c['ftype'], c['order'], c['ripple']]
    data = synthetic.plane_wave(synthetic.array_geometry(c['N'], c['radius']), c['npts'], c['fs'], c['fmin'], c['fmax'],
                                timing_error_s=0.25, bad_element=c['N'] - 1, seed=synthetic.SEED + 1)
    return c, args, data


def main():
    argv = sys.argv[1:]
    opts = {'--out': 'profiles/r06_multi_time.jsonl', '--shapes': 'cfg2,cfg3', '--label': ''}
    for key in list(opts):
        if key in argv:
            i = argv.index(key)
            opts[key] = argv[i + 1]
            del argv[i:i + 2]
    singles_only = '--singles-only' in argv
    argv = [a for a in argv if a != '--singles-only']
    reps = int(argv[0]) if argv else 9
    multi_fn = getattr(nbls, 'narrow_band_least_squares_multi', None)
    if multi_fn is None:
        singles_only = True
    h = engine.get_handle()
    lines = []
    for name in opts['--shapes'].split(','):
        c, args, data = shape(name)
        N, rij = c['N'], c['rij']
        full = synthetic.make_stream(data, c['fs'])
        for ests in ([(0.5, ()), (1.0, ())], [(0.5, ()), (1.0, (N - 1,))]):
            subs = []
            for alpha, remove in ests:
                kept = [i for i in range(N) if i not in remove]
                st = full if not remove else synthetic.make_stream(data[kept], c['fs'])
                subs.append((alpha, st, np.ascontiguousarray(rij[:, kept])))

            def singles():
                for alpha, st, r in subs:
                    a = list(args)
                    a[2], a[3] = alpha, st
                    nbls.narrow_band_least_squares(*a, rij=r)

            def multi():
                a = list(args)
                a[2], a[3] = ests, full
                multi_fn(*a, rij=rij)

            def singles_device():
                dev = 0.0
                for alpha, st, r in subs:
                    a = list(args)
                    a[2], a[3] = alpha, st
                    nbls.narrow_band_least_squares(*a, rij=r)
                    dev += h.timings()['total_ms']
                return dev

            with contextlib.redirect_stdout(io.StringIO()):
                for _ in range(3):
                    singles()
                    if not singles_only:
                        multi()
                s_ms, m_ms, s_dev, m_dev = [], [], [], []
                for _ in range(reps):
                    h.set_profiling(False)
                    t = time.perf_counter()
                    singles()
                    s_ms.append((time.perf_counter() - t) * 1e3)
                    if not singles_only:
                        t = time.perf_counter()
                        multi()
                        m_ms.append((time.perf_counter() - t) * 1e3)
                    h.set_profiling(True)
                    s_dev.append(singles_device())
                    if not singles_only:
                        multi()
                        m_dev.append(h.timings()['total_ms'])
                    h.set_profiling(False)
            rec = dict(shape=name, estimators=[[a, list(r)] for a, r in ests], reps=reps, label=opts['--label'],
                       singles_sum_ms=float(np.median(s_ms)), singles_sum_min_ms=float(np.min(s_ms)),
                       singles_sum_max_ms=float(np.max(s_ms)), singles_device_pass_ms=float(np.median(s_dev)))
            if not singles_only:
                rec.update(multi_ms=float(np.median(m_ms)), multi_min_ms=float(np.min(m_ms)), multi_max_ms=float(np.max(m_ms)),
                           multi_device_pass_ms=float(np.median(m_dev)),
                           speedup=float(np.median(s_ms) / np.median(m_ms)))
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if opts['--out']:
        with open(opts['--out'], 'a') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
