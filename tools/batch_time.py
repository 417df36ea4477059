"""Several recordings of one array: a loop of single calls against ONE batch call (narrow_band_least_squares_batch),
for S recordings of cfg-1b shape (OLS, 8 elements, 8 bands, adaptive windows) and of cfg-2 shape (LTS alpha 0.75,
6 elements, 24 bands), every recording with its own trace seed.

    python tools/batch_time.py [reps] [S ...] [--out FILE]

Per (shape, S): the median ms per recording of the loop of single calls and of the batch call, the speed-up, and the
device pass (set_profiling: filter -> solve, summed over the single calls / of the batch pass).  Both forms are warmed
first (the first upload of a process costs 5-9 ms once).  One JSON line per (shape, S); --out writes them to FILE too."""
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit('/', 2)[0])
from narrow_band_least_squares_amd import (engine, synthetic, narrow_band_least_squares,  # noqa: E402
                                           narrow_band_least_squares_batch)


def shape(name):
    c = synthetic.build_config(name, 1.0)
    alpha = 1.0 if name == 'cfg1b' else 0.75
    fr = np.logspace(-2, 1, 1000 if name == 'cfg1b' else 100)
    w = np.zeros(len(fr))
    args = [c['WINLEN_list'], c['overlap'], alpha, None, None, None, c['NBANDS'], w, w, c['freqlist'], c['band_type'], fr,
            c['ftype'], c['order'], c['ripple']]
    return c, args


def streams(c, S):
    out = []
    for s in range(S):
        data = synthetic.plane_wave(synthetic.array_geometry(c['N'], c['radius']), c['npts'], c['fs'], c['fmin'], c['fmax'],
                                    timing_error_s=0.25 if c['alpha'] < 1.0 else 0.0,
                                    bad_element=c['N'] - 1 if c['alpha'] < 1.0 else None, seed=synthetic.SEED + 1 + s)
        out.append(synthetic.make_stream(data, c['fs'], starttime=17884.0729166667 + s / 1440.0))
    return out


def main():
    argv = sys.argv[1:]
    out_path = None
    if '--out' in argv:
        i = argv.index('--out')
        out_path = argv[i + 1]
        del argv[i:i + 2]
    reps = int(argv[0]) if argv else 5
    sizes = [int(a) for a in argv[1:]] or [1, 8, 64, 256]
    h = engine.get_handle()
    lines = []
    for name in ('cfg1b', 'cfg2'):
        c, args = shape(name)
        c['alpha'] = args[2]
        sts_all = streams(c, max(sizes))

        def call(st):
            a = list(args)
            a[3] = st
            return narrow_band_least_squares(*a, rij=c['rij'])

        def batch(sts):
            a = list(args)
            a[3] = sts
            return narrow_band_least_squares_batch(*a, rij=c['rij'])

        import contextlib
        import io
        quiet = contextlib.redirect_stdout(io.StringIO())     # (the BT caution of every call)
        with quiet:
            for _ in range(3):                                # warm both forms
                call(sts_all[0])
                batch(sts_all[:min(8, len(sts_all))])
        for S in sizes:
            sts = sts_all[:S]
            loop_ms, batch_ms, loop_dev, batch_dev = [], [], [], []
            for _ in range(reps):
                with contextlib.redirect_stdout(io.StringIO()):
                    h.set_profiling(False)
                    t = time.perf_counter()
                    for st in sts:
                        call(st)
                    loop_ms.append((time.perf_counter() - t) * 1e3 / S)
                    t = time.perf_counter()
                    batch(sts)
                    batch_ms.append((time.perf_counter() - t) * 1e3 / S)
                    h.set_profiling(True)
                    dev = 0.0
                    for st in sts[:min(S, 16)]:
                        call(st)
                        dev += h.timings()['total_ms']
                    loop_dev.append(dev / min(S, 16))
                    batch(sts)
                    batch_dev.append(h.timings()['total_ms'] / S)
                    h.set_profiling(False)
            rec = dict(shape=name, S=S, reps=reps, single_ms_per_rec=float(np.median(loop_ms)),
                       batch_ms_per_rec=float(np.median(batch_ms)),
                       speedup=float(np.median(loop_ms) / np.median(batch_ms)),
                       single_device_pass_ms=float(np.median(loop_dev)),
                       batch_device_pass_ms_per_rec=float(np.median(batch_dev)),
                       batch_device_pass_ms=float(np.median(batch_dev)) * S)
            print(json.dumps(rec), flush=True)
            lines.append(rec)
    if out_path:
        with open(out_path, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
