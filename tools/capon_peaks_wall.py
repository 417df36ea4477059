"""Where the host's time of a call with a peak request goes (nbls_set_capon_peaks), LDS route against
HBM route: the cfg-3 call of tools/capon_peaks_time.py (G = 1257, K = 4) without profiling, the two routes alternating in three
orders, six repetitions each; every method of the Handle is timed.  Prints per order and route the wall time of every call
and the medians of the methods that take more than 0.3 ms.

    python tools/capon_peaks_wall.py"""
import collections, functools, os, sys, time, contextlib, io
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from narrow_band_least_squares_amd import engine, planner, synthetic, _hip

acc = collections.defaultdict(float)
for name, f in list(vars(_hip.Handle).items()):
    if callable(f) and not name.startswith('__'):
        def wrap(f, name):
            @functools.wraps(f)
            def g(*a, **k):
                t = time.perf_counter()
                try:
                    return f(*a, **k)
                finally:
                    acc[name] += time.perf_counter() - t
            return g
        setattr(_hip.Handle, name, wrap(f, name))

c = synthetic.build_config('cfg3', 1.0)
data, fs, t0 = engine.stream_rows(c['st'])
edges = [(c['freqlist'][b], c['freqlist'][b + 1]) for b in range(c['NBANDS'])]
grid = planner.slowness_grid(4.0, 41)
xij = planner.co_array(c['rij'])[0]
W = engine.plan_windows(len(data[0]), fs, c['WINLEN_list'], c['overlap'])[0]
freqs = planner.capon_frequencies(edges)
Ls, Hs = planner.capon_snapshots(xij, grid, fs, freqs, W)
h = engine.get_handle()
kw = dict(capon_grid=grid, capon_freqs=freqs, capon_snapshots=(Ls, Hs), capon_peaks=4, capon_peak_floor=0.25)
def run(route):
    h.set_option('capon_peak_route', route)
    t = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        engine.process(data, fs, t0, c['rij'], edges, c['WINLEN_list'], c['overlap'], c['alpha'], c['ftype'], c['order'], c['ripple'], **kw)
    return (time.perf_counter() - t) * 1e3
for order in ((1, 2), (2, 1), (1, 1, 2, 2)):
    for r in order: run(r)
    tot = collections.defaultdict(lambda: collections.defaultdict(list)); walls = collections.defaultdict(list)
    for rep in range(6):
        for r in order:
            acc.clear(); w = run(r); walls[r].append(w)
            for k, v in acc.items(): tot[r][k].append(v * 1e3)
    print('order', order)
    for r in sorted(walls):
        print(' route', r, 'wall ms', ' '.join('%.1f' % w for w in walls[r]))
        print('   ', ', '.join('%s %.1f' % (k, np.median(v)) for k, v in sorted(tot[r].items(), key=lambda kv: -np.median(kv[1])) if np.median(v) > 0.3))
