"""The cost of the eigenvalues and the MUSIC spectrum (nbls_set_capon_music, csrc/capon_music.hip) in a device pass: the cfg-3
pass (8 elements, 48 bands, W = 1200, 69 024 units, LTS 0.5) with the Capon spectra alone over planner.slowness_grid(4.0, 41)
— the 1257 points of a 41 x 41 lattice over +-4 s/km that lie within 4 s/km of the origin —, with MUSIC of M = 2, with M by
the floor rho = 0.05, with M = 2 and its K = 4 peaks (beside the spectra with their own K = 4 peaks, whose request the MUSIC
peaks use), and with CLEAN-SC of I = 16 iterations beside it, from the handle's events (set_profiling).

    python tools/capon_music_time.py [reps]

capon_music_kernel runs behind capon_kernel inside the solve interval of nbls_timings: its time is the difference of the
form's solve interval and that of the spectra alone (with peaks: of the spectra with their peaks).  The forms alternate rep
by rep after a warm-up; one JSON line with the medians, minima and maxima, the distribution of music_sweeps and of
music_sources, and the scan's rate against its arithmetic lower bound, 4 G N (N - M) multiply-adds per unit (the Jacobi
sweeps are not counted: the rate is a lower bound of the scan's own)."""
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
    edges = [(c['freqlist'][b], c['freqlist'][b + 1]) for b in range(c['NBANDS'])]
    grid = planner.slowness_grid(4.0, 41)
    xij = planner.co_array(c['rij'])[0]
    W = engine.plan_windows(len(data[0]), fs, c['WINLEN_list'], c['overlap'])[0]
    freqs = planner.capon_frequencies(edges)
    Ls, Hs = planner.capon_snapshots(xij, grid, fs, freqs, W)
    h = engine.get_handle()
    capon = dict(capon_grid=grid, capon_freqs=freqs, capon_snapshots=(Ls, Hs))
    peaks = dict(capon_peaks=4, capon_peak_floor=0.25)
    N = len(data)
    forms = dict(spectra=capon,
                 music_2=dict(capon, capon_music=(2, 0.05, False, False)),
                 music_rule=dict(capon, capon_music=(0, 0.05, False, False)),
                 spectra_peaks=dict(capon, **peaks),
                 music_2_peaks=dict(capon, capon_music=(2, 0.05, False, False, True, 0.0), **peaks),
                 clean_16=dict(capon, capon_clean=(16, 0.5, 0.02, False)))
    base = dict(music_2_peaks='spectra_peaks')

    def run(form):
        res = engine.process(data, fs, t0, c['rij'], edges, c['WINLEN_list'], c['overlap'], c['alpha'], c['ftype'], c['order'],
                             c['ripple'], **forms[form])
        return res, h.timings()

    out = {k: [] for k in forms}
    stats = {}
    with contextlib.redirect_stdout(io.StringIO()):
        for form in forms:
            run(form)
        h.set_profiling(True)
        for _ in range(reps):
            for form in forms:
                res, t = run(form)
                out[form].append((t['solve_ms'], t['total_ms']))
                if res.music_sweeps is not None and form not in stats:
                    cat = lambda a: np.concatenate([a[b, :int(n)] for b, n in enumerate(res.nwin)])
                    stats[form] = (cat(res.music_sweeps), cat(res.music_sources))
        h.set_profiling(False)
    G = len(grid)
    rec = dict(shape='cfg3', reps=reps, units=int(res.nwin.sum()), elements=N, grid_points=G)
    for key in forms:
        a = np.array(out[key])
        rec[key] = dict(solve_ms=[float(np.median(a[:, 0])), float(a[:, 0].min()), float(a[:, 0].max())],
                        total_ms=[float(np.median(a[:, 1])), float(a[:, 1].min()), float(a[:, 1].max())])
    for key in ('music_2', 'music_rule', 'music_2_peaks', 'clean_16'):
        rec[key]['kernel_ms'] = rec[key]['solve_ms'][0] - rec[base.get(key, 'spectra')]['solve_ms'][0]
    for key, (sweeps, sources) in stats.items():
        computed = sources > 0
        fma = float(np.sum(4.0 * G * N * (N - sources[computed])))
        rec[key].update(sweeps_mean=float(sweeps[computed].mean()), sweeps_histogram=np.bincount(sweeps[computed]).tolist(),
                        sources_histogram=np.bincount(sources[computed], minlength=N).tolist(), degenerate_units=int((~computed).sum()),
                        scan_fp64_fma=fma, scan_fp64_tflops=2.0 * fma / (rec[key]['kernel_ms'] * 1e-3) / 1e12)
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
