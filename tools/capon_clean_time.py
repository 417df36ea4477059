"""The cost of the CLEAN-SC components (nbls_set_capon_clean, csrc/capon_clean.hip) in a device pass: the cfg-3 pass (8 elements,
48 bands, W = 1200, 69 024 units, LTS 0.5) with the Capon spectra alone over planner.slowness_grid(4.0, 41) — the 1257 points
of a 41 x 41 lattice over +-4 s/km that lie within 4 s/km of the origin —, with CLEAN-SC of I = 4, 16 and 32 iterations at
floor 0.02, with I = 16 at floor 0 (no unit stops early), and with I = 16 on the elements LTS kept, from the handle's events
(set_profiling).

    python tools/capon_clean_time.py [reps]

capon_clean_kernel runs behind capon_kernel inside the solve interval of nbls_timings: its time is the difference of the
form's solve interval and that of the spectra alone (the KEPT form: of the spectra on the kept elements).  The forms
alternate rep by rep after a warm-up; one JSON line with the medians, minima and maxima, the distribution of count, and the
kernel's rate against the arithmetic lower bound of the scan, 4 G N (N - 1) / 2 + 3 G N multiply-adds per iteration taken
(capon_bartlett_point reads the lower triangle; the definition's G N^2 complex products are twice that)."""
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
    N = len(data)
    kept = dict(kept=(N - 1, False, True))
    forms = dict(spectra=capon,
                 clean_4=dict(capon, capon_clean=(4, 0.5, 0.02, False)),
                 clean_16=dict(capon, capon_clean=(16, 0.5, 0.02, False)),
                 clean_32=dict(capon, capon_clean=(32, 0.5, 0.02, False)),
                 clean_16_no_floor=dict(capon, capon_clean=(16, 0.5, 0.0, False)),
                 spectra_kept=dict(capon, **kept),
                 clean_16_kept=dict(capon, capon_clean=(16, 0.5, 0.02, False), **kept))
    base = dict(clean_16_kept='spectra_kept')

    def run(form):
        res = engine.process(data, fs, t0, c['rij'], edges, c['WINLEN_list'], c['overlap'], c['alpha'], c['ftype'], c['order'],
                             c['ripple'], **forms[form])
        return res, h.timings()

    out = {k: [] for k in forms}
    counts = {}
    with contextlib.redirect_stdout(io.StringIO()):
        for form in forms:
            run(form)
        h.set_profiling(True)
        for _ in range(reps):
            for form in forms:
                res, t = run(form)
                out[form].append((t['solve_ms'], t['total_ms']))
                if res.clean_count is not None and form not in counts:
                    done = np.concatenate([res.clean_count[b, :int(n)] for b, n in enumerate(res.nwin)])
                    counts[form] = done
        h.set_profiling(False)
    G = len(grid)
    rec = dict(shape='cfg3', reps=reps, units=int(res.nwin.sum()), elements=N, grid_points=G)
    for key in forms:
        a = np.array(out[key])
        rec[key] = dict(solve_ms=[float(np.median(a[:, 0])), float(a[:, 0].min()), float(a[:, 0].max())],
                        total_ms=[float(np.median(a[:, 1])), float(a[:, 1].min()), float(a[:, 1].max())])
    per_scan = 4.0 * G * N * (N - 1) / 2 + 3.0 * G * N
    for key, done in counts.items():
        ms = rec[key]['solve_ms'][0] - rec[base.get(key, 'spectra')]['solve_ms'][0]
        scans = float(np.sum(np.minimum(done + 1, int(forms[key]['capon_clean'][0]))))    # a unit that stops has scanned once more
        rec[key].update(kernel_ms=ms, count_mean=float(done.mean()), count_quartiles=[float(q) for q in np.percentile(done, [0, 25, 50, 75, 100])],
                        count_histogram=np.bincount(done, minlength=int(forms[key]['capon_clean'][0]) + 1).tolist(),
                        scans=scans, scan_fp64_fma=scans * per_scan, scan_fp64_tflops=2.0 * scans * per_scan / (ms * 1e-3) / 1e12)
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
