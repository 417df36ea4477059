"""The cost of the slowness-grid search (nbls_set_beam_grid, csrc/beam_grid.hip) in a device pass: the cfg-3 pass (8
elements, 48 bands, W = 1200, 69 024 units, LTS 0.5) with and without the 41 x 41 grid over +-4 s/km (1257 points), from
the handle's events (set_profiling).

    python tools/beam_grid_time.py [reps] [--shape cfg3] [--points 41]

beam_grid_kernel runs behind every unit range's solve, inside the solve interval of nbls_timings: its time is the
difference of the two solve intervals.  The two forms alternate rep by rep after a warm-up; one JSON line with the
medians, minima and maxima, the work (G N W samples per unit) and the fraction of the two bounds the kernel reaches: one
8-byte LDS read per sample at 256 B/clk/CU, and the FP64 vector operations per sample (three as the loop stands, b += v,
v * v, q += ...; two is the least a form with both sums can do) at 64 lane-operations/clk/CU, 256 CUs at 2.4 GHz."""
import contextlib
import io
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from narrow_band_least_squares_amd import engine, planner, synthetic, _hip  # noqa: E402

CUS, CLK = 256, 2.4e9


def main():
    argv = sys.argv[1:]
    name, points = 'cfg3', 41
    for flag in ('--shape', '--points'):
        if flag in argv:
            i = argv.index(flag)
            if flag == '--shape':
                name = argv[i + 1]
            else:
                points = int(argv[i + 1])
            del argv[i:i + 2]
    reps = int(argv[0]) if argv else 9
    c = synthetic.build_config(name, 1.0)
    data, fs, t0 = engine.stream_rows(c['st'])
    edges = [(c['freqlist'][b], c['freqlist'][b + 1]) for b in range(c['NBANDS'])]
    grid = planner.slowness_grid(4.0, points)
    h = engine.get_handle()

    def run(search):
        res = engine.process(data, fs, t0, c['rij'], edges, c['WINLEN_list'], c['overlap'], c['alpha'], c['ftype'], c['order'],
                             c['ripple'], slowness_grid=grid if search else None)
        return res, h.timings()

    out = {False: [], True: []}
    with contextlib.redirect_stdout(io.StringIO()):
        for search in (False, True, False, True):
            run(search)
        h.set_profiling(True)
        for _ in range(reps):
            for search in (False, True):
                res, t = run(search)
                out[search].append((t['solve_ms'], t['total_ms']))
        h.set_profiling(False)
    units, N, W, G = int(res.nwin.sum()), res.nchans, int(res.W[0]), len(grid)
    xij = planner.co_array(c['rij'])[0]
    tau = fs * (xij[None, :N - 1, 0] * grid[:, None, 0] + xij[None, :N - 1, 1] * grid[:, None, 1])
    halo = int(np.abs(np.rint(tau)).max())
    samples = float(units) * G * N * W
    rec = dict(shape=name, reps=reps, units=units, elements=N, W=W, grid_points=G, halo=halo,
               lds_bytes=int(_hip.load_library().nbls_beam_grid_lds_bytes(N, W, halo)), samples=samples,
               bytes_staged_per_unit=8 * N * (W + 2 * halo), bytes_written_per_unit=20,
               index_found=float(np.mean(res.grid_index[res.grid_fstat != 0] >= 0)),
               fstat_median=float(np.nanmedian(res.grid_fstat[res.grid_fstat != 0])))
    for search, key in ((False, 'plain'), (True, 'grid')):
        a = np.array(out[search])
        rec[key] = dict(solve_ms=[float(np.median(a[:, 0])), float(a[:, 0].min()), float(a[:, 0].max())],
                        total_ms=[float(np.median(a[:, 1])), float(a[:, 1].min()), float(a[:, 1].max())])
    k = rec['grid']['solve_ms'][0] - rec['plain']['solve_ms'][0]
    rec['kernel_ms'] = k
    rec['lds_bound_ms'] = samples * 8 / (256.0 * CUS * CLK) * 1e3
    rec['fp64_bound_ms_2ops'] = samples * 2 / (64.0 * CUS * CLK) * 1e3
    rec['fp64_bound_ms_3ops'] = samples * 3 / (64.0 * CUS * CLK) * 1e3
    rec['fraction_of_lds_bound'] = rec['lds_bound_ms'] / k
    rec['fraction_of_fp64_bound_3ops'] = rec['fp64_bound_ms_3ops'] / k
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
