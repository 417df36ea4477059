"""The cost of the element delays (nbls_set_element_delays; csrc/element_delay.hip) in a device pass: the cfg-3 pass (8
elements, 48 bands, W = 1200, half overlap, 69 024 units, LTS 0.5, element 7 0.25 s late) without the feature and with it —
plain and against the beam of the kept elements, in the automatic (staged) and the forced global form where both apply —
with planner.element_shifts of the bands' upper edges, from the handle's events (set_profiling).

    python tools/element_delay_time.py [reps]

The forms alternate rep by rep after a warm-up; one JSON line with the medians, minima and maxima, the multiply-adds the
kernel does for C and E_m (2 N (2K + 1) W per unit) and the bytes its staged form reads from LDS (three doubles per
multiply-add pair with one shift per item, (2 + 4) / 4 with four: the reads of the (m, k) items alone, without the N E_b
items, the two re-summed neighbours per element and the staging, so a lower figure).  Option "element_delay_chunk" = 1
runs the one-shift-per-item instances beside the default ones."""
import contextlib
import io
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from narrow_band_least_squares_amd import engine, planner, synthetic, _hip  # noqa: E402


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    c = synthetic.build_config('cfg3', 1.0)
    data, fs, t0 = engine.stream_rows(c['st'])
    N, npts = len(data), len(data[0])
    edges = [(c['freqlist'][b], c['freqlist'][b + 1]) for b in range(c['NBANDS'])]
    shifts = planner.element_shifts([e[1] for e in edges], fs)
    h = engine.get_handle()
    kept = (N - 1, False, False)
    on, on_kept = dict(element_max_shift=shifts), dict(kept=kept, element_max_shift=shifts, element_delays_kept=True)
    # (form, shifts per item): options "element_delay_form" and "element_delay_chunk"
    forms = dict(off=(0, 0, dict()), kept_only=(0, 0, dict(kept=kept)),
                 plain_auto=(0, 0, on), plain_auto_chunk1=(0, 1, on), plain_global=(2, 0, on), plain_global_chunk1=(2, 1, on),
                 kept_auto=(0, 0, on_kept), kept_auto_chunk1=(0, 1, on_kept), kept_global=(2, 0, on_kept))

    def run(form):
        opt, chunk, kw = forms[form]
        h.set_option('element_delay_form', opt)
        h.set_option('element_delay_chunk', chunk)
        try:
            res = engine.process(data, fs, t0, c['rij'], edges, c['WINLEN_list'], c['overlap'], c['alpha'], c['ftype'], c['order'],
                                 c['ripple'], **kw)
        finally:
            h.set_option('element_delay_form', 0)
            h.set_option('element_delay_chunk', 0)
        return res, h.timings()

    out = {k: [] for k in forms}
    with contextlib.redirect_stdout(io.StringIO()):
        for form in forms:
            run(form)
        h.set_profiling(True)
        for _ in range(reps):
            for form in forms:
                res, t = run(form)
                out[form].append((t['solve_ms'], t['total_ms']))
        h.set_profiling(False)
    W = int(res.W[0])
    units = int(res.nwin.sum())
    pairs = int(sum(2 * N * (2 * int(k) + 1) * int(w) * int(n) for k, w, n in zip(shifts, res.W, res.nwin)))
    lib = _hip.load_library()
    rec = dict(shape='cfg3', reps=reps, units=units, elements=N, bands=len(edges), npts=npts, W=W, inc=int(res.inc[0]),
               max_shift=[int(k) for k in shifts], multiply_adds=pairs, lds_read_bytes_chunk1=pairs // 2 * 24,
               lds_read_bytes_chunk4=int(sum(8 * N * int(w) * int(n) * (2 * -(-(2 * int(k) + 1) // 4) + 2 * int(k) + 1)
                                             for k, w, n in zip(shifts, res.W, res.nwin))),
               staged_lds_bytes=[int(lib.nbls_element_delay_lds_bytes(N, int(w), int(k))) for k, w in zip(shifts, res.W)],
               nonzero_shift_fraction=float(np.mean(res.element_shift != 0)))
    for key in forms:
        a = np.array(out[key])
        rec[key] = dict(solve_ms=[float(np.median(a[:, 0])), float(a[:, 0].min()), float(a[:, 0].max())],
                        total_ms=[float(np.median(a[:, 1])), float(a[:, 1].min()), float(a[:, 1].max())])
    for key, base in (('plain_auto', 'off'), ('plain_auto_chunk1', 'off'), ('plain_global', 'off'), ('plain_global_chunk1', 'off'),
                      ('kept_auto', 'kept_only'), ('kept_auto_chunk1', 'kept_only'), ('kept_global', 'kept_only')):
        rec[key + '_extra_solve_ms'] = rec[key]['solve_ms'][0] - rec[base]['solve_ms'][0]
        rec[key + '_extra_total_ms'] = rec[key]['total_ms'][0] - rec[base]['total_ms'][0]
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
