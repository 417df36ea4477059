"""The cost of the beam trace (nbls_set_beam_trace, csrc/beam_trace.hip: beam_trace_kernel) in a device pass: the cfg-3 pass
(8 elements, 48 bands, W = 1200, half overlap, 69 024 units, LTS 0.5) without the trace, with it ungated, and with it gated
at the demonstration's threshold (MdCCM >= 0.295, tests/beam_trace_cases.py), Hann synthesis window, from the handle's events
(set_profiling).

    python tools/beam_trace_time.py [reps]

The kernel is one launch behind the pass's last solve, ahead of the closing event: what it costs is the difference of the
passes' total intervals with and without it (the solve interval grows by the same amount where the pass solves in one
piece).  The three forms alternate rep by rep after a warm-up; one JSON line with the medians, minima and maxima, the share
of windows the gate lets through, the bytes the kernel asks for (C N 8 per sample read, 8 written, C = ceil(W / inc) windows
over a sample) and the effective load bandwidth that difference amounts to."""
import contextlib
import io
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from narrow_band_least_squares_amd import engine, synthetic  # noqa: E402

GATE = 0.295


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    c = synthetic.build_config('cfg3', 1.0)
    data, fs, t0 = engine.stream_rows(c['st'])
    N, npts = len(data), len(data[0])
    edges = [(c['freqlist'][b], c['freqlist'][b + 1]) for b in range(c['NBANDS'])]
    h = engine.get_handle()
    forms = dict(plain={}, trace=dict(want_beam_trace='hann'), trace_gated=dict(want_beam_trace=dict(window='hann', mdccm_min=GATE)))

    def run(form):
        res = engine.process(data, fs, t0, c['rij'], edges, c['WINLEN_list'], c['overlap'], c['alpha'], c['ftype'], c['order'],
                             c['ripple'], **forms[form])
        return res, h.timings()

    out = {k: [] for k in forms}
    with contextlib.redirect_stdout(io.StringIO()):
        for form in list(forms) * 2:
            run(form)
        h.set_profiling(True)
        for _ in range(reps):
            for form in forms:
                res, t = run(form)
                out[form].append((t['solve_ms'], t['total_ms']))
        h.set_profiling(False)
    W, inc = int(res.W[0]), int(res.inc[0])
    C = -(-W // inc)
    computed = np.arange(res.mdccm.shape[1])[None, :] < np.asarray(res.nwin)[:, None]
    rec = dict(shape='cfg3', reps=reps, units=int(res.nwin.sum()), elements=N, bands=len(edges), npts=npts, W=W, inc=inc,
               windows_over_a_sample=C, gate=GATE, windows_through_the_gate=float(np.mean(res.mdccm[computed] >= GATE)),
               filtered_gb=len(edges) * N * npts * 8 / 1e9, trace_gb=len(edges) * npts * 8 / 1e9,
               asked_load_gb=len(edges) * npts * C * N * 8 / 1e9)
    for key in forms:
        a = np.array(out[key])
        rec[key] = dict(solve_ms=[float(np.median(a[:, 0])), float(a[:, 0].min()), float(a[:, 0].max())],
                        total_ms=[float(np.median(a[:, 1])), float(a[:, 1].min()), float(a[:, 1].max())])
    for key in ('trace', 'trace_gated'):
        extra = rec[key]['total_ms'][0] - rec['plain']['total_ms'][0]
        rec[key + '_extra_ms'] = extra
        rec[key + '_extra_solve_ms'] = rec[key]['solve_ms'][0] - rec['plain']['solve_ms'][0]
    rec['trace_effective_load_gb_per_s'] = rec['asked_load_gb'] / (rec['trace_extra_ms'] * 1e-3) if rec['trace_extra_ms'] > 0 else None
    print(json.dumps(rec), flush=True)


if __name__ == '__main__':
    main()
