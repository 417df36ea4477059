"""The premises of tests/test_gpu_scale.py, on the CPU: the table of tests/scale_cases.py names every
field a ``BandBatch`` can carry and every key of the public calls' result dictionaries; every input set meets the condition
under which a power-of-two scale is exact (nothing subnormal, nothing out of range, at every k the GPU test uses); and the
float64 and long-double restatements of the suite — the oracle's correlation and solves, the filter truths, the beam, Capon,
MUSIC and CLEAN-SC truths — obey the table on these inputs bit for bit.  The last is the proof that the relation holds for
the reference alone: what the GPU test then finds is the library's."""
import numpy as np
import pytest

import band_batch_cases as bb
import beam_truth
import capon_truth as ct
import clean_truth
import filter_truth as ft
import music_truth
import scale_cases as sc
from scale_cases import SAME, NEGATED, UNDEFINED, T1, T2, T3, times
from narrow_band_least_squares_amd import engine, planner


# ---- 1. the table ----------------------------------------------------------------------------------------------------
def test_the_table_names_every_field_and_every_key():
    names, _ = sc.batch_fields()
    missing = [f for f in names + sc.result_keys() if f not in sc.TABLE]
    assert not missing, 'no behaviour declared for %s (tests/scale_cases.py, DESIGN.md section 27)' % missing
    for group in (engine.CLEAN_FIELDS, engine.MUSIC_FIELDS):
        assert all(f in sc.TABLE for f in group)
    for which in ('capon', 'bartlett', 'music'):
        assert all(which + f in sc.TABLE for f in engine.PEAK_FIELDS)
    for f in bb.FIELDS + bb.PLAIN_FIELDS:
        assert f in sc.TABLE, f
    allowed = {SAME, NEGATED, UNDEFINED, times(1), times(2)}
    for f, row in sc.TABLE.items():
        assert len(row) == 3 and set(row) <= allowed, (f, row)


def test_a_field_without_an_entry_is_an_error():
    """What a future field meets: ``compare`` refuses a ``BandBatch`` (or a dictionary) that carries a name the table lacks."""
    _, res = sc.batch_fields()
    sc.compare(res, res, T1, 0)
    res.coherence_of_tomorrow = np.zeros(3)
    with pytest.raises(KeyError, match='coherence_of_tomorrow'):
        sc.compare(res, res, T1, 0)
    with pytest.raises(KeyError):
        sc.compare(dict(vel=np.zeros(2), new_key=np.zeros(2)), dict(vel=np.zeros(2), new_key=np.zeros(2)), T3)


def test_the_entries_the_definitions_imply():
    same_all = ('lag', 'lag_frac', 'cmax', 'mask', 'z', 'vel', 'baz', 'mdccm', 'sigma_tau', 'vel_uncert', 'baz_uncert', 'consistency',
                'closure_max', 'element_consistency', 'family', 'family_table', 't', 'nwin', 'dropped_mask', 'kept_count')
    for f in same_all:
        assert sc.TABLE[f] == (SAME, SAME, SAME), f
    same_t1 = ('fstat', 'grid_index', 'grid_fstat', 'grid_map', 'element_delay', 'element_cc', 'element_shift', 'music_sources',
               'music_sweeps', 'music_vectors', 'music_map', 'music_power', 'music_peak_power', 'clean_count', 'clean_index',
               'capon_index', 'bartlett_index') + tuple(w + f for w in ('capon', 'bartlett', 'music')
                                                        for f in ('_peak_count', '_peak_index', '_peak_offset'))
    for f in same_t1:
        assert sc.TABLE[f] == (SAME, UNDEFINED, SAME), f
    power = ('beam_power', 'grid_power', 'capon_power', 'capon_map', 'bartlett_power', 'bartlett_map', 'capon_csdm', 'clean_csdm',
             'clean_power', 'clean_total', 'clean_residual', 'capon_peak_power', 'bartlett_peak_power', 'music_eigenvalues')
    for f in power:
        assert sc.TABLE[f] == (times(2), UNDEFINED, SAME), f
    assert sc.TABLE['beam_trace'] == (times(1), UNDEFINED, NEGATED)
    assert sc.TABLE['filtered'] == (times(1), times(1), NEGATED)
    # a lag seed is the maximum of a beam: under per-channel gains the lags of a seeded plan are no longer defined by the pair alone
    assert sc.behaviour('lag', T2, seeded=True) == UNDEFINED and sc.behaviour('lag', T1, seeded=True) == SAME
    assert sc.behaviour('lag_frac', T2) == SAME


def test_the_comparison_sees_one_bit():
    x = np.linspace(0.1, 1.0, 7)
    assert sc.check_field('beam_power', x, np.ldexp(x, 48), T1, 24) == 7
    with pytest.raises(AssertionError, match='beam_power'):
        sc.check_field('beam_power', x, np.ldexp(x, 48) * (1.0 + 2.0 ** -52), T1, 24)
    with pytest.raises(AssertionError):
        sc.check_field('vel', x, np.nextafter(x, 2.0), T3)
    assert sc.check_field('beam_trace', np.array([0.0, 1.5]), np.array([0.0, -1.5]), T3) == 2        # an untouched +0.0 stays
    with pytest.raises(AssertionError):
        sc.check_field('beam_trace', np.array([0.0, 1.5]), np.array([0.0, 1.5]), T3)
    assert sc.check_field('grid_power', x, x, T2) == 0                                                  # undefined: not compared
    z = x + 1j * x[::-1]
    assert sc.check_field('capon_csdm', z, z * 2.0 ** -60, T1, -30) == 7
    f = np.arange(12.0).reshape(6, 2) + 1.0
    assert sc.check_field('filtered', f, f * (2.0 ** sc.gains(6))[:, None], T2) == 12


# ---- 2. the condition on the inputs ----------------------------------------------------------------------------------
GPU_CASES = {'screen': sc.cases(), 'long': sc.cases(ks=(-30, 100), t2=False), 'groups': sc.cases(ks=(-30, 100), t2=False),
             'general': sc.cases(), 'plans': sc.cases()}


@pytest.mark.parametrize('name', sorted(GPU_CASES))
def test_prefiltered_sets_stay_in_range_at_every_scale(name):
    c = sc.prefiltered(name)
    W, inc = planner.window_plan(c['data'].shape[1], c['fs'], c['winlen'], 0.5)[:2]
    assert int(W) == c['W']
    for label, T, k in GPU_CASES[name]:
        lo, hi = sc.check_condition(sc.transform(c['data'], T, k), int(W), int(inc), '%s %s' % (name, label))
        if T == T1 and abs(k) == 100:
            assert max(abs(lo), abs(hi)) > 2 * 126          # ... and far outside what a float holds: the point of k = +-100


def test_other_sets_stay_in_range():
    for N in (8, 32):
        c = sc.extras(N)
        W, inc = planner.window_plan(c['data'].shape[1], c['fs'], c['winlen'], 0.5)[:2]
        for label, T, k in sc.cases(ks=(-30, 24, 100)):
            sc.check_condition(sc.transform(c['data'], T, k), int(W), int(inc), 'extras %d %s' % (N, label))
    data, half = sc.gain_step()
    c = sc.prefiltered('screen')
    sc.check_condition(data, c['W'], c['W'] // 2, 'gain step')
    before, after, across = sc.window_sides(data.shape[1], c['fs'], c['winlen'], 0.5, half)
    assert len(before) >= 2 and len(after) >= 2 and len(across) >= 1 and len(before) + len(after) + len(across) == 9
    # a window quantised with the scale of the window before it is visible behind the step: the window before the first one
    # wholly behind it straddles the step, and on some channel its largest unscaled sample lies before the step, so that its
    # max |x| in the stepped trace is not 2^40 times the unscaled one
    W, inc = c['W'], c['W'] // 2
    prev = int(after[0]) - 1
    assert prev in across
    seg = np.abs(c['data'][:, prev * inc:prev * inc + W])
    assert np.any(seg[:, :half - prev * inc].max(axis=1) > seg[:, half - prev * inc:].max(axis=1))
    recs = bb.recordings()[0]
    for s, k in enumerate((-30, 0, 24)):
        sc.check_condition(sc.transform(recs[s], T1, k), 65, 32, 'batch recording %d' % s)
    counts = sc.counts_int32()
    assert counts.dtype == np.int32 and np.abs(counts).max() == 2 ** 23 and len(np.unique(counts)) > 1000
    x32 = c['data'].astype(np.float32)
    assert np.all(np.abs(x32[x32 != 0]) >= np.finfo(np.float32).tiny)


# ---- 3. the references obey the table --------------------------------------------------------------------------------
def _oracle_rows(oracle, c, data, alpha, first_only=False):
    """The oracle's float64 restatement on a prefiltered trace -> dict in the names of the table."""
    W, inc, intervals = oracle.window_plan(data.shape[1], c['fs'], c['winlen'], 0.5)
    xij, idx = oracle.co_array(c['rij'])
    if first_only:
        tau, mdccm, cmax = oracle.correlate_windows(np.ascontiguousarray(data.T), W, intervals[:1], idx, c['fs'])
        return dict(lag=np.rint(tau * c['fs']).astype(np.int32), cmax=cmax, mdccm=mdccm)
    st = oracle.make_stream(np.array(data), c['fs'], starttime=sc.T0)
    out, internals = oracle.ltsva(st, None, None, c['winlen'], 0.5, alpha, rij=c['rij'], return_internals=True, ci_samples=0)
    return dict(lag=np.rint(internals['tau'] * c['fs']).astype(np.int32), cmax=internals['cmax'], z=internals['z'],
                mask=internals['weights'], vel=out[0], baz=out[1], t=out[2], mdccm=out[3], sigma_tau=out[5], vel_uncert=out[6],
                baz_uncert=out[7])


@pytest.mark.parametrize('name,alpha', [('screen', 1.0), ('screen', 0.5), ('general', 1.0), ('plans', 0.5), ('long', 1.0),
                                        ('groups', 1.0)])
def test_the_oracle_obeys_the_table(oracle, name, alpha):
    """Lags, maxima, MdCCM, the OLS and the LTS solve and the confidence intervals of the oracle: the same bits under every
    transformation the GPU test applies to the set (the long windows: their first window, np.correlate is quadratic)."""
    c = sc.prefiltered(name)
    first = name in ('long', 'groups')
    ref = _oracle_rows(oracle, c, c['data'], alpha, first)
    assert np.isfinite(ref['cmax']).all() and np.ptp(ref['lag']) > 0
    for label, T, k in GPU_CASES[name]:
        got = _oracle_rows(oracle, c, sc.transform(c['data'], T, k), alpha, first)
        nf, nc = sc.compare(ref, got, T, k, label='oracle %s %s:' % (name, label))
        assert nf == len(ref)


def test_the_oracle_obeys_the_table_across_a_gain_step(oracle):
    c = sc.prefiltered('screen')
    data, half = sc.gain_step()
    before, after, across = sc.window_sides(data.shape[1], c['fs'], c['winlen'], 0.5, half)
    ref, got = _oracle_rows(oracle, c, c['data'], 1.0), _oracle_rows(oracle, c, data, 1.0)
    for idx in (before, after):
        assert sc.same_bits(ref['lag'][:, idx], got['lag'][:, idx]) and sc.same_bits(ref['cmax'][:, idx], got['cmax'][:, idx])
        assert sc.same_bits(ref['vel'][idx], got['vel'][idx])


def _raw_filters():
    c = sc.raw()
    return c, [planner.design_bandpass_many(sc.RAW_FILTER[0], sc.RAW_EDGES, sc.RAW_FILTER[1], sc.RAW_FILTER[2], c['fs'])[b][:2]
               for b in range(len(sc.RAW_EDGES))]


def test_the_filter_truths_obey_the_table():
    """SciPy's float64 cascade, the chunked scan in float64 and the long-double truth on the raw trace, both bands, zero-phase
    with the taper: times 2^k (per channel under T2), negated under T3; no filtered sample and no window energy is
    subnormal at the smallest scale."""
    c, filters = _raw_filters()
    assert sc.RAW_EDGES[0] == ft.NARROW_BANDS[5][1:3] and ft.NARROW_BANDS[5][4] == c['fs']
    widths = [(hi - lo) / lo for _, lo, hi, _, fs in ft.NARROW_BANDS]
    assert min(widths) == widths[5]                                   # the narrowest band of the filter tests
    for b, (sos, zero_phase) in enumerate(filters):
        assert zero_phase
        W = int(sc.RAW_WINLENS[b] * c['fs'])
        ref = {name: fn(sos, c['data'], True) for name, fn in (('scipy', ft.scipy_float64), ('chunked', ft.chunked_float64))}
        ref['truth'] = ft.df2t_truth(sos, c['data'], True)
        for label, T, k in sc.cases():
            x = sc.transform(c['data'], T, k)
            for name, fn in (('scipy', ft.scipy_float64), ('chunked', ft.chunked_float64)):
                y = fn(sos, x, True)
                assert sc.check_field('filtered', ref[name], y, T, k, label='%s band %d %s:' % (name, b, label)) == x.size
                sc.check_condition(y, W, W // 2, 'filtered band %d %s' % (b, label))
            if T != T2:
                y = ft.df2t_truth(sos, x, True)
                exp = -ref['truth'] if T == T3 else np.ldexp(ref['truth'], k)
                assert np.array_equal(exp, y), (b, label)


def _extras_truths(oracle, c, data, loading=0.01):
    N, W, fs = c['N'], c['W'], c['fs']
    Ws, Ls, Hs = sc.EXTRAS_SHAPE
    _, inc, intervals = oracle.window_plan(data.shape[1], fs, c['winlen'], 0.5)
    nwin = len(intervals)
    xij, idx = oracle.co_array(c['rij'])
    tau = oracle.correlate_windows(np.ascontiguousarray(data.T), W, intervals, idx, fs)[0]
    z = oracle.ols_solve(xij, tau)[0].T
    beam = beam_truth.beam_reference(data, fs, xij, z, W, inc, nwin)
    coef, steer = ct.tables(xij, c['grid'], fs, c['freq'], Ls, N)
    R = ct.csdm_reference(data, coef, W, inc, nwin, Hs)[0]
    out = dict(z=z, beam_power=beam['beam_power'], fstat=beam['fstat'], capon_csdm=R.astype(np.complex128))
    rows = {k: [] for k in ('bartlett_map', 'capon_map', 'bartlett_index', 'capon_index', 'music_eigenvalues', 'music_vectors',
                            'music_sweeps', 'music_map', 'music_index', 'clean_count', 'clean_index', 'clean_power', 'clean_total',
                            'clean_residual', 'clean_csdm')}
    for w in range(nwin):
        R64 = out['capon_csdm'][w]
        sp = ct.spectra_reference(R64, steer, loading)
        mu = music_truth.music(R64, steer, 2)
        cl = clean_truth.clean_reference(R64, steer, 6, 0.5, 0.02)
        for k, v in (('bartlett_map', sp['PB'].astype(np.float64)), ('capon_map', sp['PC'].astype(np.float64)),
                     ('bartlett_index', sp['index_B']), ('capon_index', sp['index_C']),
                     ('music_eigenvalues', mu['lam'].astype(np.float64)), ('music_vectors', mu['E'].astype(np.complex128)),
                     ('music_sweeps', mu['sweeps']), ('music_map', mu['D'].astype(np.float64)), ('music_index', mu['index']),
                     ('clean_count', cl['count']), ('clean_index', cl['index']), ('clean_power', cl['power']),
                     ('clean_total', cl['total']), ('clean_residual', cl['residual']), ('clean_csdm', cl['R'])):
            rows[k].append(v)
    out.update({k: np.array(v) for k, v in rows.items()})
    return out


def test_the_truths_of_the_opt_in_results_obey_the_table(oracle):
    """The beam, Capon / Bartlett, MUSIC and CLEAN-SC references on the 8-element set: powers, matrices and eigenvalues carry
    2^(2k), ratios, vectors, indices and counts nothing, at k = -30, +24, +100 and under negation."""
    c = sc.extras(8)
    ref = _extras_truths(oracle, c, c['data'])
    assert np.all(ref['clean_count'] > 0) and np.all(ref['music_eigenvalues'][:, 0] > 0) and np.isfinite(ref['fstat']).all()
    for label, T, k in sc.cases(ks=(-30, 24, 100), t2=False):
        got = _extras_truths(oracle, c, sc.transform(c['data'], T, k))
        nf, nc = sc.compare(ref, got, T, k, label='truths %s:' % label)
        assert nf == len(ref)
