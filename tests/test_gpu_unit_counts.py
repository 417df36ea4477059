"""Every kernel that shares units — (band or recording row, window) cells — among its waves, workgroups or XCD ranges, at
the unit counts where that share-out changes ("Unit share-outs"; tests/unit_count_cases.py).

Each case is one pre-filtered pass over a periodic trace at one unit count, with two kinds of assertion:

* the first m units (the *templates*; all of them where the pass has fewer) against the references the suite already
  has, at the tolerances their own tests use: lags exact and cmax at rtol 1e-12 / atol 1e-15 against the FFT + long-double
  reference of tests/test_gpu_routes.py; z, vel, baz, sigma_tau, MdCCM, weights and both confidence intervals against the
  oracle on the GPU's own lags (tests/test_gpu_solve.py: _check_against_oracle); beam, closure and kept elements against
  beam_truth, closure_truth and kept_truth; a sub-array estimator against the call on the sub-array;
* every other unit against its template: row w of every fetched array equals row w mod m bit for bit (NaNs as
  patterns), and the cells behind the last window are zero.

A mismatch names the kernel family, the count, the unit, its template and the unit whose row it holds instead."""
import types

import numpy as np
import pytest
import torch

import beam_truth
import bounded_truth
import closure_truth as ct
import kept_truth as kt
import solve_truth as st
import steer_truth
import unit_count_cases as uc
from narrow_band_least_squares_amd import _hip, engine, planner
from test_gpu_bounded import _mixed_limits, _pass as _bounded_pass
from test_gpu_closure import REL as CLOSURE_REL
from test_gpu_seeded import GRID5, _check as _seeded_check, _geometry as _seeded_geometry, _pass as _seeded_pass
from test_gpu_solve import _check_against_oracle

pytestmark = pytest.mark.gpu

FS, T0 = uc.FS, uc.T0
PAD = 3                  # result cells behind the last window: they stay zero
POSITIONAL = ('beam_power', 'fstat')     # read samples outside the unit's window: compared with beam_truth at the trace ends


def _cus():
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


def _rows(res, band=0):
    """{name: (vector_len, ...) array} of every per-unit array of a ``BandBatch`` row."""
    VL = res.mask.shape[1]
    out = {}
    for k, v in vars(res).items():
        if isinstance(v, np.ndarray) and v.ndim >= 2 and k not in ('t', 'grids') and not k.startswith('_') and v.shape[1] == VL and v.shape[0] == res.mask.shape[0]:
            out[k] = v[band]
    return out


def _bytes(a, n):
    return np.ascontiguousarray(a[:n]).view(np.uint8).reshape(n, -1)


def _check_units(rows, nu, m, family, rot=0, templates=None, skip=(), interior=None):
    """Row w of every array equals the row of template (w + rot) mod m bit for bit — ``templates``: the arrays whose rows
    0..m-1 are the templates (default: these) —, and the rows behind unit nu are zero.  ``skip``: arrays left out;
    ``interior``: for the POSITIONAL arrays, the units (bool) whose reads stay inside the trace — those are compared with
    the first interior unit of their template, the others are the caller's."""
    key = (np.arange(nu) + rot) % m
    for name, a in rows.items():
        if name in skip:
            continue
        assert not _bytes(a[nu:], len(a) - nu).any(), '%s, %d units: %s is not zero behind the last unit' % (family, nu, name)
        got = _bytes(a, nu)
        src = got if templates is None else _bytes(templates[name], min(m, len(templates[name])))
        if name in POSITIONAL:
            if interior is None:
                continue
            units = np.flatnonzero(interior)
            first = {}
            for w in units:
                first.setdefault(int(key[w]), int(w))
            exp = got[np.array([first[int(key[w])] for w in units], dtype=int)]
        else:
            units = np.flatnonzero(key < len(src))
            exp = src[key[units]]
        bad = units[(got[units] != exp).any(axis=1)]
        if len(bad):
            w = int(bad[0])
            same = [int(v) for v in np.flatnonzero((got == got[w]).all(axis=1)) if v != w][:4]
            raise AssertionError('%s, %d units (m = %d): %s of unit %d is not the row of its template %d (%d units differ: %s); '
                                 'it equals the row of unit(s) %s' % (family, nu, m, name, w, int(key[w]), len(bad),
                                                                     bad[:8].tolist(), same or 'none'))


def _process(N, W, inc, nu, alpha, solve=False, **kw):
    """One pass at nu units -> (result, m, trace).  ``solve``: the templates also meet the conditions of the solve checks
    (``uc.solve_seed``)."""
    m = uc.choose_m(nu, N, _cus(), inc)
    x = uc.trace(N, W, inc, m, nu, seed=uc.solve_seed(N, W, inc, m, alpha) if solve else 0)
    kw = dict(dict(want_lag=True, want_cmax=True, want_z=True, want_uncert=True, vector_len=nu + PAD), **kw)
    res = engine.process(x, FS, T0, uc.geometry(N), [(None, None)], [uc.winlen(W)], uc.overlap(W, inc), alpha, prefiltered=True, **kw)
    assert int(res.nwin[0]) == nu and int(res.W[0]) == W and int(res.inc[0]) == inc
    return res, m, x


def _check_correlation(lag, cmax, N, W, inc, m, nu, family, rot=0, seed=0):
    """The template units against the FFT + long-double reference."""
    k = min(nu, m)
    lag_r, cmax_r = uc.template_reference(N, W, inc, m, seed)
    key = (np.arange(k) + rot) % m
    msg = '%s, %d units, N=%d W=%d inc=%d m=%d' % (family, nu, N, W, inc, m)
    np.testing.assert_array_equal(lag[:k], lag_r[key], err_msg=msg)
    np.testing.assert_allclose(cmax[:k], cmax_r[key], rtol=1e-12, atol=1e-15, err_msg=msg)


def _view(res, k):
    """The first k units of a result as ``_check_against_oracle`` reads them."""
    v = types.SimpleNamespace(**{name: a[None, :k] for name, a in _rows(res).items()})
    v.weights = None if res.weights is None else res.weights[:, :k]
    return v


def _check_solve(oracle, res, N, alpha, nu, m, family):
    """The template units' solve against the oracle on the GPU's own lags."""
    k = min(nu, m)
    xij, _, _ = planner.co_array(uc.geometry(N))
    tag = '%s, %d units, N=%d alpha=%g' % (family, nu, N, alpha)
    v = _view(res, k)
    names = ['template %d' % w for w in range(k)]
    if alpha < 1.0:
        r = st.oracle_lts(oracle, res.lag[0, :k], xij, alpha, FS)
        np.testing.assert_array_equal(v.weights[0], r['weights'].T, err_msg='SOLVE finding (%s): weights' % tag)
        z_o, sig_o = r['z'], r['sigma_tau']
    else:
        tau = np.ascontiguousarray(res.lag[0, :k].T / FS)
        z_o, _, _, sig_o = oracle.ols_solve(xij, tau)
        P = len(xij)
        assert np.all(np.unpackbits(res.mask[0, :k], axis=-1, bitorder='little')[:, :P] == 1), tag
    _check_against_oracle(oracle, v, k, xij, z_o, sig_o, names, tag)


def _correlation_case(N, W, inc, counts, family, alpha=1.0, oracle=None, expect=None, **kw):
    npts_pad = lambda nu: (uc.npts_of(W, inc, nu) + 63) // 64 * 64       # noqa: E731
    for nu in counts:
        if expect:
            r = _hip.route(N, W, npts_pad=npts_pad(nu))
            assert all(r[k] == v for k, v in expect.items()), (family, nu, r)
        res, m, _ = _process(N, W, inc, nu, alpha, solve=oracle is not None, **kw)
        _check_correlation(res.lag[0], res.cmax[0], N, W, inc, m, nu, family,
                           seed=uc.solve_seed(N, W, inc, m, alpha) if oracle is not None else 0)
        if oracle is not None:
            _check_solve(oracle, res, N, alpha, nu, m, family)
        _check_units(_rows(res), nu, m, family)


# ---- screening with the persistent DMA verifier ----------------------------------------------------------------------
def test_dma_verifier_at_every_walk_of_its_persistent_workgroups():
    """3 elements at the shortest window that screens, even hop: one to four units per persistent workgroup, ragged between
    the workgroups of an XCD and between XCDs, the last XCD's range short or empty; the screening grid's rows of 8 units
    and the quantiser's four-wave workgroups on the way."""
    s = uc.correlation_shapes()['dma_short']
    _correlation_case(s['N'], s['W'], uc.hop_for(s['W']), uc.unit_counts('verify_dma', _cus()), 'verify_dma_kernel', expect=s['expect'])


def test_dma_verifier_with_windows_on_odd_samples():
    """The same with an odd hop: every other window starts on an odd sample and is copied from one sample earlier; m is
    even, so a window and its template share the alignment class."""
    s = uc.correlation_shapes()['dma_short']
    c = uc.per_xcd(_cus())
    inc = uc.hop_for(s['W'], even=False)
    assert inc % 2 == 1 and uc.choose_m(9, 3, _cus(), inc) % 2 == 0
    _correlation_case(s['N'], s['W'], inc, (9, 8 * c + 1, 24 * c + 1), 'verify_dma_kernel, odd hop', expect=s['expect'])


def test_dma_verifier_at_8_elements():
    s = uc.correlation_shapes()['dma8']
    c = uc.per_xcd(_cus())
    _correlation_case(s['N'], s['W'], 100, (1, 9, 8 * c + 1), 'verify_dma_kernel, 8 elements', expect=s['expect'])


def test_dma_verifier_walks_across_the_rows_of_three_recordings():
    """Three recordings in one pass, each the base rotated by another number of hops: the smallest total of units at or
    above 8 c + 1 that three equal rows make, so that a row seam falls inside one workgroup's walk."""
    s = uc.correlation_shapes()['dma_short']
    N, W, S, rots = s['N'], s['W'], 3, (0, 2, 5)
    inc = uc.hop_for(W)
    nwin = uc.ceil_div(8 * uc.per_xcd(_cus()) + 1, S)
    m = uc.choose_m(S * nwin, N, _cus(), inc)
    recs = [uc.trace(N, W, inc, m, nwin, rot=a) for a in rots]
    npts = recs[0].shape[1]
    assert _hip.route(N, W, vrows=S, npts_pad=(npts + 63) // 64 * 64)['verifier'] == 1
    prep = engine.prepare(N, npts, FS, uc.geometry(N), [(None, None)], [uc.winlen(W)], uc.overlap(W, inc), 1.0, prefiltered=True,
                          vector_len=nwin + PAD)
    h = engine.get_handle()
    try:
        h.set_segments(S)
        h.set_trace_rows([row for r in recs for row in np.ascontiguousarray(r)], FS)
        h.set_geometry(prep.xij, prep.pair_idx, prep.xpinv)
        h.plan(None, prep.zero_phase, prep.tl, prep.tr, prep.W, prep.inc, prep.vector_len, lts=None)
        h.execute()
        got = h.fetch(want_lag=True, want_cmax=True, want_z=True)
    finally:
        h.set_segments(1)
    assert int(prep.nwin[0]) == nwin >= m
    names = ('lag', 'cmax', 'z', 'vel', 'baz', 'mdccm', 'sigma_tau')
    first = {k: got[k][0] for k in names}
    for s_, a in enumerate(rots):
        family = 'verify_dma_kernel, recording %d of 3' % s_
        _check_correlation(got['lag'][s_], got['cmax'][s_], N, W, inc, m, nwin, family, rot=a)
        _check_units({k: got[k][s_] for k in names}, nwin, m, family, rot=a, templates=first)


# ---- the quantiser instances -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('qi,qw', uc.QUANT_INSTANCES)
def test_quantiser_instances_at_the_item_totals_of_their_xcd_ranges(qi, qw):
    """One window length per reachable quantiser instance and wave count, 3 elements: item totals (units x channels) around
    8, around a full workgroup per XCD and with a share that is no multiple of the waves of a workgroup."""
    W = dict(((a, b), w) for a, b, w in uc.quantiser_shapes())[qi, qw]
    _correlation_case(3, W, uc.hop_for(W), uc.unit_counts('xcd_item', _cus(), N=3, waves=qw), 'quantize (inst %d, %d waves)' % (qi, qw),
                      expect=dict(quant_inst=qi, quant_waves=qw))


# ---- the other verifiers -----------------------------------------------------------------------------------------------
def test_lds_verifier_at_the_unit_totals_of_its_xcd_ranges():
    s = uc.correlation_shapes()['lds']
    _correlation_case(s['N'], s['W'], 50, uc.unit_counts('xcd_item', _cus()), 'verify_lds_kernel', expect=s['expect'])


def test_global_memory_verifier_at_its_items_of_four():
    s = uc.correlation_shapes()['glob']
    _correlation_case(s['N'], s['W'], uc.hop_for(s['W']), uc.unit_counts('verify_glob'), 'verify_kernel', expect=s['expect'])


# ---- the bounded and the seeded simple kernels ---------------------------------------------------------------------------
def test_bounded_simple_kernel_at_its_items_of_four():
    """17 elements x W = 48 (the general form of the bounded search), limits that mix 0, 1, W / 3, W - 1 and 10^6: every
    unit against the slice arg-max of tests/bounded_truth.py."""
    N, W, inc = 17, 48, 12
    pairs = bounded_truth.pair_table(N)
    lim = _mixed_limits(len(pairs), W, 0)
    assert _hip.lag_limit_form(N, W, int(lim.min())) == 2
    for nu in uc.unit_counts('range_pick'):
        x = uc.trace(N, W, inc, 7, nu)
        exp_lag, exp_cmax = bounded_truth.pick_windows(x, W, [w * inc for w in range(nu)], pairs, lim)
        lag, cmax = _bounded_pass(x, W, inc, lim)
        np.testing.assert_array_equal(lag, exp_lag, err_msg='xcorr_bounded_simple_kernel, %d units' % nu)
        np.testing.assert_allclose(cmax, exp_cmax, rtol=0, atol=1e-12, err_msg='xcorr_bounded_simple_kernel, %d units' % nu)


def test_seeded_simple_kernel_at_its_items_of_four():
    """17 elements x W = 65, half-width 9 (the general form of the seeded search): every unit against the slice arg-max of
    tests/seeded_truth.py around the GPU's own grid maxima."""
    N, W, inc, K = 17, 65, 16, 9
    assert _hip.lag_seed_form(N, W, K, 0) == 2
    for nu in uc.unit_counts('range_pick'):
        x = uc.trace(N, W, inc, 7, nu)
        got = _seeded_pass(x, _seeded_geometry(N), W, inc, GRID5, K)
        assert got['lag'].shape[0] == nu
        _seeded_check(got, x, W, [w * inc for w in range(nu)], K)


# ---- solve ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [4, 8])
def test_lts_wave_kernel_at_its_units_of_four(oracle, N):
    assert _hip.route(N, 16)['correlator'] != _hip.ROUTE_SCREEN
    _correlation_case(N, 16, 4, uc.unit_counts('solve_lts_wave'), 'solve_lts_wave_kernel', alpha=0.5, oracle=oracle)


def test_ols_and_uncertainty_kernels_at_their_units_of_64(oracle):
    _correlation_case(5, 16, 4, uc.unit_counts('solve_ols'), 'solve_ols_kernel / uncertainty_kernel', alpha=1.0, oracle=oracle)


@pytest.mark.parametrize('N', [4, 9])
def test_pack_weights_kernel_at_its_items_of_256(oracle, N):
    """4 elements (6 pairs: one mask byte per unit) and 9 (36 pairs: five): unit counts whose (unit, mask byte) items end
    just below, at and just above 256.  Every unit's packed mask against the weight bytes of ``nbls_fetch``."""
    P = N * (N - 1) // 2
    MB = (P + 7) // 8
    for nu in uc.unit_counts('pack_weights', mask_bytes=MB):
        family = 'pack_weights_kernel, %d mask byte(s)' % MB
        res, m, _ = _process(N, 16, 4, nu, 0.5, solve=True)
        _check_correlation(res.lag[0], res.cmax[0], N, 16, 4, m, nu, family, seed=uc.solve_seed(N, 16, 4, m, 0.5))
        _check_solve(oracle, res, N, 0.5, nu, m, family)
        _check_units(_rows(res), nu, m, family)
        wts = res.handle.fetch(grids=False, want_weights=True)['weights']
        assert wts.shape == (1, nu + PAD, P) and set(np.unique(wts[0, :nu])) == {0, 1}
        bits = np.unpackbits(res.mask, axis=-1, bitorder='little')
        np.testing.assert_array_equal(bits[0, :nu, :P], wts[0, :nu], err_msg='%s, %d units' % (family, nu))
        assert not bits[0, :, P:].any()


# ---- a sub-array estimator: gather_pairs_kernel ----------------------------------------------------------------------------
GATHER_REFINED = 5       # the count that also runs with lag refinement


def _gather_case(nu, refined):
    N, W, inc, keep = 4, 16, 4, (0, 1, 2)
    family = 'gather_pairs_kernel' + (' with fractions' if refined else '')
    m = uc.choose_m(nu, N, _cus(), inc)
    x = uc.trace(N, W, inc, m, nu)
    rij = uc.geometry(N)
    ests = engine.normalize_estimators([1.0, (1.0, (3,))], N)
    assert tuple(engine.kept_elements(N, ests[1][1])) == keep
    rijs = [rij, np.ascontiguousarray(rij[:, keep])]
    kw = dict(prefiltered=True, want_lag=True, want_cmax=True, want_uncert=True, want_subsample=refined, vector_len=nu + PAD)
    full, sub = engine.process_multi(list(x), FS, [T0, T0], rijs, [(None, None)], [uc.winlen(W)], uc.overlap(W, inc), ests, **kw)
    one = engine.process(np.ascontiguousarray(x[list(keep)]), FS, T0, rijs[1], [(None, None)], [uc.winlen(W)], uc.overlap(W, inc), 1.0, **kw)
    assert int(full.nwin[0]) == int(sub.nwin[0]) == int(one.nwin[0]) == nu
    _check_correlation(full.lag[0], full.cmax[0], N, W, inc, m, nu, family)
    pmap = engine.kept_pair_map(N, ests[1][1])
    for name in ('lag', 'cmax') + (('lag_frac',) if refined else ()):
        np.testing.assert_array_equal(getattr(sub, name), getattr(full, name)[..., pmap], err_msg='%s, %d units: %s' % (family, nu, name))
    for name in ('lag', 'vel', 'baz', 'sigma_tau', 'mask', 'vel_uncert', 'baz_uncert'):
        np.testing.assert_array_equal(getattr(sub, name), getattr(one, name), err_msg='%s, %d units: %s' % (family, nu, name))
    np.testing.assert_allclose(sub.mdccm, one.mdccm, rtol=0, atol=1e-12, err_msg=family)
    _check_units(_rows(full), nu, m, family + ' (the whole array)')
    _check_units(_rows(sub), nu, m, family)


def test_gather_pairs_kernel_below_and_at_its_workgroup_cap():
    """4 elements with the estimator of elements (0, 1, 2): one trip of 4 units per workgroup up to 32 units per compute unit,
    grid-stride trips with dead waves beyond; against the call on the sub-array, bit for bit."""
    for nu in uc.unit_counts('gather_pairs', _cus()):
        _gather_case(nu, refined=False)


def test_gather_pairs_kernel_gathers_the_fraction_rows():
    _gather_case(GATHER_REFINED, refined=True)



# ---- the kept elements -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', [5, 9, 17])
def test_kept_elements_kernel_at_its_units_per_wave_and_workgroup(N):
    """8, 16 and 32 lanes per unit: 32, 16 and 8 units per workgroup.  Mask and count of every unit against the rule of
    tests/kept_truth.py on the pass's own weights."""
    family = 'kept_elements_kernel<%d>' % uc.kept_lanes(N)
    dropped, q = 0, 2                  # an element is dropped where LTS took the weight of two of its pairs
    for nu in uc.unit_counts('kept_elements', N=N):
        res, m, _ = _process(N, 16, 4, nu, 0.5, kept=(q, False, False))
        mask, count = kt.rule_table(np.asarray(res.weights)[0, :nu], N, q)
        np.testing.assert_array_equal(res.dropped_mask[0, :nu], mask, err_msg='%s, %d units' % (family, nu))
        np.testing.assert_array_equal(res.kept_count[0, :nu], count, err_msg='%s, %d units' % (family, nu))
        _check_correlation(res.lag[0], res.cmax[0], N, 16, 4, m, nu, family)
        _check_units(_rows(res), nu, m, family)
        dropped += int(np.count_nonzero(mask))
        assert nu < 3 or len(np.unique(mask)) > 1, (family, nu)
    assert dropped > 0


# ---- closure and beam -----------------------------------------------------------------------------------------------------
def test_closure_kernel_at_its_units_of_four():
    N, W, inc = 5, 16, 4
    for nu in uc.unit_counts('closure'):
        res, m, _ = _process(N, W, inc, nu, 1.0, want_consistency=True)
        for w in range(nu):
            cons, cmax, el, Q = ct.outputs_int(res.lag[0, w], N, FS)
            assert Q < 2 ** 48
            assert abs(res.consistency[0, w] - cons) <= CLOSURE_REL * cons, ('closure_kernel', nu, w)
            assert abs(res.closure_max[0, w] - cmax) <= CLOSURE_REL * cmax, ('closure_kernel', nu, w)
            assert np.all(np.abs(res.element_consistency[0, w] - el) <= CLOSURE_REL * el), ('closure_kernel', nu, w)
        _check_correlation(res.lag[0], res.cmax[0], N, W, inc, m, nu, 'closure_kernel')
        _check_units(_rows(res), nu, m, 'closure_kernel')


def _beam_case(W, inc, family, taps=0):
    """Every unit against the long-double beam of its own fetched slowness (beam_truth; steer_truth with ``taps``), and the
    units whose reads stay inside the trace bit for bit against each other by template."""
    N, K = 4, taps // 2
    for nu in uc.unit_counts('beam_fstat'):
        res, m, x = _process(N, W, inc, nu, 1.0, want_beam=True, beam_taps=taps)
        if taps:
            ref = steer_truth.beam_reference(x, FS, res.xij, res.z[0], W, inc, nu, taps)
        else:
            ref = beam_truth.beam_reference(x, FS, res.xij, res.z[0], W, inc, nu)
        on_f, skipped = beam_truth.compare(res.beam_power[0, :nu], res.fstat[0, :nu], ref)
        assert on_f >= 1, (family, nu)
        interior = np.zeros(nu, dtype=bool)
        for w in range(nu):
            d = steer_truth.beam_delays(res.xij[:N - 1], res.z[0, w], FS)[0] if taps else beam_truth.delays(res.xij[:N - 1], res.z[0, w], FS)[0]
            interior[w] = w * inc + int(d.min()) - max(K - 1, 0) >= 0 and w * inc + W + int(d.max()) + K <= x.shape[1]
        _check_correlation(res.lag[0], res.cmax[0], N, W, inc, m, nu, family)
        _check_units(_rows(res), nu, m, family, interior=interior)


def test_beam_kernel_at_its_units_of_four_one_wave_per_unit():
    assert 64 <= uc.BEAM_WAVE_W
    _beam_case(64, 16, 'beam_fstat_kernel, one wave per unit')


def test_beam_kernel_at_its_units_of_four_four_waves_per_unit():
    W = uc.BEAM_WAVE_W + 8
    _beam_case(W, uc.hop_for(W), 'beam_fstat_kernel, four waves per unit')


def test_steered_beam_kernel_at_its_units_of_four():
    _beam_case(64, 16, 'beam_fstat_kernel, beam_taps = 4', taps=4)


# ---- one streamed pass ------------------------------------------------------------------------------------------------
def test_screening_batches_with_a_ragged_last_batch(oracle):
    """8 elements x W = 600 with ``screen_batch_mb`` lowered: three equal unit batches whose last is neither a multiple of 8
    nor of 4 — a first unit other than 0 together with a ragged tail in every kernel of the chain."""
    N, W, inc, nu = 8, 600, 100, 250
    batches = uc.screen_batches(nu, N, (W + 15) // 16 * 16, 1)
    assert len(batches) >= 3 and batches[-1] % 4 and sum(batches) == nu, batches
    h = engine.get_handle()
    h.set_option('screen_batch_mb', 1)
    h.set_profiling(True)
    try:
        res, m, _ = _process(N, W, inc, nu, 0.5, solve=True)
        assert h.timings()['xcorr_launches'] == len(batches), (h.timings()['xcorr_launches'], batches)
    finally:
        h.set_profiling(False)
        h.set_option('screen_batch_mb', 192)
    family = 'screening unit batches %s' % batches
    _check_correlation(res.lag[0], res.cmax[0], N, W, inc, m, nu, family, seed=uc.solve_seed(N, W, inc, m, 0.5))
    _check_solve(oracle, res, N, 0.5, nu, m, family)
    _check_units(_rows(res), nu, m, family)
