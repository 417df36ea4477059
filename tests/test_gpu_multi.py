"""Several estimators (ALPHA, removed elements) on one pass's lags (``narrow_band_least_squares_multi``, ``ltsva_multi``,
``nbls_set_estimators``) against the single calls: same array bit for bit, a sub-array against the single call on the
reduced stream (MdCCM within the project's 1e-12: a smaller array may route to another verifier instance)."""
import ctypes

import numpy as np
import pytest

from narrow_band_least_squares_amd import (engine, synthetic, planner, ltsva, ltsva_multi, narrow_band_least_squares,
                                           narrow_band_least_squares_multi, filter_data)
from narrow_band_least_squares_amd import _hip

pytestmark = pytest.mark.gpu

T0 = 17884.0729166667


def _recording(N, npts, fs, fmin, fmax, seed=500, radius=1.0):
    """One recording of an N-element array whose last element is mistimed -> (data, centred rij)."""
    rij = synthetic.array_geometry(N, radius)
    data = synthetic.plane_wave(rij, npts, fs, fmin, fmax, baz_deg=20.0, timing_error_s=0.25, bad_element=N - 1, seed=seed)
    return data, rij - rij.mean(axis=1, keepdims=True)


def _case(name):
    """The three shapes of tests/test_gpu_batch.py -> (data, rij, fs, argument list with ALPHA / stream left open)."""
    if name == 'cfg1b':            # 8 elements, cheby1, adaptive windows
        c = synthetic.build_config('cfg1b', 1.0)
        fr = np.logspace(-2, 1, 64)
        args = [c['WINLEN_list'], 0.5, None, None, None, None, c['NBANDS'], np.zeros(64), np.zeros(64), c['freqlist'],
                'log', fr, 'cheby1', 2, 0.01]
        return _recording(8, c['npts'], 20.0, 0.1, 5.0) + (20.0, args)
    if name == 'cfg2':             # 6 elements, butter
        c = synthetic.build_config('cfg2', 0.1)
        fr = np.logspace(-2, 1, 32)
        args = [c['WINLEN_list'], 0.5, None, None, None, None, c['NBANDS'], np.zeros(32), np.zeros(32), c['freqlist'],
                'log', fr, 'butter', 2, 0.01]
        return _recording(6, c['npts'], 20.0, 0.1, 5.0) + (20.0, args)
    freqlist = np.array([0.5, 1.0, 2.0, 4.0])          # 12 elements: the bucket LTS kernel
    fr = np.logspace(-2, 1, 16)
    args = [[30.0, 30.0, 30.0], 0.5, None, None, None, None, 3, np.zeros(16), np.zeros(16), freqlist, 'log', fr, 'butter', 2, 0.01]
    return _recording(12, 6000, 20.0, 0.5, 4.0, radius=1.5) + (20.0, args)


def _with(args, alpha, st):
    a = list(args)
    a[2], a[3] = alpha, st
    return a


def _kept(N, remove):
    return [i for i in range(N) if i not in remove]


def _single(args, data, rij, fs, alpha, remove=()):
    """The project's single call at ``alpha`` on the stream without ``remove``, with ``rij[:, kept]``."""
    kept = _kept(len(data), remove)
    st = synthetic.make_stream(data[kept], fs, starttime=T0)
    return narrow_band_least_squares(*_with(args, alpha, st), rij=np.ascontiguousarray(rij[:, kept]))


def _same_dict(got, exp):
    if exp is None:
        assert got is None
        return
    assert list(got.keys()) == list(exp.keys())
    for k in exp:
        np.testing.assert_array_equal(got[k], exp[k])


def _same_nbls(got, exp, exact_mdccm=True):
    for i in (0, 1, 3, 5, 7, 8):
        np.testing.assert_array_equal(got[i], exp[i], err_msg='element %d' % i)
    if exact_mdccm:
        np.testing.assert_array_equal(got[2], exp[2], err_msg='mdccm')
    else:
        print('max |mdccm - single| = %.3g' % float(np.max(np.abs(got[2] - exp[2]))))
        np.testing.assert_allclose(got[2], exp[2], rtol=0, atol=1e-12, err_msg='mdccm')
    assert got[6] == exp[6]
    _same_dict(got[4], exp[4])


@pytest.mark.parametrize('name', ['cfg1b', 'cfg2', 'lts12'])
def test_same_array_several_alpha(name):
    data, rij, fs, args = _case(name)
    ests = [1.0, 0.75, 0.5]
    st = synthetic.make_stream(data, fs, starttime=T0)
    multi = narrow_band_least_squares_multi(*_with(args, ests, st), rij=rij)
    assert len(multi) == 3
    singles = [_single(args, data, rij, fs, a) for a in ests]
    for got, exp in zip(multi, singles):
        _same_nbls(got, exp)
    assert multi[0][4] is None and not multi[1][5].any() and not multi[2][5].any()
    # the inputs' condition: LTS dropped something at alpha 0.5, so the dictionaries compared above are not empty
    assert len(singles[2][4]) > 1 and 'size' in singles[2][4]
    for a in range(3):
        for b in range(a + 1, 3):
            for k in (0, 1, 2, 3, 5, 7, 8):
                assert not np.shares_memory(multi[a][k], multi[b][k]), (a, b, k)


SUBSETS = {
    8: [(0.5, ()), (1.0, (7,)), (0.75, (7,)), (1.0, (0, 3))],
    12: [(0.75, ()), (0.75, (11,)), (1.0, (2, 5, 11))],
}


@pytest.mark.parametrize('N', [8, 12])
def test_element_subsets(N):
    data, rij, fs, args = _case('cfg1b' if N == 8 else 'lts12')
    ests = SUBSETS[N]
    st = synthetic.make_stream(data, fs, starttime=T0)
    multi = narrow_band_least_squares_multi(*_with(args, ests, st), rij=rij)
    assert len(multi) == len(ests)
    for got, (alpha, remove) in zip(multi, ests):
        exp = _single(args, data, rij, fs, alpha, remove)
        _same_nbls(got, exp, exact_mdccm=not remove)
        if alpha < 1.0:
            assert got[4]['size'] == N - len(remove)
    assert len(multi[0][4]) > 1                       # the full array's LTS names the mistimed element


@pytest.mark.parametrize('N', [8, 12])
def test_subset_lags_are_the_reduced_calls_lags(N):
    """``engine.process_multi`` with the side arrays against ``engine.process`` on the reduced rows: lags exact, cmax
    within 1e-12, and the compact rows are the full pass's rows at ``kept_pair_map``."""
    data, rij, fs, _ = _case('cfg1b' if N == 8 else 'lts12')
    ests = engine.normalize_estimators(SUBSETS[N], N)
    edges, winlens = [(0.5, 1.0), (1.0, 2.0)], [30.0, 20.0]
    rijs = [np.ascontiguousarray(rij[:, _kept(N, rm)]) for _, rm in ests]
    multi = engine.process_multi(list(data), fs, [T0] * len(ests), rijs, edges, winlens, 0.5, ests, 'butter', 2, 0.01,
                                 want_lag=True, want_cmax=True)
    full = next(r for r, (_, rm) in zip(multi, ests) if not rm)
    for res, (alpha, remove), r in zip(multi, ests, rijs):
        one = engine.process(np.ascontiguousarray(data[_kept(N, remove)]), fs, T0, r, edges, winlens, 0.5, alpha, 'butter', 2,
                             0.01, want_lag=True, want_cmax=True)
        assert res.lag.shape == one.lag.shape and res.lag.any()
        np.testing.assert_array_equal(res.lag, one.lag)
        np.testing.assert_allclose(res.cmax, one.cmax, rtol=0, atol=1e-12)
        np.testing.assert_array_equal(res.lag, full.lag[..., engine.kept_pair_map(N, remove)])
        np.testing.assert_array_equal(res.cmax, full.cmax[..., engine.kept_pair_map(N, remove)])
        for name in ('vel', 'baz', 'sigma_tau', 't', 'mask'):
            np.testing.assert_array_equal(getattr(res, name), getattr(one, name), err_msg=name)


@pytest.mark.parametrize('ests', [[1.0, 0.75, 0.5], SUBSETS[8]])
def test_ltsva_multi_equals_single_calls(ests):
    data, rij = _recording(8, 6000, 20.0, 0.5, 4.0, seed=900)
    stf, fs, _ = filter_data(synthetic.make_stream(data, 20.0, starttime=T0), 'butter', 0.5, 4.0, 2, 0.01)
    multi = ltsva_multi(stf, None, None, 20.0, 0.5, ests, rij=rij)
    assert len(multi) == len(ests)
    for got, e in zip(multi, engine.normalize_estimators(ests, 8)):
        alpha, remove = e
        kept = _kept(8, remove)
        exp = ltsva([stf[i] for i in kept], None, None, 20.0, 0.5, alpha=alpha, rij=np.ascontiguousarray(rij[:, kept]))
        for i in (0, 1, 2, 5, 6, 7):             # vel, baz, t, sigma_tau and both confidence intervals: exact
            np.testing.assert_array_equal(got[i], exp[i], err_msg='element %d' % i)
        if remove:
            np.testing.assert_allclose(got[3], exp[3], rtol=0, atol=1e-12)
        else:
            np.testing.assert_array_equal(got[3], exp[3])
        _same_dict(got[4], exp[4])
    assert any(k != 'size' for k in multi[-2][4]) or any(k != 'size' for k in multi[0][4])


def test_streamed_and_unstreamed_are_identical(monkeypatch):
    data, rij, fs, args = _case('lts12')
    ests = SUBSETS[12]
    st = synthetic.make_stream(data, fs, starttime=T0)
    outs = []
    for flag in ('1', '0'):
        monkeypatch.setenv('NBLS_STREAM_RESULTS', flag)
        outs.append(narrow_band_least_squares_multi(*_with(args, ests, st), rij=rij))
    monkeypatch.delenv('NBLS_STREAM_RESULTS')
    for a, b in zip(*outs):
        _same_nbls(a, b)
    for got, (alpha, remove) in zip(outs[0], ests):
        _same_nbls(got, _single(args, data, rij, fs, alpha, remove), exact_mdccm=not remove)


def test_hbm_rounds(monkeypatch):
    data, rij, fs, args = _case('cfg2')
    ests = [(0.5, ()), 1.0, (0.75, (5,))]
    st = synthetic.make_stream(data, fs, starttime=T0)
    whole = narrow_band_least_squares_multi(*_with(args, ests, st), rij=rij)
    N, npts = data.shape
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', repr(1.5 * 8.0 * N * (npts + 64) / 2.0 ** 30))
    assert engine.max_bands_per_pass(N, npts) == 1 and args[6] >= 2           # one band per round
    rounds = narrow_band_least_squares_multi(*_with(args, ests, st), rij=rij)
    for a, b in zip(rounds, whole):
        _same_nbls(a, b)
    for got, e in zip(rounds, engine.normalize_estimators(ests, N)):
        _same_nbls(got, _single(args, data, rij, fs, e[0], e[1]), exact_mdccm=not e[1])


# ---- C ABI -------------------------------------------------------------------------------------------------------

def _extra(rij, N, alpha, remove):
    kept = _kept(N, remove)
    xij, pair_idx, xpinv = planner.co_array(np.ascontiguousarray(rij[:, kept]))
    return dict(kept=kept, xij=xij, pair_idx=pair_idx, xpinv=xpinv, lts=planner.lts_plan(xij, alpha) if alpha < 1.0 else None,
                eig6=None)


def _plain_pass(h, data, fs, rij, estimators=None):
    prep = engine.prepare(len(data), data.shape[1], fs, rij, [(0.5, 1.0), (1.0, 2.0)], [30.0, 20.0], 0.5, 0.75, 'butter', 2, 0.01)
    engine.launch(h, data, prep, estimators=estimators)
    h.sync()


def test_c_abi_estimator_zero_and_reset():
    data, rij, fs, _ = _case('cfg1b')
    data = np.ascontiguousarray(data[:, :6000])
    fresh = _hip.Handle()
    _plain_pass(fresh, data, fs, rij)
    ref = fresh.fetch_packed()
    ref_side = fresh.fetch(want_lag=True, want_cmax=True, want_weights=True, want_z=True)
    fresh.close()

    h = _hip.Handle()
    _plain_pass(h, data, fs, rij, [_extra(rij, 8, 0.5, ()), _extra(rij, 8, 1.0, (7,))])
    lay0, lay = (ctypes.c_int64 * 4)(), (ctypes.c_int64 * 4)()
    assert h.lib.nbls_result_layout(h._h, lay0) == 0 and h.lib.nbls_est_result_layout(h._h, 0, lay) == 0
    assert list(lay0) == list(lay)
    a, b = np.zeros(lay[2], dtype=np.uint8), np.ones(lay[2], dtype=np.uint8)
    assert h.lib.nbls_fetch_packed(h._h, a.ctypes.data, lay[2]) == 0
    assert h.lib.nbls_est_fetch_packed(h._h, 0, b.ctypes.data, lay[2]) == 0
    assert a.tobytes() == b.tobytes()
    old = h.fetch(want_lag=True, want_cmax=True, want_weights=True, want_z=True)
    new = {k: np.empty_like(old[k]) for k in old}
    ptr = {'nwin': _hip._iptr, 'lag': _hip._iptr, 'weights': _hip._u8ptr}
    assert h.lib.nbls_est_fetch(h._h, 0, *[ptr.get(k, _hip._dptr)(new[k]) for k in
                                           ('vel', 'baz', 'mdccm', 'sigma_tau', 'nwin', 'lag', 'cmax', 'weights', 'z')]) == 0
    for k in old:
        assert old[k].tobytes() == new[k].tobytes(), k
    # estimator 0 is untouched by the further ones; estimator 2's compact rows have 21 pairs
    for k in ('vel', 'baz', 'mdccm', 'sigma_tau', 'mask'):
        assert h.fetch_packed()[k].tobytes() == ref[k].tobytes(), k
    sub = h.fetch(est=2, want_lag=True, want_weights=True)
    assert sub['lag'].shape[-1] == 21 and h.fetch_packed(est=2)['mask'].shape[-1] == 3
    np.testing.assert_array_equal(sub['lag'], ref_side['lag'][..., engine.kept_pair_map(8, (7,))])
    with pytest.raises(ValueError):
        h.fetch_packed(est=3)
    # reset to zero estimators: the next plain pass gives the bytes of a fresh handle
    _plain_pass(h, data, fs, rij)
    assert h.est_npairs == []
    again = h.fetch_packed()
    for k in ('vel', 'baz', 'mdccm', 'sigma_tau', 'mask'):
        assert again[k].tobytes() == ref[k].tobytes(), k
    side = h.fetch(want_lag=True, want_cmax=True, want_weights=True, want_z=True)
    for k in ('lag', 'cmax', 'weights', 'z'):
        assert side[k].tobytes() == ref_side[k].tobytes(), k
    with pytest.raises(ValueError):
        h.fetch_packed(est=1)
    h.close()


def test_c_abi_error_codes():
    """Argument checks only: every call returns before anything is launched, and a refused call leaves the handle's
    estimators as they were."""
    data, rij, fs, _ = _case('cfg1b')
    data = np.ascontiguousarray(data[:, :4000])
    h = _hip.Handle()
    h.set_trace(data, fs)

    def code(ests):
        descs, keep, _ = _hip.estimator_descs(ests)
        return h.lib.nbls_set_estimators(h._h, len(ests), descs)

    good = _extra(rij, 8, 1.0, (7,))
    assert code([good]) == 0
    two = dict(good, kept=[0, 1], xij=np.ones((1, 2)), pair_idx=np.array([[0, 1]]), xpinv=np.ones((2, 1)))
    assert code([two]) == _hip.NBLS_ERR_GEOMETRY
    three = _extra(rij, 8, 1.0, (0, 1, 2, 3, 4))
    assert code([three]) == 0
    assert code([dict(three, lts=planner.lts_plan(_extra(rij, 8, 1.0, (0, 1, 2, 3))['xij'], 0.75))]) == _hip.NBLS_ERR_GEOMETRY
    assert code([dict(good, kept=[0, 1, 2, 3, 4, 5, 8])]) == _hip.NBLS_ERR_ARG          # out of range
    assert code([dict(good, kept=[0, 1, 2, 3, 4, 5, -1])]) == _hip.NBLS_ERR_ARG
    assert code([dict(good, kept=[0, 1, 2, 3, 4, 5, 5])]) == _hip.NBLS_ERR_ARG          # given twice
    assert code([dict(good, kept=[0, 1, 2, 3, 5, 4, 6])]) == _hip.NBLS_ERR_ARG          # not ascending
    assert code([good] * 9) == _hip.NBLS_ERR_UNSUPPORTED
    assert code([good] * 8) == 0
    # a refused list changes nothing: the eight accepted ones are still there
    assert code([good, two]) == _hip.NBLS_ERR_GEOMETRY
    h.set_geometry(*planner.co_array(rij))
    prep = engine.prepare(8, data.shape[1], fs, rij, [(0.5, 1.0)], [30.0], 0.5, 1.0, 'butter', 2, 0.01)
    h.plan(prep.sos, prep.zero_phase, prep.tl, prep.tr, prep.W, prep.inc, prep.vector_len)
    lay = (ctypes.c_int64 * 4)()
    assert h.lib.nbls_est_result_layout(h._h, 8, lay) == 0 and lay[1] == 3
    assert h.lib.nbls_est_result_layout(h._h, 9, lay) == _hip.NBLS_ERR_ARG
    assert code([]) == 0                                                                # a count of zero resets
    # together with segments, window ranges
    h.set_segments(2)
    assert code([good]) == _hip.NBLS_ERR_UNSUPPORTED
    h.set_segments(1)
    h.set_window_ranges([0], [1])
    assert code([good]) == _hip.NBLS_ERR_UNSUPPORTED
    h.set_window_ranges(None)
    assert code([good]) == 0
    h.set_segments(2)                                                                   # ... whichever was set first
    with pytest.raises(ValueError):
        h.plan(prep.sos, prep.zero_phase, prep.tl, prep.tr, prep.W, prep.inc, prep.vector_len)
    h.set_segments(1)
    assert code([]) == 0
    h.close()
