"""Several recordings of one array in one device pass (``narrow_band_least_squares_batch``, ``ltsva_batch``,
``nbls_set_segments``): every recording's results equal its own single call bit for bit."""
import numpy as np
import pytest

from narrow_band_least_squares_amd import (engine, synthetic, planner, ltsva, ltsva_batch, narrow_band_least_squares,
                                           narrow_band_least_squares_batch)
from narrow_band_least_squares_amd import _hip

pytestmark = pytest.mark.gpu

T0 = 17884.0729166667


def _recordings(N, npts, fs, S, fmin, fmax, lts, seed=500, radius=1.0):
    """S recordings of one N-element array: different noise, back-azimuth and start time each."""
    rij = synthetic.array_geometry(N, radius)
    sts = []
    for i in range(S):
        data = synthetic.plane_wave(rij, npts, fs, fmin, fmax, baz_deg=20.0 + 67.0 * i, timing_error_s=0.25 if lts else 0.0,
                                    bad_element=N - 1 if lts else None, seed=seed + i)
        sts.append(synthetic.make_stream(data, fs, starttime=T0 + 0.0173 * i))
    return sts, rij - rij.mean(axis=1, keepdims=True)


def _case(name):
    """-> (streams factory, argument tuple without the stream) of one of the three shapes of the issue."""
    if name == 'cfg1b':            # OLS, cheby1, adaptive windows (example.py's parameters)
        c = synthetic.build_config('cfg1b', 1.0)
        fr = np.logspace(-2, 1, 64)
        args = (c['WINLEN_list'], 0.5, 1.0, None, None, None, c['NBANDS'], np.zeros(64), np.zeros(64), c['freqlist'],
                'log', fr, 'cheby1', 2, 0.01)
        return (lambda S: _recordings(8, c['npts'], 20.0, S, 0.1, 5.0, False)), args
    if name == 'cfg2':             # LTS alpha 0.75, 6 elements
        c = synthetic.build_config('cfg2', 0.1)
        fr = np.logspace(-2, 1, 32)
        args = (c['WINLEN_list'], 0.5, 0.75, None, None, None, c['NBANDS'], np.zeros(32), np.zeros(32), c['freqlist'],
                'log', fr, 'butter', 2, 0.01)
        return (lambda S: _recordings(6, c['npts'], 20.0, S, 0.1, 5.0, True)), args
    # 12 elements under LTS (the large-array LTS kernel), butter
    freqlist = np.array([0.5, 1.0, 2.0, 4.0])
    fr = np.logspace(-2, 1, 16)
    args = ([30.0, 30.0, 30.0], 0.5, 0.75, None, None, None, 3, np.zeros(16), np.zeros(16), freqlist, 'log', fr, 'butter', 2, 0.01)
    return (lambda S: _recordings(12, 6000, 20.0, S, 0.5, 4.0, True, radius=1.5)), args


def _with(args, st):
    a = list(args)
    a[3] = st
    return a


def _same_nbls(got, exp):
    for i in (0, 1, 2, 3, 5, 7, 8):
        np.testing.assert_array_equal(got[i], exp[i], err_msg='element %d' % i)
    assert got[6] == exp[6]
    if exp[4] is None:
        assert got[4] is None
    else:
        assert list(got[4].keys()) == list(exp[4].keys())
        for k in exp[4]:
            np.testing.assert_array_equal(got[4][k], exp[4][k])


def _independent(outs, idx):
    for i in range(len(outs)):
        for j in range(i + 1, len(outs)):
            for k in idx:
                assert not np.shares_memory(outs[i][k], outs[j][k]), (i, j, k)
    for o in outs:
        for k in idx:
            assert o[k].flags.c_contiguous


@pytest.mark.parametrize('S', [1, 2, 5])
@pytest.mark.parametrize('name', ['cfg1b', 'cfg2', 'lts12'])
def test_batch_equals_single_calls(name, S):
    make, args = _case(name)
    sts, rij = make(S)
    singles = [narrow_band_least_squares(*_with(args, st), rij=rij) for st in sts]
    batch = narrow_band_least_squares_batch(*_with(args, sts), rij=rij)
    assert len(batch) == S
    for got, exp in zip(batch, singles):
        _same_nbls(got, exp)
    _independent(batch, (0, 1, 2, 3, 5, 7, 8))
    if name != 'cfg1b':
        assert any(k != 'size' for k in batch[-1][4])                  # LTS dropped something: the dictionary is exercised
    if S > 1:
        assert not np.array_equal(batch[0][1], batch[1][1])           # (a mix-up of recordings would show)
        assert not np.array_equal(batch[0][3], batch[1][3])


@pytest.mark.parametrize('alpha', [1.0, 0.75])
def test_ltsva_batch_equals_single_calls(alpha):
    sts, rij = _recordings(7, 4000, 20.0, 4, 0.5, 4.0, alpha < 1.0, seed=900)
    singles = [ltsva(st, None, None, 20.0, 0.5, alpha=alpha, rij=rij) for st in sts]
    batch = ltsva_batch(sts, None, None, 20.0, 0.5, alpha=alpha, rij=rij)
    assert len(batch) == len(sts)
    for got, exp in zip(batch, singles):
        for i in (0, 1, 2, 3, 5, 6, 7):
            np.testing.assert_array_equal(got[i], exp[i], err_msg='element %d' % i)
        assert list(got[4].keys()) == list(exp[4].keys())
        for k in exp[4]:
            np.testing.assert_array_equal(got[4][k], exp[4][k])
    _independent(batch, (0, 1, 2, 3, 5, 6, 7))


def test_a_bad_recording_does_not_touch_the_others():
    """One recording holds a NaN sample, another a dead element under LTS: the rest equal their single calls, and the
    two equal theirs too."""
    make, args = _case('cfg2')
    sts, rij = make(4)
    sts[1][2].data[1000] = np.nan
    sts[2][4].data[:] = 0.0
    singles = [narrow_band_least_squares(*_with(args, st), rij=rij) for st in sts]
    batch = narrow_band_least_squares_batch(*_with(args, sts), rij=rij)
    for got, exp in zip(batch, singles):
        _same_nbls(got, exp)
    assert not np.isnan(batch[0][0]).any() and not np.isnan(batch[3][0]).any()


def test_long_windows_take_the_general_correlator_in_a_batch():
    """A window group longer than 13 000 samples (beyond the screening correlator's LDS images): the general correlator
    reads the rows of every recording."""
    sts, rij = _recordings(5, 60000, 100.0, 3, 0.5, 4.0, False, seed=70)
    fr = np.logspace(-2, 1, 8)
    args = ([140.0, 30.0], 0.5, 1.0, None, None, None, 2, np.zeros(8), np.zeros(8), np.array([0.5, 1.0, 2.0]), 'log', fr,
            'butter', 2, 0.01)
    singles = [narrow_band_least_squares(*_with(args, st), rij=rij) for st in sts]
    assert singles[0][6][0] >= 1
    batch = narrow_band_least_squares_batch(*_with(args, sts), rij=rij)
    for got, exp in zip(batch, singles):
        _same_nbls(got, exp)


def test_streamed_rounds_and_sub_batches_equal_the_plain_batch(monkeypatch):
    make, args = _case('cfg2')
    sts, rij = make(4)
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    plain = narrow_band_least_squares_batch(*_with(args, sts), rij=rij)
    h = engine.get_handle()
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '1')
    try:
        h.set_option('screen_batch_mb', 1)            # several result batches that cut through rows of recordings
        h.set_option('solve_min_units', 1)
        streamed = narrow_band_least_squares_batch(*_with(args, sts), rij=rij)
        assert h.result_batches() >= 3
    finally:
        h.set_option('screen_batch_mb', 192)
        h.set_option('solve_min_units', 0)
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    npts, N = len(sts[0][0].data), len(sts[0])
    row = 8.0 * N * (npts + 64)
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', repr(3.5 * 4 * row / 2.0 ** 30))          # 4 recordings: three bands per round
    assert engine.max_bands_per_pass(4 * N, npts) == 3
    rounds = narrow_band_least_squares_batch(*_with(args, sts), rij=rij)
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', repr(2.5 * row / 2.0 ** 30))              # not one band of 4: sub-batches of 2
    assert engine.max_bands_per_pass(4 * N, npts) == 0 and engine.max_bands_per_pass(N, npts) == 2
    subs = narrow_band_least_squares_batch(*_with(args, sts), rij=rij)
    for other in (streamed, rounds, subs):
        for got, exp in zip(other, plain):
            _same_nbls(got, exp)


def _raw_handle_pass(h, sts, rij, prep, band_idx, nseg):
    h.set_segments(nseg)
    h.set_trace_rows([tr.data for st in sts for tr in st], prep.fs)
    h.set_geometry(prep.xij, prep.pair_idx, prep.xpinv)
    h.plan(prep.sos[band_idx], prep.zero_phase, prep.tl, prep.tr, prep.W[band_idx], prep.inc[band_idx], prep.vector_len,
           lts=prep.lts)
    h.execute()
    return h.fetch()


def test_segments_through_the_c_abi():
    """nbls_set_segments + nbls_plan + nbls_fetch: B*S rows in the order b*S + s, each equal to the recording's own pass;
    nbls_result_layout counts B*S*VL cells; every error case returns its status code."""
    S, N = 3, 6
    sts, rij = _recordings(N, 5000, 20.0, S, 0.5, 4.0, True, seed=31)
    edges = [(0.5, 1.0), (1.0, 2.0), (2.0, 4.0)]
    prep = engine.prepare(N, 5000, 20.0, rij, edges, [30.0, 20.0, 20.0], 0.5, 0.75, 'butter', 2, 0.01)
    idx = np.arange(3)
    h = _hip.Handle(engine.default_device())
    try:
        singles = [_raw_handle_pass(h, [st], rij, prep, idx, 1) for st in sts]
        got = _raw_handle_pass(h, sts, rij, prep, idx, S)
        assert got['vel'].shape == (3 * S, prep.vector_len)
        for b in range(3):
            for s in range(S):
                for k in ('vel', 'baz', 'mdccm', 'sigma_tau'):
                    np.testing.assert_array_equal(got[k][b * S + s], singles[s][k][b], err_msg='%s row %d' % (k, b * S + s))
                assert got['nwin'][b * S + s] == singles[s]['nwin'][b]
        lay = (_hip.C.c_int64 * 4)()
        assert h.lib.nbls_result_layout(h._h, lay) == 0
        assert lay[0] == 3 * S * prep.vector_len

        lib, hh = h.lib, h._h
        codes = []
        h._chk = lambda rc: codes.append(rc)           # the raw status codes of the calls below
        assert lib.nbls_set_segments(hh, 0) == _hip.NBLS_ERR_ARG
        assert lib.nbls_set_segments(hh, -2) == _hip.NBLS_ERR_ARG

        def plan_rc(rows, nseg, geometry_of=None, lts=None, ranges=False):
            lib.nbls_set_segments(hh, 1)
            h.set_trace_rows(rows, 20.0)
            assert lib.nbls_set_segments(hh, nseg) == 0
            h.nseg = nseg
            if geometry_of is not None:
                xij, pair_idx, xpinv = planner.co_array(geometry_of)
                h.set_geometry(xij, pair_idx, xpinv)
            if ranges:
                h.set_window_ranges(np.zeros(1, np.int32), -np.ones(1, np.int32))
            del codes[:]
            h.plan(prep.sos[:1], prep.zero_phase, prep.tl, prep.tr, prep.W[:1], prep.inc[:1], prep.vector_len, lts=lts)
            rc = codes[-1]
            if ranges:
                h.set_window_ranges(None)
            return rc

        rows = [tr.data for st in sts for tr in st]                              # 18 rows
        assert plan_rc(rows, 4) == _hip.NBLS_ERR_ARG                              # 18 % 4 != 0
        assert plan_rc(rows[:4], 2) == _hip.NBLS_ERR_GEOMETRY                     # 2 elements per recording
        assert plan_rc([rows[0]] * 66, 2) == _hip.NBLS_ERR_GEOMETRY               # 33 elements per recording
        rij3 = rij[:, :3]
        assert plan_rc(rows[:6], 2, geometry_of=rij3, lts=prep.lts) == _hip.NBLS_ERR_GEOMETRY   # LTS, 3 elements
        assert plan_rc(rows, S, geometry_of=rij, ranges=True) == _hip.NBLS_ERR_UNSUPPORTED
        assert plan_rc(rows, S, geometry_of=rij) == 0
    finally:
        h.close()


def test_batch_against_the_oracle(oracle):
    """One batch against the CPU oracle, recording by recording (tolerances of test_gpu_parity.py)."""
    make, args = _case('cfg2')
    sts, rij = make(3)
    batch = narrow_band_least_squares_batch(*_with(args, sts), rij=rij)
    for st, got in zip(sts, batch):
        ost = oracle.make_stream(np.array([tr.data for tr in st]), st[0].stats.sampling_rate, starttime=st[0].stats.starttime)
        exp = oracle.narrow_band_least_squares(*_with(args, ost), rij=rij)
        assert got[6] == exp[6]
        for i, name in ((0, 'vel'), (1, 'baz'), (2, 'mdccm')):
            np.testing.assert_allclose(got[i], exp[i], rtol=1e-9, atol=0, err_msg=name)
        np.testing.assert_array_equal(got[3], exp[3])
        np.testing.assert_allclose(got[7], exp[7], rtol=1e-13)
        np.testing.assert_allclose(got[8], exp[8], rtol=1e-12, atol=1e-300)
        assert set(got[4].keys()) == set(exp[4].keys())
        for k in got[4]:
            np.testing.assert_array_equal(got[4][k], exp[4][k])
