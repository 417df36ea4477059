"""The correlators at every window length where their route changes (nbls_route_xcorr: tiling, LDS layout, kernel
instance), against a host FP64 / extended-precision reference of the oracle's definition

    cij = np.correlate(a, b, 'full') / sqrt(sum a^2 * sum b^2),  cmax = max cij,  lag = W - 1 - (first arg-max)

(oracle/nbls_oracle.py: correlate_windows).  The window lengths come from route_boundaries: both sides of every
change of the automatic route, for array sizes that cover all partners in one workgroup, partner groups, more than 16
elements, the eight-tile screening instance and the DMA verifier.  The samples go in prefiltered, so the reference sees
the very bytes the kernels read.  Inputs alternate white noise (the arg-max anywhere among the 2W - 1 lags) and a
plane wave."""
import numpy as np
import pytest

from narrow_band_least_squares_amd import _hip, engine, planner, synthetic

pytestmark = pytest.mark.gpu

NS = (3, 4, 5, 6, 8, 12, 16, 17, 24, 32)
EXTRA_W = (2, 3, 31, 63, 64, 65)
GAP = 1e-12             # the best lag of every pair must beat the second best by this much of |a| |b|
SHORT = 4096            # N * W up to this: the oracle's own correlate_windows checks the reference


def _windows(n):
    return sorted({w for p in _hip.route_boundaries(n) for w in p} | set(EXTRA_W))


def _data(n, W, k):
    """Two windows (hop W) of n channels: white noise for even k, a plane wave for odd k."""
    npts = 2 * W + 1 + (k % 3)
    if k % 2 == 0:
        return np.random.default_rng(1000 * n + k).standard_normal((n, npts))
    rij = synthetic.array_geometry(n, 1.0, seed=n)
    return synthetic.plane_wave(rij, npts, 1.0, 0.02, 0.2, snr_db=10.0, seed=2000 * n + k)


def _reference(x, W, nwin, pairs):
    """-> lag (nwin, P) int, cmax (nwin, P): all 2W - 1 lags with an FP64 FFT, the lags within 1e-9 |a| |b| of the
    maximum evaluated again with extended-precision dot products; the first of the exact maxima wins."""
    P = len(pairs)
    lag = np.empty((nwin, P), dtype=np.int64)
    cmax = np.empty((nwin, P))
    L = 1 << int(np.ceil(np.log2(2 * W - 1)))
    for w in range(nwin):
        seg = x[:, w * W:(w + 1) * W]
        F = np.fft.rfft(seg, L, axis=1)
        c = np.fft.irfft(F[pairs[:, 0]] * np.conj(F[pairs[:, 1]]), L, axis=1)
        full = np.concatenate((c[:, L - (W - 1):], c[:, :W]), axis=1)         # index k = lag shift k - (W - 1)
        sl = seg.astype(np.longdouble)
        ss = np.sum(sl * sl, axis=1)
        nrm = np.sqrt(ss[pairs[:, 0]] * ss[pairs[:, 1]])
        top = full.max(axis=1)
        for p, (i, j) in enumerate(pairs):
            ks = np.flatnonzero(full[p] >= top[p] - 1e-9 * float(nrm[p]))
            a, b = sl[i], sl[j]
            vals = []
            for kk in ks:
                d = int(kk) - (W - 1)
                vals.append(np.dot(a[d:], b[:W - d]) if d >= 0 else np.dot(a[:W + d], b[-d:]))
            vals = np.array(vals)
            best = int(np.argmax(vals))
            if len(vals) > 1:
                second = np.max(np.delete(vals, best))
                assert vals[best] - second > GAP * nrm[p], 'window %d pair %d: two lags within %g of each other' % (w, p, GAP)
            lag[w, p] = (W - 1) - int(ks[best])
            cmax[w, p] = float(vals[best] / nrm[p])
    return lag, cmax


def _run(x, W, rij, impl):
    return engine.process(x, 1.0, 0.0, rij, [(None, None)], [float(W)], 0.0, 1.0, prefiltered=True, want_lag=True,
                          want_cmax=True, xcorr_impl=impl)


def _check_case(oracle, n, W, k, impls=(0, 1), expect_rejected=()):
    x = _data(n, W, k)
    rij = synthetic.array_geometry(n, 1.0, seed=n)
    rij = rij - rij.mean(axis=1, keepdims=True)
    pairs = planner.pair_table(n)
    npts = x.shape[1]
    nwin = planner.window_plan(npts, 1.0, float(W), 0.0)[2]
    assert nwin >= 2
    lag_r, cmax_r = _reference(x, W, nwin, pairs)
    if n * W <= SHORT:
        tau_o, _, cmax_o = oracle.correlate_windows(x.T, W, np.arange(nwin) * W, [tuple(p) for p in pairs], 1.0)
        np.testing.assert_array_equal(lag_r, np.rint(tau_o.T).astype(int))
        np.testing.assert_allclose(cmax_r, cmax_o.T, rtol=1e-13, atol=1e-15)
    npts_pad = (npts + 63) // 64 * 64
    h = engine.get_handle()
    out = {}
    for impl in impls:
        r = _hip.route(n, W, npts_pad=npts_pad, xcorr_impl=impl)
        msg = 'N=%d W=%d impl=%d route=%s' % (n, W, impl, r)
        if impl in expect_rejected:
            assert r['correlator'] == _hip.ROUTE_REJECTED, msg
            with pytest.raises(_hip.NblsError):
                _run(x, W, rij, impl)
            continue
        assert r['correlator'] != _hip.ROUTE_REJECTED, msg
        h.set_profiling(True)
        try:
            res = _run(x, W, rij, impl)
            assert h.timings()['xcorr_impl'] == r['impl'], msg
        finally:
            h.set_profiling(False)
        np.testing.assert_array_equal(res.lag[0, :nwin], lag_r, err_msg=msg)
        np.testing.assert_allclose(res.cmax[0, :nwin], cmax_r, rtol=1e-12, atol=1e-15, err_msg=msg)
        out[impl] = res
    if 1 in out:
        for impl, res in out.items():
            np.testing.assert_array_equal(res.vel, out[1].vel, err_msg='N=%d W=%d impl=%d' % (n, W, impl))
            np.testing.assert_array_equal(res.baz, out[1].baz, err_msg='N=%d W=%d impl=%d' % (n, W, impl))


@pytest.mark.parametrize('n', NS)
def test_every_route_boundary_against_the_fp64_reference(oracle, n):
    """Both sides of every change of the automatic route, and the shortest windows (W < 64 never screens): the automatic
    correlator and the VALU kernel give the reference's lags and maxima, and the same slowness."""
    for k, W in enumerate(_windows(n)):
        _check_case(oracle, n, W, k)


@pytest.mark.parametrize('n', (3, 8))
def test_valu_kernel_where_its_windows_leave_lds(oracle, n):
    """xcorr_simple_kernel keeps both windows in LDS up to W = 10 235 (2 * W * 8 B + its 80 B of static LDS) and reads
    them from global memory beyond: W = 10 236..10 240 used to fail to launch."""
    for k, W in enumerate(range(10235, 10242)):
        _check_case(oracle, n, W, k, impls=(1,))


@pytest.mark.parametrize('n', (3, 5, 8))
def test_f64_mfma_kernel_at_its_lds_limit(oracle, n):
    """The last window length the f64-MFMA kernel takes, and the first it refuses (a forced xcorr_impl=2 then fails
    loudly instead of falling back)."""
    (w0, w1), = _hip.route_boundaries(n, xcorr_impl=2)
    _check_case(oracle, n, w0, 0, impls=(2, 1))
    _check_case(oracle, n, w1, 1, impls=(2, 1), expect_rejected=(2,))


def test_batch_of_recordings_at_a_dma_verifier_boundary():
    """Three recordings in one pass (nbls_set_segments): the DMA verifier's LDS holds a W / inc table entry per result
    row, so a batch sits closer to the verifier's LDS limit than a single recording.  Both sides of that limit, every
    recording's rows against the reference."""
    n, S = 3, 3
    (w0, w1), = [p for p in _hip.route_boundaries(n)
                 if _hip.route(n, p[0])['verifier'] == 1 and _hip.route(n, p[1])['verifier'] != 1]
    rij = synthetic.array_geometry(n, 1.0, seed=n)
    rij = rij - rij.mean(axis=1, keepdims=True)
    pairs = planner.pair_table(n)
    h = engine.get_handle()
    for k, W in enumerate((w0, w1)):
        recs = [_data(n, W, 2 * k + s) for s in range(S)]
        recs = [r[:, :2 * W + 1] for r in recs]
        npts = 2 * W + 1
        assert _hip.route(n, W, vrows=S, npts_pad=(npts + 63) // 64 * 64)['verifier'] == (1 if W == w0 else 2)
        prep = engine.prepare(n, npts, 1.0, rij, [(None, None)], [float(W)], 0.0, 1.0, prefiltered=True)
        try:
            h.set_segments(S)
            h.set_trace_rows([row for r in recs for row in np.ascontiguousarray(r)], 1.0)
            h.set_geometry(prep.xij, prep.pair_idx, prep.xpinv)
            h.plan(None, prep.zero_phase, prep.tl, prep.tr, prep.W, prep.inc, prep.vector_len, lts=None)
            h.execute()
            got = h.fetch(want_lag=True, want_cmax=True)
        finally:
            h.set_segments(1)
        nwin = int(prep.nwin[0])
        for s in range(S):
            lag_r, cmax_r = _reference(recs[s], W, nwin, pairs)
            np.testing.assert_array_equal(got['lag'][s, :nwin], lag_r, err_msg='W=%d recording %d' % (W, s))
            np.testing.assert_allclose(got['cmax'][s, :nwin], cmax_r, rtol=1e-12, atol=1e-15)
