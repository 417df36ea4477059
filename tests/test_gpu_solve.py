"""The solve kernels (csrc/solve.hip, solve_bucket.inc, lts_bucket*.h: every FAST-LTS instance, OLS, the uncertainty
kernel, pack_weights_kernel) on lag tables chosen for their edges: exact fits, MAD(tau) = 0, lags at +-(W - 1), mistimed
elements at and past the breakdown point, a single pair off closure, vertical incidence under OLS.

The tables are traces of unit pulses (tests/solve_truth.py): a pre-filtered pass with hop = W = 64 hands them to the
correlators as they are, and the lags that come back ARE the designed table — the first assertion of every case, a
correlator finding if it fails.  Everything behind it is judged on the GPU's own fetched lags: against the oracle's
``fast_lts`` + ``lts_post_process`` / ``ols_solve`` on those lags (weights and NaN pattern exact, the rest within the
tolerances of tests/test_gpu_parity.py: _compare_ltsva), and, under OLS, against the exact-rational truth within its
derived rounding bounds.  tests/test_solve_truth.py asserts on the CPU that the tables reach the paths they were built
for, for every (N, ALPHA) used here."""
from fractions import Fraction

import numpy as np
import pytest

import solve_truth as st
from narrow_band_least_squares_amd import engine, planner

pytestmark = pytest.mark.gpu

T0 = 17884.0729166667
PAD = 3                 # result cells behind the last window: they stay zero
GRIDS = ('vel', 'baz', 'mdccm', 'sigma_tau', 'vel_uncert', 'baz_uncert')


def _process(N, alpha, tabs, **kw):
    """One pre-filtered pass over the pulse trace -> (result, nwin, xij, xpinv); the fetched lags are the designed ones."""
    x = st.pulse_trace(tabs)
    rij = st.grid_geometry(N)
    n = len(tabs)
    res = engine.process(x, st.FS, T0, rij, [(None, None)], [st.W / st.FS], 0.0, alpha, prefiltered=True, want_lag=True,
                         want_cmax=True, want_z=True, want_uncert=True, vector_len=n + PAD, **kw)
    assert int(res.nwin[0]) == n
    lag, cmax = st.designed_lags(tabs)
    names = [t for t, _ in tabs]
    for w in range(n):
        np.testing.assert_array_equal(res.lag[0, w], lag[w], err_msg='CORRELATOR finding, not a solve finding: N=%d window %d '
                                      '(%s): the fetched lags are not the designed table' % (N, w, names[w]))
    np.testing.assert_allclose(res.cmax[0, :n], cmax, rtol=1e-12, atol=0, err_msg='CORRELATOR finding: cmax, N=%d' % N)
    xij, _, xpinv = planner.co_array(rij)
    return res, n, xij, xpinv


def _check_padding(res, n):
    for k in GRIDS + ('z', 'lag', 'cmax', 'mask'):
        assert not np.any(getattr(res, k)[0, n:]), 'solve: %s is not zero behind the last window' % k


def _check_against_oracle(oracle, res, n, xij, z_o, sig_o, names, tag):
    """z, vel, baz, sigma_tau, MdCCM and both confidence intervals against the oracle's values on the same lags."""
    def msg(what):
        return 'SOLVE finding (%s): %s; windows: %s' % (tag, what, names)
    vel_o, baz_o = oracle.vel_baz(z_o)
    for what, got, exp in (('z', res.z[0, :n], z_o.T), ('sigma_tau', res.sigma_tau[0, :n], sig_o),
                           ('vel', res.vel[0, :n], vel_o), ('baz', res.baz[0, :n], baz_o)):
        np.testing.assert_array_equal(np.isnan(got), np.isnan(exp), err_msg=msg('NaN pattern of ' + what))
        np.testing.assert_array_equal(np.isinf(got), np.isinf(exp), err_msg=msg('inf pattern of ' + what))
    np.testing.assert_allclose(res.z[0, :n], z_o.T, rtol=1e-9, atol=1e-14, equal_nan=True, err_msg=msg('z'))
    np.testing.assert_allclose(res.vel[0, :n], vel_o, rtol=1e-9, equal_nan=True, err_msg=msg('vel'))
    np.testing.assert_allclose(res.baz[0, :n], baz_o, rtol=1e-9, equal_nan=True, err_msg=msg('baz'))
    np.testing.assert_allclose(res.sigma_tau[0, :n], sig_o, rtol=1e-7, atol=1e-12, equal_nan=True, err_msg=msg('sigma_tau'))
    with np.errstate(invalid='ignore'):
        np.testing.assert_allclose(res.mdccm[0, :n], np.nanmedian(res.cmax[0, :n], axis=1), rtol=1e-12, err_msg=msg('mdccm'))
    # the closed form on the GPU's own z and sigma_tau (rounding only), then the oracle's dense sampling end to end
    cv, cb = oracle.confidence_intervals_closed_form(xij, res.z[0, :n].T, res.sigma_tau[0, :n])
    np.testing.assert_allclose(res.vel_uncert[0, :n], cv, rtol=1e-9, atol=1e-15, equal_nan=True, err_msg=msg('vel_uncert'))
    np.testing.assert_allclose(res.baz_uncert[0, :n], cb, rtol=1e-9, atol=1e-10, equal_nan=True, err_msg=msg('baz_uncert'))
    dv, db = oracle.confidence_intervals(xij, z_o, sig_o, nphi=20000)
    np.testing.assert_allclose(res.vel_uncert[0, :n], dv, rtol=1e-4, atol=1e-12, equal_nan=True, err_msg=msg('vel_uncert, dense'))
    np.testing.assert_allclose(res.baz_uncert[0, :n], db, rtol=1e-4, atol=1e-7, equal_nan=True, err_msg=msg('baz_uncert, dense'))
    _check_padding(res, n)


def _lts_case(oracle, N, alpha):
    tabs = st.tables(N)
    names = [t for t, _ in tabs]
    res, n, xij, _ = _process(N, alpha, tabs)
    r = st.oracle_lts(oracle, res.lag[0, :n], xij, alpha)            # the GPU's own lags; no second correlation
    tag = 'LTS N=%d alpha=%g' % (N, alpha)
    for w in range(n):
        np.testing.assert_array_equal(res.weights[0, w], r['weights'][:, w],
                                      err_msg='SOLVE finding (%s): weights of window %d (%s)' % (tag, w, names[w]))
    _check_against_oracle(oracle, res, n, xij, r['z'], r['sigma_tau'], names, tag)
    return res


@pytest.mark.parametrize('N,alpha', st.LTS_REGISTER)
def test_lts_register_kernel(oracle, N, alpha):
    """4..8 elements: solve_lts_wave_kernel<P, HALF> at ALPHA = 0.5 (the instance pruned to h of 0.5) and the generic
    <P, 0> at 0.75, every table."""
    P = N * (N - 1) // 2
    assert planner.lts_h(P, 0.5) == st.half_h(P)
    assert (planner.lts_h(P, alpha) != st.half_h(P)) == (alpha != 0.5)
    _lts_case(oracle, N, alpha)


@pytest.mark.parametrize('N,alpha', st.LTS_BUCKET)
def test_lts_bucket_kernel(oracle, N, alpha):
    """9 elements (36 pairs, the smallest), 12 at ALPHA = 0.75, 16, 23 (253 pairs: the last size with u8 counters and
    subset merging), 24 (276: the first with u16 counters and none) and 32 (496).  More than h keys that are all
    (nearly) zero — the exact-fit rows — are the bucket selection's worst input."""
    _lts_case(oracle, N, alpha)


def _variant(N, alpha, option):
    tabs = st.tables(N)
    a, n, _, _ = _process(N, alpha, tabs)
    h = engine.get_handle()
    h.set_option(option, 1)
    try:
        b, _, _, _ = _process(N, alpha, tabs)
    finally:
        h.set_option(option, 0)
    for k in ('z', 'weights', 'sigma_tau', 'vel', 'baz'):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k), err_msg='N=%d %s=1: %s' % (N, option, k))
    assert np.isnan(a.z[0, :n]).any() and np.isfinite(a.z[0, :n]).any()          # both kinds of window were compared


@pytest.mark.parametrize('N', [8, 9, 23, 24, 32])
def test_generic_lane_per_start_kernel_agrees(N):
    """Option lts_impl = 1 (solve_lts_kernel) against the default kernel of the size, bit for bit."""
    _variant(N, 0.5, 'lts_impl')


@pytest.mark.parametrize('N', [4, 5, 6, 7, 8])
def test_generic_h_instance_agrees(N):
    """Option lts_generic_h = 1 (<P, 0> also at the h of ALPHA = 0.5) against the pruned instance, bit for bit."""
    _variant(N, 0.5, 'lts_generic_h')


@pytest.mark.parametrize('N', st.OLS_N)
def test_ols(oracle, N):
    """3, 8, 11 (55 pairs: the MdCCM columns in LDS), 12 (66: not) and 32 elements, every table: against the oracle, and
    against the exact-rational truth within the derived bounds of tests/solve_truth.py."""
    tabs = st.tables(N, slowness=st.SLOWNESS, nrandom=4, short=False)
    names = [t for t, _ in tabs]
    res, n, xij, xpinv = _process(N, 1.0, tabs)
    P = len(xij)
    tau = np.ascontiguousarray(res.lag[0, :n].T / st.FS)
    z_o, _, _, sig_o = oracle.ols_solve(xij, tau)
    tag = 'OLS N=%d' % N
    assert np.all(np.unpackbits(res.mask[0, :n], axis=-1, bitorder='little')[:, :P] == 1), 'SOLVE finding (%s): weights' % tag
    _check_against_oracle(oracle, res, n, xij, z_o, sig_o, names, tag)
    for w, name in enumerate(names):
        t = st.ols_truth(xij, xpinv, res.lag[0, w])
        for c in range(2):
            err = abs(Fraction(float(res.z[0, w, c])) - t['z'][c])
            assert err <= t['z_bound'][c], 'SOLVE finding (%s): z[%d] of %s off by %g, bound %g' % (
                tag, c, name, float(err), float(t['z_bound'][c]))
        acc, e_acc, e_sig = st.ols_acc(xij, t['tau'], res.z[0, w])
        sig = float(res.sigma_tau[0, w])
        if np.isnan(sig):
            assert acc <= e_acc, 'SOLVE finding (%s): sigma_tau NaN at %s although acc* = %g > %g' % (
                tag, name, float(acc), float(e_acc))
        else:
            err = abs(Fraction(sig) ** 2 * (P - 2) - acc)
            assert err <= e_sig, 'SOLVE finding (%s): sigma_tau^2 (P - 2) of %s off by %g, bound %g' % (
                tag, name, float(err), float(e_sig))
    for name in ('exact z(0,0)', 'all_same'):                 # z = (0, 0): the point branch of the uncertainty kernel
        w = names.index(name)
        assert not res.z[0, w].any() and res.sigma_tau[0, w] == 0.0 and res.vel[0, w] == np.inf, name
        assert res.vel_uncert[0, w] == 0.0 and res.baz_uncert[0, w] == 0.0, name


def test_several_estimators_in_one_pass():
    """The 8-element tables through ``engine.process_multi`` at ALPHA = 0.5, 0.9, 1.0 and for a 6-element subset: every
    estimator equals its own single call bit for bit (MdCCM of the subset within 1e-12, as tests/test_gpu_multi.py)."""
    N = 8
    tabs = st.tables(N)
    x = st.pulse_trace(tabs)
    rij = st.grid_geometry(N)
    n = len(tabs)
    ests = engine.normalize_estimators([0.5, 0.9, 1.0, (0.5, (2, 5))], N)
    kept = [engine.kept_elements(N, rm) for _, rm in ests]
    rijs = [np.ascontiguousarray(rij[:, k]) for k in kept]
    kw = dict(prefiltered=True, want_lag=True, want_cmax=True, want_uncert=True, vector_len=n + PAD)
    multi = engine.process_multi(list(x), st.FS, [T0] * len(ests), rijs, [(None, None)], [st.W / st.FS], 0.0, ests, **kw)
    lag, _ = st.designed_lags(tabs)
    np.testing.assert_array_equal(multi[0].lag[0, :n], lag, err_msg='CORRELATOR finding: the fetched lags are not the designed table')
    dropped = 0
    for res, (alpha, remove), k, r in zip(multi, ests, kept, rijs):
        one = engine.process(np.ascontiguousarray(x[k]), st.FS, T0, r, [(None, None)], [st.W / st.FS], 0.0, alpha, **kw)
        tag = 'alpha=%g remove=%s' % (alpha, remove)
        assert int(res.nwin[0]) == int(one.nwin[0]) == n
        np.testing.assert_array_equal(res.lag, one.lag, err_msg='CORRELATOR finding: lags, ' + tag)
        np.testing.assert_array_equal(res.lag, multi[0].lag[..., engine.kept_pair_map(N, remove)], err_msg=tag)
        for name in ('vel', 'baz', 'sigma_tau', 't', 'mask', 'vel_uncert', 'baz_uncert'):
            np.testing.assert_array_equal(getattr(res, name), getattr(one, name), err_msg='%s, %s' % (name, tag))
        if remove:
            np.testing.assert_allclose(res.mdccm, one.mdccm, rtol=0, atol=1e-12, err_msg=tag)
        else:
            np.testing.assert_array_equal(res.mdccm, one.mdccm, err_msg=tag)
        if alpha < 1.0:
            dropped += int(np.sum(res.weights[0, :n] == 0))
    assert dropped > 0


@pytest.mark.parametrize('N', [6, 23])
def test_packed_mask_equals_the_weight_bytes(N):
    """pack_weights_kernel at 15 and 253 pairs (neither a multiple of 8): bit k & 7 of byte k >> 3 of ``nbls_fetch_packed``
    is the weight byte of pair k from ``nbls_fetch``; the bits behind the last pair are zero."""
    tabs = st.tables(N)
    res, n, xij, _ = _process(N, 0.5, tabs)
    P = len(xij)
    assert P % 8 != 0
    h = res.handle
    wts = h.fetch(grids=False, want_weights=True)['weights']
    mask = h.fetch_packed()['mask']
    assert wts.shape == (1, n + PAD, P) and mask.shape == (1, n + PAD, (P + 7) // 8)
    assert set(np.unique(wts[0, :n])) == {0, 1}
    bits = np.unpackbits(mask, axis=-1, bitorder='little')
    np.testing.assert_array_equal(bits[0, :n, :P], wts[0, :n])
    assert not bits[0, :, P:].any() and not mask[0, n:].any()
    np.testing.assert_array_equal(mask, res.mask)
