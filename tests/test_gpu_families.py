"""The family labelling on the GPU (``nbls_set_families`` / ``nbls_label_families``, csrc/families.hip)
against tests/families_truth.py: exact equality of ``family``, ``nfamilies`` and every table column, no tolerance anywhere.
The designed lattices of tests/families_cases.py go through ``nbls_label_families``; a pass's own labelling is compared with
the truth on the rows the pass returned and with ``nbls_label_families`` on the same rows, in every form of a pass."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import families_cases as fc
import families_demo as demo
import families_truth as ft
from narrow_band_least_squares_amd import (engine, planner, synthetic, _hip, label_families, ltsva, ltsva_families, ltsva_families_batch,
                                           narrow_band_least_squares, narrow_band_least_squares_families,
                                           narrow_band_least_squares_families_batch)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = fc.all_cases()
PLAIN = ('vel', 'baz', 'mdccm', 'sigma_tau', 'mask')
_truth = {}


def truth(c):
    if c['name'] not in _truth:
        _truth[c['name']] = ft.label(*fc.args_of(c))
    return _truth[c['name']]


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _label(c, capacity=None, h=None):
    h = h or engine.get_handle()
    return h.label_families(_hip.family_params(**c['par']), c['nseg'], c['winlen'], c['wininc'], c['nwin'], c['vel'], c['baz'], c['mdccm'],
                            c['sigma_tau'], capacity=capacity)


def _same(got, want, what=''):
    fam, n, tab = got
    efam, en, etab = want
    assert n == en, (what, n, en)
    assert fam.dtype == np.int32 and tab.dtype == np.int64
    assert np.array_equal(fam, efam), (what, np.flatnonzero((fam != efam).reshape(-1))[:8])
    assert tab.shape == etab.shape and np.array_equal(tab, etab), (what, np.flatnonzero((tab != etab).any(axis=1))[:8])


# ---- nbls_label_families on the designed lattices ----

@pytest.mark.parametrize('c', CASES, ids=lambda c: c['name'])
def test_designed_lattice(c):
    _same(_label(c), truth(c), c['name'])


def test_capacity_below_the_family_count():
    c = next(c for c in CASES if c['name'] == 'random_6')
    efam, en, etab = truth(c)
    assert en > 5
    for cap in (0, 1, 5, en, en + 3):
        fam, n, tab = _label(c, capacity=cap)
        assert n == en and np.array_equal(fam, efam) and np.array_equal(tab, etab[:cap])
    h = engine.get_handle()                                  # every pointer may be NULL
    p = _hip.family_params(**c['par'])
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    n = C.c_int32(-1)
    rc = h.lib.nbls_label_families(h._h, C.byref(p), len(c['winlen']), 1, c['vel'].shape[1], c['winlen'].ctypes.data_as(ip),
                                   c['wininc'].ctypes.data_as(ip), c['nwin'].ctypes.data_as(ip), c['vel'].ctypes.data_as(dp),
                                   c['baz'].ctypes.data_as(dp), c['mdccm'].ctypes.data_as(dp), c['sigma_tau'].ctypes.data_as(dp), None,
                                   C.byref(n), None, 0)
    assert rc == 0 and n.value == en


def test_a_second_call_on_the_same_handle_gives_the_same_bits():
    h = engine.get_handle()
    big, small = (next(c for c in CASES if c['name'] == k) for k in ('cells_65537', 'mix_b2_t3'))
    first = _label(big, h=h)
    _same(_label(small, h=h), truth(small))                  # (smaller lattice in the same buffers)
    again = _label(big, h=h)
    assert again[1] == first[1] and _bits(again[0], first[0]) and _bits(again[2], first[2])
    _same(again, truth(big))


def test_label_families_refuses_bad_lattices_and_requests():
    h = engine.get_handle()
    c = next(c for c in CASES if c['name'] == 'min_pixels')
    ip, dp = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    one = np.ones(4, dtype=np.int32)
    z = np.zeros(16)

    def call(par=None, nbands=1, nseg=1, vl=4, winlen=one, wininc=one, nwin=one, sig=None):
        p = _hip.family_params(**dict(c['par'], **(par or {})))
        n = C.c_int32(0)
        return h.lib.nbls_label_families(h._h, C.byref(p), nbands, nseg, vl, winlen.ctypes.data_as(ip), wininc.ctypes.data_as(ip),
                                         nwin.ctypes.data_as(ip), z.ctypes.data_as(dp), z.ctypes.data_as(dp), z.ctypes.data_as(dp),
                                         None if sig is None else sig.ctypes.data_as(dp), None, C.byref(n), None, 0)
    assert call() == 0
    assert call(nbands=2, vl=2 ** 30) == _hip.NBLS_ERR_ARG            # 2^31 cells (refused before anything is read)
    assert call(nbands=2 ** 15, nseg=2 ** 15, vl=2) == _hip.NBLS_ERR_ARG
    assert call(winlen=one * 0) == _hip.NBLS_ERR_ARG and call(wininc=-one) == _hip.NBLS_ERR_ARG
    assert call(nwin=one * 5) == _hip.NBLS_ERR_ARG and call(nwin=-one) == _hip.NBLS_ERR_ARG
    assert call(nwin=one * 4) == 0
    assert call(sig=z) == _hip.NBLS_ERR_ARG and call(par=dict(sigma_tau_max=1.0)) == _hip.NBLS_ERR_ARG
    assert call(par=dict(sigma_tau_max=1.0), sig=z) == 0
    for bad in (dict(mdccm_min=np.nan), dict(mdccm_min=np.inf), dict(vel_min=0.7), dict(vel_max=np.inf), dict(vel_min=np.nan),
                dict(sigma_tau_max=np.inf), dict(baz_tol=-1.0), dict(baz_tol=180.5), dict(baz_tol=np.nan), dict(vel_tol=-0.1),
                dict(vel_tol=np.nan), dict(band_reach=-1), dict(band_reach=9), dict(time_reach=0), dict(time_reach=9), dict(min_pixels=0)):
        assert call(par=bad, sig=z if 'sigma_tau_max' in bad else None) == _hip.NBLS_ERR_ARG, bad
        p = _hip.family_params(**dict(c['par'], **bad))
        assert h.lib.nbls_set_families(h._h, C.byref(p)) == _hip.NBLS_ERR_ARG, bad
    p = _hip.family_params(**c['par'])
    p.flags = 1
    assert h.lib.nbls_set_families(h._h, C.byref(p)) == _hip.NBLS_ERR_ARG
    assert call(par=dict(band_reach=8, time_reach=8, baz_tol=180.0, vel_tol=0.0)) == 0


def test_the_public_label_families():
    c = next(c for c in CASES if c['name'] == 'segments')
    fam, tab = label_families(c['vel'], c['baz'], c['mdccm'], None, c['nwin'], c['winlen'], c['wininc'], nseg=3, **c['par'])
    _same((fam, len(tab), tab), truth(c))
    c = next(c for c in CASES if c['name'] == 'random_9')
    fam, tab = label_families(c['vel'], c['baz'], c['mdccm'], c['sigma_tau'], c['nwin'], c['winlen'], c['wininc'], **c['par'])
    _same((fam, len(tab), tab), truth(c))


# ---- in a pass ----

FILTER = ('butter', 2, 0.01)


def _pass(data, t0=demo.T0, alpha=1.0, par=demo.PAR4, **kw):
    return engine.process(data, demo.FS, t0, demo.RIJ, demo.EDGES4, demo.WINLEN4, 0.5, alpha, *FILTER, families=par, **kw)


def _three_ways(res, par=demo.PAR4, what=''):
    """The pass's labelling, the truth on the rows the pass returned, and nbls_label_families on the same rows."""
    assert res.family.shape == res.vel.shape and res.family.dtype == np.int32
    gate = par['sigma_tau_max'] is not None
    want = ft.label(par, 1, res.W, res.inc, res.nwin, res.vel, res.baz, res.mdccm, res.sigma_tau if gate else None)
    _same((res.family, len(res.family_table), res.family_table), want, what + ' pass / truth')
    again = res.handle.label_families(_hip.family_params(**par), 1, res.W, res.inc, res.nwin, res.vel, res.baz, res.mdccm,
                                      res.sigma_tau if gate else None)
    _same(again, want, what + ' label / truth')
    return want


@pytest.fixture(scope='module')
def one_pass():
    res = _pass(demo.traces4(0))
    assert res.families_in_pass
    return res


def test_in_pass_three_ways(one_pass):
    fam, n, tab = _three_ways(one_pass)
    assert n >= 2                                            # the two sources (the oracle's rows give 22 and 31 cells)
    assert tab[:, 0].min() >= demo.PAR4['min_pixels']
    ungated = _pass(demo.traces4(0), par=dict(demo.PAR4, sigma_tau_max=None, min_pixels=1))
    fam1, n1, _ = _three_ways(ungated, dict(demo.PAR4, sigma_tau_max=None, min_pixels=1), 'ungated')
    assert n1 > n and not (fam1 == -2).any()
    lts = _pass(demo.traces4(1), alpha=0.5, par=dict(demo.PAR4, sigma_tau_max=None))
    assert _three_ways(lts, dict(demo.PAR4, sigma_tau_max=None), 'lts')[1] >= 2


def test_the_plain_results_of_the_plan_are_unchanged(one_pass):
    off = engine.process(demo.traces4(0), demo.FS, demo.T0, demo.RIJ, demo.EDGES4, demo.WINLEN4, 0.5, 1.0, *FILTER)
    assert getattr(off, 'family', None) is None
    for k in PLAIN:
        assert _bits(getattr(off, k), getattr(one_pass, k)), k
    with pytest.raises(_hip.NblsError) as err:                # fetching without the request
        off.handle.fetch_families()
    assert err.value.code == _hip.NBLS_ERR_STATE


def test_batch_of_three_recordings_equals_three_single_calls():
    recs = [demo.traces4(i) for i in range(3)]
    t0s = [demo.T0 + 0.0173 * i for i in range(3)]
    batch = engine.process_batch([list(d) for d in recs], demo.FS, t0s, demo.RIJ, demo.EDGES4, demo.WINLEN4, 0.5, 1.0, *FILTER,
                                 families=demo.PAR4)
    assert len(batch) == 3
    for s in range(3):
        single = _pass(recs[s], t0s[s])
        assert len(single.family_table) >= 2
        assert _bits(batch[s].family, single.family) and _bits(batch[s].family_table, single.family_table), s
        for k in PLAIN:
            assert _bits(getattr(batch[s], k), getattr(single, k)), (s, k)
    assert not _bits(batch[0].family, batch[1].family)


def test_streamed_and_overlapped_passes_equal_the_unstreamed_pass(monkeypatch, one_pass):
    h = engine.get_handle()
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '1')
    try:
        h.set_option('screen_batch_mb', 1)
        h.set_option('solve_min_units', 1)
        h.set_option('overlap', 1)
        overlapped = _pass(demo.traces4(0))
        nbatches = h.result_batches()
        h.set_option('overlap', -1)
        serial = _pass(demo.traces4(0))
    finally:
        h.set_option('overlap', 0)
        h.set_option('screen_batch_mb', 192)
        h.set_option('solve_min_units', 0)
    print('result batches of the streamed pass:', nbatches)
    for name, got in (('overlap on', overlapped), ('overlap off', serial)):
        assert got.families_in_pass
        assert _bits(got.family, one_pass.family) and _bits(got.family_table, one_pass.family_table), name
        for k in PLAIN:
            assert _bits(getattr(got, k), getattr(one_pass, k)), (name, k)


def test_two_band_rounds_equal_the_one_pass_call(monkeypatch, one_pass):
    # room for two of the four bands: 8 filtered rows per band
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', repr(2.5 * 8.0 * 8 * (demo.NPTS4 + 64) / 2.0 ** 30))
    assert engine.max_bands_per_pass(8, demo.NPTS4) == 2
    rounds = _pass(demo.traces4(0))
    assert not rounds.families_in_pass
    assert _bits(rounds.family, one_pass.family) and _bits(rounds.family_table, one_pass.family_table)
    for k in PLAIN:
        assert _bits(getattr(rounds, k), getattr(one_pass, k)), k


def test_plan_refusals_and_the_fetch_before_a_pass():
    h = _pass(demo.traces4(0)).handle                                # (its trace and geometry stay on the handle)
    rij = demo.RIJ
    plan = lambda: h.plan(None, False, None, None, [65], [32], 200)
    par = _hip.family_params(**demo.PAR4)
    try:
        h.set_families(par)
        h.set_window_ranges(np.array([1]), np.array([5]))
        with pytest.raises(ValueError, match='nbls_set_families') as err:
            plan()
        assert err.value.code == _hip.NBLS_ERR_UNSUPPORTED and 'nbls_set_window_ranges' in str(err.value)
        h.set_window_ranges(None)
        sub = [0, 1, 2, 3]
        xs, ps, xp = planner.co_array(rij[:, sub])
        h.set_estimators([dict(kept=sub, xij=xs, pair_idx=ps, xpinv=xp, lts=None, eig6=None)])
        with pytest.raises(ValueError, match='nbls_set_families') as err:
            plan()
        assert err.value.code == _hip.NBLS_ERR_UNSUPPORTED and 'nbls_set_estimators' in str(err.value)
        h.set_estimators(())
        plan()                                                       # accepted
        fam, n, tab = h.fetch_families()                             # nothing labelled until a pass has run the solve stage
        assert n == 0 and (fam == -1).all() and tab.shape == (0, 8)
        h.execute(stages=3)
        assert h.fetch_families()[1] == 0
        h.execute()
        r = h.fetch()
        got = h.fetch_families()
        _same(got, ft.label(demo.PAR4, 1, [65], [32], r['nwin'], r['vel'], r['baz'], r['mdccm'], r['sigma_tau']), 'raw plan')
        h.execute(stages=3)                                          # a pass without the solve stage leaves it as it is
        assert _bits(h.fetch_families()[0], got[0])
        fam, n, tab = h.fetch_families(capacity=0)
        assert n == got[1] and tab.shape == (0, 8)
    finally:
        h.set_window_ranges(None)
        h.set_estimators(())
        h.set_families(None)
    plan()
    with pytest.raises(_hip.NblsError) as err:                        # switched off again
        h.fetch_families()
    assert err.value.code == _hip.NBLS_ERR_STATE


def test_rccl_communicator_refuses_the_request_at_plan_time():
    """A communicator lives as long as its process: a child process over the tests' loopback transport."""
    src = os.path.join(ROOT, 'tests', 'c_caller', 'loopback_rccl.cpp')
    lib = os.path.join(ROOT, 'tests', 'c_caller', 'libloopback_rccl.so')
    if not os.path.exists(lib) or os.path.getmtime(lib) < os.path.getmtime(src):
        subprocess.run(['/opt/rocm/bin/hipcc', '-O2', '-shared', '-fPIC', '--offload-arch=gfx950', src, '-o', lib], check=True,
                       timeout=300)
    env = dict(os.environ, NBLS_TEST_TRANSPORT=lib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', '_families_comm_worker.py')], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and 'FAMILIES_COMM_OK' in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


# ---- the public calls and the demonstration ----

def test_demonstration_and_the_narrow_band_calls():
    streams = {k: synthetic.make_stream(demo.traces(src, seed), demo.FS, starttime=demo.T0) for k, (src, seed) in demo.RECORDINGS.items()}
    out = narrow_band_least_squares_families(*demo.call_args(streams['signal']), rij=demo.RIJ, **demo.PAR)
    ref = narrow_band_least_squares(*demo.call_args(streams['signal']), rij=demo.RIJ)
    assert len(out) == 11 and len(ref) == 9
    for i in (0, 1, 2, 3, 5, 6):
        np.testing.assert_array_equal(out[i], ref[i])
    vel, baz, mdccm, sig, nwin, family, fams = out[0], out[1], out[2], out[5], out[6], out[9], out[10]
    table = np.stack([fams[k] for k in planner.FAMILY_FIELDS], axis=1)
    _same((family, len(table), table), ft.label(demo.PAR, 1, demo.W, demo.INC, nwin, vel, baz, mdccm), 'demonstration')
    demo.check_signal(family, table, vel, baz, mdccm, sig)
    print('demonstration on the GPU rows: counts', table[:, 0], 'baz', fams['baz_mean'], 't', fams['t_start'], fams['t_end'])
    quiet = narrow_band_least_squares_families(*demo.call_args(streams['noise']), rij=demo.RIJ, **demo.PAR)
    assert len(quiet[10]['count']) == 0 and (quiet[9] < 0).all()
    assert ft.label(demo.PAR, 1, demo.W, demo.INC, quiet[6], quiet[0], quiet[1], quiet[2])[1] == 0
    args = demo.call_args(None)
    batch = narrow_band_least_squares_families_batch(*args[:3], [streams['signal'], streams['noise'], streams['signal']], *args[4:],
                                                     rij=demo.RIJ, **demo.PAR)
    assert len(batch) == 3 and all(len(b) == 11 for b in batch)
    for b, single in zip(batch, (out, quiet, out)):
        assert _bits(b[9], single[9])
        for k in single[10]:
            np.testing.assert_array_equal(b[10][k], single[10][k])


def test_the_ltsva_calls():
    W = 20.0
    st = [synthetic.make_stream(engine_filtered, demo.FS, starttime=demo.T0) for engine_filtered in _filtered_band()]
    par = dict(demo.PAR, min_pixels=3)
    got = ltsva_families(st[0], None, None, W, 0.5, rij=demo.RIJ, **par)
    plain = ltsva(st[0], None, None, W, 0.5, rij=demo.RIJ)
    assert len(got) == 10 and len(plain) == 8
    for i in (0, 1, 2, 3, 5, 6, 7):
        np.testing.assert_array_equal(got[i], plain[i])
    n = len(got[0])
    Ws, inc = int(W * demo.FS), int(W * demo.FS) // 2
    fam, nf, tab = ft.label(par, 1, [Ws], [inc], [n], got[0][None], got[1][None], got[3][None])
    assert nf >= 1 and np.array_equal(got[8], fam[0]) and np.array_equal(got[9]['count'], tab[:, 0])
    assert np.array_equal(got[9]['sample_end'], tab[:, 7]) and np.isnan(got[9]['f_lo']).all()
    batch = ltsva_families_batch(st, None, None, W, 0.5, rij=demo.RIJ, **par)
    assert len(batch) == 2 and _bits(batch[0][8], got[8])
    other = ltsva_families(st[1], None, None, W, 0.5, rij=demo.RIJ, **par)
    assert _bits(batch[1][8], other[8])
    for k in other[9]:
        np.testing.assert_array_equal(batch[1][9][k], other[9][k])


def _filtered_band():
    """Two recordings of one transient wave in a band the caller has filtered already (white noise around it)."""
    T = demo.NPTS4 / demo.FS
    return [synthetic.transient_waves(demo.RIJ, demo.NPTS4, demo.FS, [(50.0 + 90.0 * i, 0.34, 1.0, 0.2 * T, 0.6 * T, 0.5, 3.0)], snr_db=6.0,
                                      seed=31 + i) for i in range(2)]
