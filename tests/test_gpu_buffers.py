"""One handle through the transitions that move, grow, keep or drop its buffers (csrc/dev_buf.h; ``ensure`` / ``alloc_copy``
in csrc/api.hip): after every step its results are those of the same call on a FRESH handle, bit for bit — grids, lags,
cmax, the weight mask, and every further estimator's block.  Whether anything leaks is the stand-alone program's business
(tests/c_caller/dev_buf_test.cpp, CPU suite): the device's free memory is shared and says nothing here."""
import numpy as np
import pytest

from narrow_band_least_squares_amd import _hip, engine, planner, synthetic

pytestmark = pytest.mark.gpu

FS = 20.0
EDGES = [(0.5, 1.0), (1.0, 2.0)]
WINLENS = [30.0, 20.0]


@pytest.fixture(scope='module')
def recording():
    """cfg-2 cut to 5 elements and 6000 samples: the smallest input with LTS tables, the arena and screening buffers."""
    c = synthetic.build_config('cfg2', 1.0 / 12.0)
    data = np.ascontiguousarray(c['data'][:5])
    assert data.shape == (5, 6000)
    rij = c['rij'][:, :5]
    return data, rij - rij.mean(axis=1, keepdims=True)


def _sub_array(rij, kept, alpha):
    """A further estimator on the elements ``kept`` (``Handle.set_estimators``)."""
    r = np.ascontiguousarray(rij[:, kept])
    xij, pair_idx, xpinv = planner.co_array(r - r.mean(axis=1, keepdims=True))
    return dict(kept=list(kept), xij=xij, pair_idx=pair_idx, xpinv=xpinv,
                lts=planner.lts_plan(xij, alpha) if alpha < 1.0 else None, eig6=None)


def _run(h, data, rij, bands, alpha, extras=(), taper_npts=None, stream=False, options=()):
    """Upload, plan and run bands ``bands`` of the two on ``h`` -> per estimator, everything a caller can fetch."""
    nchans, npts = data.shape
    prep = engine.prepare(nchans, npts, FS, rij, [EDGES[b] for b in bands], [WINLENS[b] for b in bands], 0.5, alpha,
                          'butter', 2, 0.01)
    if taper_npts is not None:                       # the ramps of another trace length: another taper length
        prep.tl, prep.tr = planner.taper_ramps(taper_npts)
    for key in options:
        h.set_option(key, 1)
    engine.launch(h, data, prep, estimators=list(extras), stream=stream)
    h.sync()
    out = []
    for est in range(1 + len(extras)):
        r = h.fetch(want_lag=True, want_cmax=True, est=est)
        packed = h.fetch_packed(est=est)
        r['mask'] = packed['mask']
        for k in ('vel', 'baz', 'mdccm', 'sigma_tau'):
            assert r[k].tobytes() == packed[k].tobytes()
        if stream:                                   # the pinned mirror holds the same cells, batch by batch
            flat = np.stack([packed[k].reshape(-1) for k in ('vel', 'baz', 'mdccm', 'sigma_tau')])
            for k in range(h.result_batches()):
                _, _, c0, c1, grids, mask = h.wait_result_batch(k, est=est)
                assert grids[:, c0:c1].tobytes() == flat[:, c0:c1].tobytes()
                assert mask[c0:c1].tobytes() == packed['mask'].reshape(mask.shape)[c0:c1].tobytes()
        out.append(r)
    return out


def _same(got, exp, what):
    assert len(got) == len(exp), what
    for e, (g, x) in enumerate(zip(got, exp)):
        assert g['vel'].any() and g['lag'].any(), (what, e)          # the pass computed something
        for k in ('vel', 'baz', 'mdccm', 'sigma_tau', 'nwin', 'lag', 'cmax', 'mask'):
            assert g[k].dtype == x[k].dtype and g[k].shape == x[k].shape, (what, e, k)
            assert g[k].tobytes() == x[k].tobytes(), '%s: estimator %d: %s differs from a fresh handle' % (what, e, k)


def test_one_handle_through_every_buffer_transition(recording):
    data, rij = recording
    data4, rij4 = np.ascontiguousarray(data[:4]), rij[:, :4] - rij[:, :4].mean(axis=1, keepdims=True)
    extras = [_sub_array(rij, (0, 1, 2, 3, 4), 1.0), _sub_array(rij, (0, 1, 3, 4), 0.5)]    # the second has compact rows of its own
    block = np.arange(1 << 20, dtype=np.uint8)       # larger than any result block of these plans

    first = dict(data=data, rij=rij, bands=(0, 1), alpha=0.5)
    steps = [                                        # (what, arguments of _run, done to the one handle alone before it)
        ('an LTS plan', first, None),
        ('a smaller plan (one band, OLS): every buffer kept', dict(first, bands=(1,), alpha=1.0), None),
        ('the first plan again, streamed', dict(first, stream=True), None),
        ('two further estimators, one a 4-element sub-array', dict(first, extras=extras, stream=True), None),
        ('no further estimators again', first, None),
        ('a longer taper', dict(first, taper_npts=4 * data.shape[1]), None),
        ('a 4-element trace and geometry', dict(first, data=data4, rij=rij4), None),
        ('a loaded result block, then the 5-element plan', first, lambda h: h.load_result_block(block)),
    ]
    if _hip.load_library().nbls_developer_build() == 1:
        steps.append(('the developer build\'s stamp buffer', dict(first, options=('screen_stamps',)), None))

    fresh = {}                                       # results on a fresh handle, once per distinct call

    def reference(kw):
        key = tuple((k, v if k not in ('data', 'rij', 'extras') else len(v)) for k, v in sorted(kw.items()))
        if key not in fresh:
            f = _hip.Handle()
            try:
                fresh[key] = _run(f, **kw)
            finally:
                f.close()
        return fresh[key]

    h = _hip.Handle()
    try:
        for what, kw, only_here in steps:
            if only_here is not None:
                only_here(h)
            _same(_run(h, **kw), reference(kw), what)
    finally:
        h.close()                                    # explicit: the buffers go with the handle, arena places skipped
    assert h._h is None
