"""Every opt-in request that combines, in ONE call (tests/requests_cases.py), through the three forms of a pass: ``process``
in one pass, ``process`` in HBM rounds of one band, and ``process_batch`` of the same recording twice.  The three read one
table of result groups (``call_requests.RESULT_GROUPS``) in three ways — one result, one result in rounds, rows interleaved
over two — so a row of the table that is wrong in one form only shows here as a field whose bytes differ."""
import numpy as np
import pytest

import requests_cases as rc
import scale_cases as sc
from narrow_band_least_squares_amd import engine

pytestmark = pytest.mark.gpu

NOT_COMPARED = sc.CONFIG + ('weights', 'lag', 'cmax', 'z', 'lag_frac')        # the call's own, and what a batch does not fetch


def _same(got, exp, label):
    names, _ = sc.batch_fields()
    compared = 0
    for k in [k for k in names if k not in NOT_COMPARED]:
        a, b = getattr(got, k, None), getattr(exp, k, None)
        assert a is not None and b is not None, (label, k)
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (label, k, a.shape, b.shape, a.dtype, b.dtype)
        if a.tobytes() != b.tobytes():
            np.testing.assert_array_equal(a, b, err_msg='%s %s' % (label, k))         # (says where)
            raise AssertionError('%s %s: equal values in different bits' % (label, k))
        compared += 1
    return compared


def test_every_request_in_the_three_forms_of_a_pass(monkeypatch):
    data, rij = rc.recording()

    def single():
        return engine.process(data, rc.FS, rc.T0, rij, rc.EDGES, rc.WINLENS, rc.OVERLAP, rc.ALPHA, *rc.FILTER, **rc.ALL_ON)

    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    whole = single()
    assert [int(w) for w in whole.W] == list(rc.WINDOWS) and whole.families_in_pass
    for k in ('beam_trace', 'music_vectors', 'clean_residual', 'element_shift', 'capon_peak_offset', 'grid_map', 'family_table'):
        assert np.any(getattr(whole, k)), k
    assert any(np.any(np.asarray(whole.weights)[b, :int(whole.nwin[b])] == 0) for b in range(2))         # LTS dropped pairs
    batch = engine.process_batch([list(data), list(data)], rc.FS, [rc.T0, rc.T0], rij, rc.EDGES, rc.WINLENS, rc.OVERLAP, rc.ALPHA,
                                 *rc.FILTER, **rc.ALL_ON)
    for s, res in enumerate(batch):
        n = _same(res, whole, 'recording %d of the batch against the single call:' % s)
    # two HBM rounds of one band each: N rows of the filtered band and one of its beam trace
    monkeypatch.setenv('NBLS_MAX_FILTERED_GB', repr(1.5 * 8.0 * (rc.N + 1) * (rc.NPTS + 64) / 2.0 ** 30))
    assert engine.max_bands_per_pass(rc.N, rc.NPTS, 1) == 1
    rounds = single()
    assert not rounds.families_in_pass
    assert _same(rounds, whole, 'rounds of one band against one pass:') == n
    print('%d fields compared in each form' % n)
