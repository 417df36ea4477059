"""Host-side checks of the batch entry points: input validation happens before any GPU work."""
import numpy as np
import pytest

import narrow_band_least_squares_amd as nbls
from narrow_band_least_squares_amd import engine, synthetic


def _streams(N=5, npts=2000, fs=20.0, S=3):
    rij = synthetic.array_geometry(N, 1.0)
    return [synthetic.make_stream(synthetic.plane_wave(rij, npts, fs, 0.5, 4.0, seed=i), fs) for i in range(S)], rij


def _nbls_args(sts, rij):
    fr = np.logspace(-2, 1, 8)
    return ([30.0, 30.0], 0.5, 1.0, sts, None, None, 2, np.zeros(8), np.zeros(8), np.array([0.5, 1.0, 2.0]), 'log', fr,
            'butter', 2, 0.01)


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('a device was opened')
    monkeypatch.setattr(engine, 'get_handle', refuse)
    monkeypatch.setattr(engine, 'Handle', refuse)


@pytest.mark.parametrize('what', ['npts', 'fs', 'elements'])
def test_mismatched_recordings_raise_before_any_gpu_work(what, no_device):
    sts, rij = _streams()
    if what == 'npts':
        odd, _ = _streams(npts=1999, S=1)
        match = 'samples'
    elif what == 'fs':
        odd, _ = _streams(fs=40.0, S=1)
        match = 'sampled'
    else:
        odd, _ = _streams(N=6, S=1)
        match = 'elements'
    sts = sts[:1] + odd + sts[1:]
    rij = rij - rij.mean(axis=1, keepdims=True)
    with pytest.raises(ValueError, match=match):
        nbls.narrow_band_least_squares_batch(*_nbls_args(sts, rij), rij=rij)
    with pytest.raises(ValueError, match=match):
        nbls.ltsva_batch(sts, None, None, 30.0, 0.5, rij=rij)


def test_empty_batch_returns_an_empty_list(no_device):
    assert nbls.narrow_band_least_squares_batch(*_nbls_args([], None)) == []
    assert nbls.ltsva_batch([], None, None, 30.0, 0.5) == []
    assert nbls.ltsva_batch(iter(()), None, None, 30.0, 0.5) == []


def test_batch_functions_are_exported_but_not_installed_as_reference_modules():
    assert 'narrow_band_least_squares_batch' in nbls.__all__ and 'ltsva_batch' in nbls.__all__
    from narrow_band_least_squares_amd import _hip
    assert 'nbls_set_segments' in _hip.EXPORTS
    import inspect
    src = inspect.getsource(nbls.install_as_reference_modules)
    assert 'batch' not in src


def test_batch_rows_keeps_the_streams_own_buffers():
    sts, _ = _streams(S=2)
    rows, fs, t0s = engine.batch_rows(sts)
    assert fs == 20.0 and len(t0s) == 2 and len(rows) == 2
    for st, rec in zip(sts, rows):
        for tr, r in zip(st, rec):
            assert r is tr.data or np.shares_memory(r, tr.data)
