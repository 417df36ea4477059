"""Host side of the multi-estimator calls (``narrow_band_least_squares_multi``, ``ltsva_multi``): argument checks that
raise before any device is opened, the normal form of an estimator list and the map from a reduced array's pairs to the
full array's.  No GPU."""
import inspect

import numpy as np
import pytest

import narrow_band_least_squares_amd as nbls
from narrow_band_least_squares_amd import _hip, engine, planner, synthetic


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError('a device was opened')
    monkeypatch.setattr(engine, 'get_handle', refuse)
    monkeypatch.setattr(engine, 'Handle', refuse)


def _stream(N=8, npts=2000, fs=20.0):
    rij = synthetic.array_geometry(N, 1.0)
    data = synthetic.plane_wave(rij, npts, fs, 0.5, 4.0, seed=11)
    return synthetic.make_stream(data, fs), rij


def _nbls_args(ests, st, rij):
    freqlist = np.array([0.5, 1.0, 2.0])
    fr = np.logspace(-2, 1, 8)
    return ([30.0, 30.0], 0.5, ests, st, None, None, 2, np.zeros(8), np.zeros(8), freqlist, 'log', fr, 'butter', 2, 0.01), dict(rij=rij)


BAD = [
    ([], 'empty'),
    ([0.4], 'ALPHA'),
    ([1.5], 'ALPHA'),
    ([(0.75, (8,))], 'out of range'),
    ([(0.75, (-1,))], 'out of range'),
    ([(1.0, (3, 3))], 'ascend'),
    ([(1.0, (5, 2))], 'ascend'),
    ([(1.0, (0, 1, 2, 3, 4, 5))], 'at least 3'),              # 2 kept
    ([(0.5, (0, 1, 2, 3, 4))], 'at least 4'),                 # 3 kept under LTS
    ([1.0] * 9, 'at most 8'),
]


@pytest.mark.parametrize('ests,match', BAD)
def test_bad_estimators_raise_before_any_gpu_work(ests, match, no_device):
    st, rij = _stream()
    a, kw = _nbls_args(ests, st, rij)
    with pytest.raises(ValueError, match=match):
        nbls.narrow_band_least_squares_multi(*a, **kw)
    with pytest.raises(ValueError, match=match):
        nbls.ltsva_multi(st, None, None, 30.0, 0.5, ests, rij=rij)


def test_three_elements_are_enough_for_ols_only():
    assert engine.normalize_estimators([(1.0, (0, 1, 2, 3, 4))], 8) == [(1.0, (0, 1, 2, 3, 4))]
    with pytest.raises(ValueError):
        engine.normalize_estimators([(0.99, (0, 1, 2, 3, 4))], 8)


def test_a_bare_float_means_nothing_removed():
    got = engine.normalize_estimators([1.0, 0.75, (0.5, [7]), (1, (0, 3))], 8)
    assert got == [(1.0, ()), (0.75, ()), (0.5, (7,)), (1.0, (0, 3))]
    assert all(isinstance(a, float) and isinstance(r, tuple) for a, r in got)


def test_reduced_pair_map_against_a_direct_construction():
    N, remove = 8, (2, 7)
    full = [(i, j) for i in range(N - 1) for j in range(i + 1, N)]
    direct = [k for k, (i, j) in enumerate(full) if i not in remove and j not in remove]
    got = engine.kept_pair_map(N, remove)
    assert got.dtype == np.int32 and got.tolist() == direct
    # ... and they are the reduced array's own pair list, in its order
    kept = engine.kept_elements(N, remove)
    assert kept == [0, 1, 3, 4, 5, 6]
    reduced = planner.pair_table(len(kept))
    assert [(kept[i], kept[j]) for i, j in reduced] == [full[k] for k in got]
    assert engine.kept_pair_map(N, ()).tolist() == list(range(len(full)))


def test_multi_functions_are_exported_but_not_installed_as_reference_modules():
    assert 'narrow_band_least_squares_multi' in nbls.__all__ and 'ltsva_multi' in nbls.__all__
    for name in ('nbls_set_estimators', 'nbls_est_result_layout', 'nbls_est_fetch_packed', 'nbls_est_fetch',
                 'nbls_est_fetch_uncertainty', 'nbls_est_wait_result_batch'):
        assert name in _hip.EXPORTS
    assert 'multi' not in inspect.getsource(nbls.install_as_reference_modules)
    sig = list(inspect.signature(nbls.narrow_band_least_squares_multi).parameters)
    ref = list(inspect.signature(nbls.narrow_band_least_squares).parameters)
    assert sig == [('ESTIMATORS' if p == 'ALPHA' else p) for p in ref]


def test_gather_kernel_uses_no_scratch(tmp_path):
    """``gather_pairs_kernel`` is a pure copy: no private segment, no spills (as tests/test_host.py asks of the hot kernels)."""
    import os
    import re
    import subprocess
    hipcc = '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    csrc = os.path.join(os.path.dirname(os.path.abspath(_hip.__file__)), 'csrc')
    out = tmp_path / 'solve.s'
    subprocess.run([hipcc, '-O3', '-std=c++17', '--offload-arch=gfx950', '-I' + csrc, '-S', '--cuda-device-only',
                    os.path.join(csrc, 'solve.hip'), '-o', str(out), '-ffp-contract=off'], check=True,
                   stderr=subprocess.DEVNULL, timeout=600)
    m = re.search(r'\.amdhsa_kernel \S*gather_pairs_kernel.*?\.amdhsa_private_segment_fixed_size (\d+)', out.read_text(), re.S)
    assert m and int(m.group(1)) == 0
