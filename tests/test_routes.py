"""The correlator route (nbls_route_xcorr / nbls_route_table, csrc/xcorr_route.hip) on the host: every window length
of every array size must give kernels whose LDS fits a CU, every kernel instance must be reachable, the static LDS the
route counts must be what the compiler gave each kernel, and the boundary helper that the GPU tests draw their window
lengths from must find every place where the route changes."""
import os
import re
import subprocess

import numpy as np
import pytest

from narrow_band_least_squares_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'narrow_band_least_squares_amd', 'csrc')
LDS_CU = 160 * 1024
W_MAX = 16384
NS = range(3, 33)

# kernel symbol (a substring of the mangled name) of each (stage, instance) the route can name
QUANT_KERNELS = {1: 'quantize_kernel', 2: 'quantize_reg_kernelILi2E', 3: 'quantize_reg_kernelILi3E',
                 4: 'quantize_reg_kernelILi4E', 6: 'quantize_reg_kernelILi6E', 8: 'quantize_reg_kernelILi8E'}
SCREEN_KERNELS = {1: 'screen_kernelILi4ELi8E', 2: 'screen_kernelILi4ELi4E', 3: 'screen_kernelILi8ELi8E'}
VERIFY_KERNELS = {1: 'verify_dma_kernel', 2: 'verify_lds_kernel', 3: 'verify_kernel'}
GENERAL_KERNELS = {_hip.ROUTE_MFMA: 'xcorr_mfma_kernel', _hip.ROUTE_VALU_LDS: 'xcorr_simple_kernel',
                   _hip.ROUTE_VALU_GLOBAL: 'xcorr_simple_kernel'}


def _scan():
    """(N, impl, vrows, npts_pad, table) for every combination the invariants cover."""
    for n in NS:
        for impl in (0, 1, 2, 3):
            for vrows in (1, 64):
                for npts_pad in (6400, 6401):
                    yield n, impl, vrows, npts_pad, _hip.route_table(n, 2, W_MAX, vrows=vrows, npts_pad=npts_pad,
                                                                      xcorr_impl=impl)


def _launched(t):
    """Per stage: the mask of the rows that launch a kernel in that stage, and the kernel's symbol per row."""
    scr = t['correlator'] == _hip.ROUTE_SCREEN
    gen = np.isin(t['correlator'], list(GENERAL_KERNELS))
    return {_hip.ROUTE_QUANTIZE: (scr, t['quant_inst'], QUANT_KERNELS),
            _hip.ROUTE_SCREEN_STAGE: (scr, t['screen_inst'], SCREEN_KERNELS),
            _hip.ROUTE_VERIFY: (scr, t['verifier'], VERIFY_KERNELS),
            _hip.ROUTE_GENERAL: (gen, t['correlator'], GENERAL_KERNELS)}


def _runs(ws):
    """[3, 4, 5, 9] -> '3..5, 9'"""
    out, i = [], 0
    while i < len(ws):
        j = i
        while j + 1 < len(ws) and ws[j + 1] == ws[j] + 1:
            j += 1
        out.append('%d' % ws[i] if i == j else '%d..%d' % (ws[i], ws[j]))
        i = j + 1
    return ', '.join(out)


def test_every_route_fits_a_cu():
    """N 3..32, W 2..16384, every xcorr_impl, 1 and 64 result rows, both parities of the padded trace length: every
    kernel a route launches asks for at most a CU's LDS, dynamic and static together — or the route reports that a
    forced correlator does not take the window.  (xcorr_simple_kernel used to keep both windows in LDS up to 2 * W * 8 B
    = 160 KB, without its 80 B of static LDS: W = 10 236..10 240 failed to launch on the VALU correlator.)"""
    bad = []
    for n, impl, vrows, npts_pad, t in _scan():
        ws = np.arange(2, W_MAX + 1)
        rejected = t['correlator'] == _hip.ROUTE_REJECTED
        if impl in (0, 1):
            assert not rejected.any(), (n, impl, ws[rejected][:5])           # the automatic and the VALU route take any W
        for stage, (mask, inst, names) in _launched(t).items():
            over = mask & (t['lds_dyn'][:, stage] + t['lds_static'][:, stage] > LDS_CU)
            if over.any():
                bad.append('N=%d impl=%d vrows=%d npts_pad=%d stage %d (%s): W = %s' % (
                    n, impl, vrows, npts_pad, stage, names[int(inst[over][0])], _runs(list(ws[over]))))
            assert not np.any(t['lds_dyn'][~mask, stage]) and not np.any(t['lds_static'][~mask, stage])
    assert not bad, 'routes beyond a CU\'s LDS:\n' + '\n'.join(bad[:40])


def test_every_kernel_instance_is_reachable():
    """Each quantiser, screening, verifier and general-correlator form is chosen by some (N, W) of the scan with the
    default options, and the forced routes are rejected somewhere (else their check would be dead code)."""
    seen = {k: set() for k in ('correlator', 'quant_inst', 'screen_inst', 'verifier', 'verify_threads')}
    for n, impl, vrows, npts_pad, t in _scan():
        for k in seen:
            scr = t['correlator'] == _hip.ROUTE_SCREEN
            seen[k] |= set(np.unique(t[k] if k == 'correlator' else t[k][scr]).tolist())
    assert seen['correlator'] == {0, 1, 2, 3, 4}
    assert seen['quant_inst'] == set(QUANT_KERNELS)
    assert seen['screen_inst'] == set(SCREEN_KERNELS)
    assert seen['verifier'] == set(VERIFY_KERNELS)
    assert seen['verify_threads'] == {256, 512, 1024}


def test_routes_follow_the_forced_correlator():
    """impl 3 is the automatic route where that screens and rejected elsewhere; impl 2 is the automatic general route
    where that is the f64-MFMA kernel and rejected elsewhere; impl 1 is always the VALU kernel; the reported xcorr_impl
    follows the correlator."""
    want_impl = {0: 0, 1: 3, 2: 2, 3: 1, 4: 1}
    for n in (3, 8, 16, 17, 32):
        auto, valu, mfma, scr = (_hip.route_table(n, 2, W_MAX, xcorr_impl=i) for i in (0, 1, 2, 3))
        for t in (auto, valu, mfma, scr):
            np.testing.assert_array_equal(t['impl'], [want_impl[c] for c in t['correlator']])
        s = auto['correlator'] == _hip.ROUTE_SCREEN
        assert np.array_equal(scr[s], auto[s]) and np.all(scr['correlator'][~s] == _hip.ROUTE_REJECTED)
        assert np.all(np.isin(valu['correlator'], [_hip.ROUTE_VALU_LDS, _hip.ROUTE_VALU_GLOBAL]))
        g = ~s
        m = auto['correlator'] == _hip.ROUTE_MFMA
        assert np.array_equal(mfma[m], auto[m])
        assert np.all(mfma['correlator'][g & ~m] == _hip.ROUTE_REJECTED)
        assert np.all(np.isin(auto['correlator'][g & ~m], [_hip.ROUTE_VALU_LDS, _hip.ROUTE_VALU_GLOBAL]))
        assert np.array_equal(auto[g & ~m], valu[g & ~m])
    assert (n > 16) == (not np.any(mfma['correlator'] == _hip.ROUTE_MFMA))
    # the VALU kernel's windows leave LDS exactly where 2 * W * 8 B and its static part outgrow a CU
    v = _hip.route_table(8, 10230, 10245, xcorr_impl=1)
    assert list(v['correlator']) == [_hip.ROUTE_VALU_LDS] * 6 + [_hip.ROUTE_VALU_GLOBAL] * 10
    assert 2 * 10235 * 8 + 80 <= LDS_CU < 2 * 10236 * 8 + 80
    with pytest.raises(ValueError):
        _hip.route(8, 1)
    with pytest.raises(ValueError):
        _hip.route(8, 100, xcorr_impl=4)


def test_route_boundaries_straddle_every_change():
    """route_boundaries (the window lengths of tests/test_gpu_routes.py) lists exactly the adjacent W whose routes
    differ — checked here against single nbls_route_xcorr calls, not the table the helper scans — and includes the
    switches of the screening geometry worked out by hand for eight elements."""
    for n in (3, 5, 8, 12, 17, 32):
        b = _hip.route_boundaries(n)
        assert b and all(w1 == w0 + 1 for w0, w1 in b)
        for w0, w1 in b:
            r0, r1 = _hip.route(n, w0), _hip.route(n, w1)
            assert any(r0[k] != r1[k] for k in _hip.ROUTE_KEYS), (n, w0, w1)
        t = _hip.route_table(n, 2, W_MAX)
        firsts = {w1 for _, w1 in b}
        for w in range(3, W_MAX + 1):
            if w not in firsts:
                assert all(t[k][w - 2] == t[k][w - 3] for k in _hip.ROUTE_KEYS), (n, w)
    firsts8 = {w1 for _, w1 in _hip.route_boundaries(8)}
    assert {64, 1329, 4977, 5425, 5825, 6353, 6913, 7569, 7729, 8513, 9745, 11105, 13009} <= firsts8
    assert _hip.route(8, 63)['correlator'] != _hip.ROUTE_SCREEN == _hip.route(8, 64)['correlator']
    assert _hip.route(8, 13008)['correlator'] == _hip.ROUTE_SCREEN != _hip.route(8, 13009)['correlator']
    # the verifier's LDS grows by 8 B per result row: rows can move a window length off the DMA verifier
    assert _hip.route(3, 3410, vrows=1)['verifier'] == 1 and _hip.route(3, 3410, vrows=9)['verifier'] == 2


def test_static_lds_matches_the_compiled_kernels(tmp_path):
    """The static LDS the route adds for each kernel is the .amdhsa_group_segment_fixed_size of that kernel in the
    gfx950 code object (xcorr_simple_kernel: 80 B, verify_kernel: 16 640 B, the others none)."""
    hipcc = '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    procs = []
    for src in ('xcorr.hip', 'xcorr_screen.hip'):
        out = tmp_path / (src + '.s')
        procs.append((out, subprocess.Popen([hipcc, '-O3', '-std=c++17', '--offload-arch=gfx950', '-I' + CSRC, '-S',
                                             '--cuda-device-only', os.path.join(CSRC, src), '-o', str(out)],
                                            stderr=subprocess.DEVNULL)))
    fixed = {}
    for out, p in procs:
        assert p.wait(timeout=900) == 0
        for name, size in re.findall(r'\.amdhsa_kernel (\S+).*?\.amdhsa_group_segment_fixed_size (\d+)', out.read_text(), re.S):
            fixed[name] = int(size)

    def compiled(sym):
        hits = [v for k, v in fixed.items() if re.search(r'\d' + sym, k)]
        assert len(hits) == 1, (sym, sorted(fixed))
        return hits[0]

    checked = set()
    for n, impl, vrows, npts_pad, t in _scan():
        for stage, (mask, inst, names) in _launched(t).items():
            for i in np.unique(inst[mask]):
                sym = names[int(i)]
                st = np.unique(t['lds_static'][mask & (inst == i), stage])
                assert len(st) == 1 and st[0] == compiled(sym), (sym, st, compiled(sym))
                checked.add(sym)
    assert checked == set(QUANT_KERNELS.values()) | set(SCREEN_KERNELS.values()) | set(VERIFY_KERNELS.values()) | \
        set(GENERAL_KERNELS.values())
    assert compiled('xcorr_simple_kernel') == 80 and compiled('verify_kernel') == 16640
