"""The filter references of tests/filter_truth.py, checked on the CPU: the long-double truth against SciPy where float64
is good and against a closed form, the float64 restatement of the chunked scan against the truth, and the margin K of
the narrow-band bound that tests/test_gpu_filter.py asserts — measured here, from the emulation, never from the kernel."""
import functools

import numpy as np
import pytest

import filter_truth as ft


def test_scan_constants_are_read_from_the_header():
    C, T, G = ft.constants()
    assert C % T == 0 and C % 64 == 0 and 64 % T == 0 and G >= 1
    lengths = ft.boundary_lengths(C, T, G)
    assert {1, C - 1, C, C + 1, 16 * C, G * C - 1, G * C, G * C + 1, 2 * G * C, (2 * G + 1) * C + 7} <= set(lengths)
    assert all(n in lengths for n in (99, 100, 101))            # taper length int(0.01 n): 0, 1, 1
    assert len(ft.taper_window(99)) == 99 and ft.taper_window(99).min() == 1.0 and ft.taper_window(100)[0] == 0.0


def test_truth_needs_the_extended_format(monkeypatch):
    """A platform whose long double is a double must fail loudly, not skip and not pass with a float64 'truth'."""
    real = np.finfo

    class Narrow:
        nmant = 52
    monkeypatch.setattr(np, 'finfo', lambda t: Narrow if t is np.longdouble else real(t))
    with pytest.raises(RuntimeError):
        ft.df2t_forward(np.array([[1.0, 0, 0, 1.0, 0, 0]]), np.ones((1, 4)))
    monkeypatch.undo()
    assert np.finfo(np.longdouble).nmant >= 63


@pytest.mark.parametrize('name', list(ft.FILTERS))
def test_truth_agrees_with_scipy_on_wide_bands(name):
    """0.5-2 Hz and 0.8-3 Hz at 20 Hz, 1 to 8 sections: SciPy's float64 sosfilt is good to a few 1e-15 there."""
    ftype, lo, hi, order, zero_phase = ft.FILTERS[name]
    sos = ft.design(ftype, lo, hi, order, ft.FS)
    assert sos.shape == (order, 6)
    x = ft.noise_with_tone(7, 3, 70000, ft.FS, lo, hi)
    truth = ft.df2t_truth(sos, x, zero_phase)
    assert truth.dtype == np.longdouble and truth.shape == x.shape
    assert ft.rel_err(ft.scipy_float64(sos, x, zero_phase), truth) <= 1e-13
    assert ft.rel_err(ft.chunked_float64(sos, x, zero_phase), truth) <= 1e-13
    # a filter of its own per series, and the truth of a prefix
    both = ft.df2t_truth(np.stack([sos, sos, sos]), x, zero_phase)
    np.testing.assert_array_equal(both, truth)
    pre = ft.truth_of_prefixes(sos, x, zero_phase, [513, 70000], rows_of=lambda n: [0, 2])
    np.testing.assert_array_equal(pre[70000], truth[[0, 2]])
    np.testing.assert_array_equal(pre[513], ft.df2t_truth(sos, x[[0, 2], :513], zero_phase))


@pytest.mark.parametrize('ftype,lo,hi,fs', [('butter', 0.5, 2.0, 20.0), ('butter', 0.1, 0.1049, 100.0), ('butter', 0.8, 3.0, 20.0)])
def test_truth_impulse_response_of_one_section_in_closed_form(ftype, lo, hi, fs):
    """H(z) = (b0 + b1/z + b2/z^2) / (1 + a1/z + a2/z^2) with poles r exp(+-i theta):
    h[n] = b0 g[n] + b1 g[n-1] + b2 g[n-2],  g[n] = r^n sin((n + 1) theta) / sin(theta)."""
    L = np.longdouble
    sos = ft.design(ftype, lo, hi, 1, fs)
    assert sos.shape == (1, 6)
    b0, b1, b2, _, a1, a2 = sos[0].astype(L)
    assert a1 * a1 < 4 * a2                                  # complex pole pair
    r = np.sqrt(a2)
    theta = np.arccos(-a1 / (2 * r))
    npts = 6000
    n = np.arange(-2, npts).astype(L)
    g = np.where(n >= 0, r ** n * np.sin((n + 1) * theta) / np.sin(theta), L(0))
    h = b0 * g[2:] + b1 * g[1:-1] + b2 * g[:-2]
    x = np.zeros((1, npts))
    x[0, 0] = 1.0
    got = ft.df2t_truth(sos, x, False, taper=False)[0]
    # the closed form is the less exact side: theta = arccos(c) with c next to 1 carries eps_L / sin(theta), and the
    # phase (n + 1) theta multiplies that by n (eps_L = 2^-63, the long double's unit); a factor 8 for the other roundings
    tol = 8 * npts * float(np.finfo(L).eps) / float(np.sin(theta))
    assert tol < 1e-12
    assert np.max(np.abs(got - h)) <= tol * np.max(np.abs(h))


def test_emulation_handles_every_boundary_length():
    """The restatement itself at every length of the GPU list (a subset of the filters: it is float64 NumPy, cheap)."""
    C, T, G = ft.constants()
    lengths = ft.boundary_lengths(C, T, G)
    for name in ('cheby1_2s_causal', 'butter_3s_zero_phase'):
        ftype, lo, hi, order, zero_phase = ft.FILTERS[name]
        sos = ft.design(ftype, lo, hi, order, ft.FS)
        x = ft.noise_with_tone(11, 1, max(lengths), ft.FS, lo, hi)
        x[0] += np.pad(ft.crafted(2 * G * C, C, G), (0, max(lengths) - 2 * G * C))
        truth = ft.truth_of_prefixes(sos, x, zero_phase, lengths)
        for n in lengths:
            y = ft.chunked_float64(sos, x[:, :n], zero_phase)
            assert y.shape == (1, n)
            assert np.max(np.abs(y - truth[n])) <= ft.TOL * np.max(np.abs(truth[n])), (name, n)


@functools.lru_cache(maxsize=None)
def _narrow_table():
    rows = []
    for i, (ftype, lo, hi, order, fs) in enumerate(ft.NARROW_BANDS):
        sos = ft.design(ftype, lo, hi, order, fs)
        x = ft.narrow_input(i)
        for zero_phase in [zp for (j, zp) in ft.narrow_cases() if j == i]:
            truth = ft.truth_of_prefixes(sos, x, zero_phase, ft.NARROW_LENGTHS)
            for n in ft.NARROW_LENGTHS:
                e_ref = ft.rel_err(ft.scipy_float64(sos, x[:, :n], zero_phase), truth[n])
                e_emu = ft.rel_err(ft.chunked_float64(sos, x[:, :n], zero_phase), truth[n])
                rows.append((ftype, lo, hi, order, fs, zero_phase, n, e_ref, e_emu))
    return rows


def test_narrow_band_margin_comes_from_the_emulation():
    """Prints e_ref (SciPy float64), e_emu (chunked float64) against the long-double truth for every narrow-band case,
    and derives K: the worst e_emu / e_ref, doubled, rounded up to a power of two.  The committed NARROW_K is that
    number, and the emulation stays inside the bound that the GPU test asserts."""
    rows = _narrow_table()
    assert len(rows) == len(ft.narrow_cases()) * len(ft.NARROW_LENGTHS)
    worst = 0.0
    print()
    print('%-7s %-15s %3s %5s %-10s %7s %10s %10s %7s' % ('type', 'band', 'ord', 'fs', 'pass', 'npts', 'e_ref', 'e_emu', 'ratio'))
    for ftype, lo, hi, order, fs, zero_phase, n, e_ref, e_emu in rows:
        ratio = e_emu / e_ref
        worst = max(worst, ratio)
        print('%-7s %-15s %3d %5g %-10s %7d %10.2e %10.2e %7.2f' % (ftype, '%g-%g' % (lo, hi), order, fs,
                                                                  'zero-phase' if zero_phase else 'causal', n, e_ref, e_emu, ratio))
    K = 2.0 ** np.ceil(np.log2(2.0 * worst))
    print('worst e_emu / e_ref = %.2f  ->  K = %g  (committed: %g)' % (worst, K, ft.NARROW_K))
    assert K == ft.NARROW_K
    for ftype, lo, hi, order, fs, zero_phase, n, e_ref, e_emu in rows:
        assert e_emu <= ft.narrow_bound(e_ref), (ftype, lo, hi, fs, zero_phase, n, e_ref, e_emu)
