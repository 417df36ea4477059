"""References for the band-pass stage (csrc/filter.hip) that do not share its arithmetic.

``df2t_truth``       SciPy's DF2T cascade in 80-bit ``np.longdouble``: the truth the filter tests compare with.  SciPy's
                     own float64 ``sosfilt`` is off by up to 1e-11 of the output's scale at the narrowest bands of the
                     baseline configurations, so it cannot be the reference there.
``chunked_float64``  the chunked scan of filter.hip's header comment restated in NumPy float64.  It is not the code
                     under test: it tells a limit of the algorithm (the rounding of the carried start states) from a
                     bug of the kernels.

Also the case lists that tests/test_filter_truth.py (CPU) and tests/test_gpu_filter.py (GPU) share, so that the bound of
the narrow-band cases is derived on the CPU from exactly the cases the GPU runs.
"""
import os
import re

import numpy as np
from scipy import signal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.2e-16


def constants():
    """(C, T, G) = NBLS_FILTER_CHUNK, NBLS_FILTER_TILE, NBLS_FILTER_GROUP as csrc/nbls_internal.h defines them."""
    text = open(os.path.join(ROOT, 'narrow_band_least_squares_amd', 'csrc', 'nbls_internal.h')).read()
    out = []
    for name in ('NBLS_FILTER_CHUNK', 'NBLS_FILTER_TILE', 'NBLS_FILTER_GROUP'):
        m = re.search(r'^#define\s+%s\s+(\d+)\b' % name, text, re.M)
        assert m, '#define %s not found in nbls_internal.h' % name
        out.append(int(m.group(1)))
    return tuple(out)


def _require_extended():
    if np.finfo(np.longdouble).nmant < 63:
        raise RuntimeError('np.longdouble has a %d-bit mantissa on this platform: the filter truth needs the 80-bit '
                           'extended format (63 bits or more)' % np.finfo(np.longdouble).nmant)


def taper_window(npts, max_percentage=0.01):
    """The oracle's ``taper_window`` (obspy's Hann taper of 1 % per side)."""
    import nbls_oracle
    return nbls_oracle.taper_window(npts, max_percentage)


def df2t_forward(sos, x):
    """One causal pass of the cascade, zero initial state, in long double.  ``sos``: (S, 6), or (n, S, 6) with a filter
    of its own per series; ``x``: (n, npts).  -> (n, npts) long double.

    Per section SciPy's recurrence  y = b0 v + s1;  s1 = (b1 v - a1 y) + s2;  s2 = b2 v - a2 y.  The Python loop runs
    over time only: the series are a vector, and so are the sections — section s works on sample k - s in step k (its
    input is what section s - 1 gave one step earlier), which is the same arithmetic in another order of evaluation."""
    _require_extended()
    L = np.longdouble
    x = np.atleast_2d(np.asarray(x)).astype(L)
    n, npts = x.shape
    sos = np.asarray(sos, dtype=np.float64).astype(L)
    if sos.ndim == 2:
        sos = np.broadcast_to(sos, (n,) + sos.shape)
    assert sos.shape[0] == n and sos.shape[2] == 6
    S = sos.shape[1]
    a0 = sos[:, :, 3]
    b0, b1, b2, a1, a2 = (np.ascontiguousarray((sos[:, :, k] / a0).T) for k in (0, 1, 2, 4, 5))     # (S, n)
    xt = np.zeros((npts + S - 1, n), dtype=L)
    xt[:npts] = x.T
    out = np.empty((npts, n), dtype=L)
    s1 = np.zeros((S, n), dtype=L)
    s2 = np.zeros((S, n), dtype=L)
    v = np.zeros((S, n), dtype=L)
    y = np.zeros((S, n), dtype=L)
    for k in range(npts + S - 1):
        v[1:] = y[:-1]
        v[0] = xt[k]
        y = b0 * v + s1
        s1 = (b1 * v - a1 * y) + s2
        s2 = b2 * v - a2 * y
        if k >= S - 1:
            out[k - (S - 1)] = y[S - 1]
    return np.ascontiguousarray(out.T)


def df2t_truth(sos, x, zero_phase, taper=True):
    """What the filter stage computes for the series ``x`` (n, npts), in long double: the cascade; zero-phase = the
    same on the reversed forward output, reversed; then the 1 % Hann taper of the whole trace."""
    y = df2t_forward(sos, x)
    if zero_phase:
        y = df2t_forward(sos, y[:, ::-1])[:, ::-1]
    if taper:
        y = y * taper_window(y.shape[1]).astype(np.longdouble)
    return y


def truth_of_prefixes(sos, x, zero_phase, lengths, rows_of=None, forward=None):
    """``df2t_truth`` of x[rows, :n] for every n of ``lengths`` -> {n: (len(rows), n) long double}.  The causal pass runs
    once, over the longest length: the truth of a prefix is the prefix of the truth.  ``rows_of(n)``: the series that
    belong to length n (default: all).  ``forward``: ``df2t_forward(sos, x)`` where the caller has it already."""
    x = np.atleast_2d(x)
    fwd = df2t_forward(sos, x[:, :max(lengths)]) if forward is None else forward
    sos = np.asarray(sos)
    out = {}
    for n in lengths:
        rows = np.arange(x.shape[0]) if rows_of is None else np.asarray(rows_of(n))
        y = fwd[rows, :n]
        if zero_phase:
            y = df2t_forward(sos if sos.ndim == 2 else sos[rows], y[:, ::-1])[:, ::-1]
        out[n] = y * taper_window(n).astype(np.longdouble)
    return out


def scan_tables(sos, C):
    """Weights w_t = A^(C-1-t) g (C, 2S) and M = A^C (2S, 2S) of the chunk map  s_out = M s_in + sum_t w_t x_t, made
    from one long-double DF2T step and rounded to double."""
    _require_extended()
    L = np.longdouble
    sos = np.asarray(sos, dtype=np.float64).astype(L)
    S = sos.shape[0]
    D = 2 * S

    def step(st, x):
        st = st.copy()
        v = L(x)
        for s in range(S):
            b0, b1, b2, _, a1, a2 = sos[s]
            y = b0 * v + st[2 * s]
            st[2 * s], st[2 * s + 1] = (b1 * v - a1 * y) + st[2 * s + 1], b2 * v - a2 * y
            v = y
        return st

    A = np.zeros((D, D), dtype=L)
    for col in range(D):
        e = np.zeros(D, dtype=L)
        e[col] = 1
        A[:, col] = step(e, 0)
    w = step(np.zeros(D, dtype=L), 1)
    fw = np.empty((C, D), dtype=L)
    M = np.eye(D, dtype=L)
    for k in range(C):
        fw[C - 1 - k] = w
        w = A.dot(w)
        M = A.dot(M)
    return fw.astype(np.float64), M.astype(np.float64)


def _chunked_pass(sos, fw, M, x, C):
    """One causal pass (n, L) -> (n, L) in float64: end states of the whole chunks as weighted sums, sequential carry,
    every chunk filtered by ``sosfilt`` from its start state."""
    n, npts = x.shape
    S = sos.shape[0]
    nchunks = (npts + C - 1) // C
    whole = npts // C
    e = np.einsum('nct,td->ncd', x[:, :whole * C].reshape(n, whole, C), fw)       # zero-state end states
    start = np.zeros((n, nchunks, 2 * S))
    s = np.zeros((n, 2 * S))
    for c in range(nchunks):
        start[:, c] = s
        if c < whole:
            s = s.dot(M.T) + e[:, c]
    y = np.empty_like(x)
    if whole:
        zi = start[:, :whole].reshape(n * whole, S, 2).transpose(1, 0, 2)
        y[:, :whole * C] = signal.sosfilt(sos, x[:, :whole * C].reshape(n * whole, C), axis=-1,
                                          zi=np.ascontiguousarray(zi))[0].reshape(n, whole * C)
    if whole < nchunks:
        zi = start[:, whole].reshape(n, S, 2).transpose(1, 0, 2)
        y[:, whole * C:] = signal.sosfilt(sos, x[:, whole * C:], axis=-1, zi=np.ascontiguousarray(zi))[0]
    return y


def chunked_float64(sos, x, zero_phase, taper=True, C=None):
    """The algorithm of filter.hip's header comment in NumPy float64 (``x``: (n, npts)).  The backward pass pads its
    index space at the start to a whole number of chunks, as the kernels do, so that its chunks coincide with the
    forward ones."""
    C = C or constants()[0]
    sos = np.asarray(sos, dtype=np.float64)
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    fw, M = scan_tables(sos, C)
    y = _chunked_pass(sos, fw, M, x, C)
    if zero_phase:
        npts = x.shape[1]
        pad = -npts % C
        z = np.concatenate([np.zeros((x.shape[0], pad)), y[:, ::-1]], axis=1)
        y = _chunked_pass(sos, fw, M, z, C)[:, pad:][:, ::-1]
    if taper:
        y = y * taper_window(y.shape[1])
    return y


def scipy_float64(sos, x, zero_phase, taper=True):
    """The oracle's ``filter_data`` arithmetic on an array: SciPy's float64 ``sosfilt``."""
    y = signal.sosfilt(sos, x, axis=-1)
    if zero_phase:
        y = signal.sosfilt(sos, y[:, ::-1], axis=-1)[:, ::-1]
    if taper:
        y = y * taper_window(y.shape[1])
    return y


def design(ftype, lo, hi, order, fs, rp=0.01):
    """The SOS the project applies for this band (the oracle's ``design_bandpass``)."""
    import nbls_oracle
    return nbls_oracle.design_bandpass(ftype, lo, hi, order, rp, fs)[0]


def rel_err(y, truth):
    """max |y - truth| as a fraction of max |truth| (NaN where either is not finite everywhere)."""
    return float(np.max(np.abs(y.astype(np.longdouble) - truth)) / np.max(np.abs(truth)))


def noise_with_tone(seed, nchans, npts, fs, lo, hi):
    """Seeded white noise plus a sinusoid at the band's (geometric) centre, a phase of its own per channel."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((nchans, npts))
    t = np.arange(npts) / fs
    for ch in range(nchans):
        x[ch] += np.sin(2.0 * np.pi * np.sqrt(lo * hi) * t + rng.uniform(0.0, 2.0 * np.pi))
    return x


# ---- length and shape boundaries (well-conditioned bands at 20 Hz: the stated 1e-11 holds against the truth) ----
FS = 20.0
TOL = 1e-11                 # of max |truth|: the project's stated tolerance
TOL_FORMS = 1e-13           # option forms against the default form: another order of summation, not bit for bit

# name -> (type, low edge, high edge, order, zero-phase); sections = order (band-pass)
FILTERS = {
    'cheby1_2s_causal': ('cheby1', 0.5, 2.0, 2, False),
    'butter_2s_zero_phase': ('butter', 0.5, 2.0, 2, True),        # recompute form, matrix-core states
    'butter_3s_zero_phase': ('butter', 0.8, 3.0, 3, True),        # recompute form, VALU states
    'butter_8s_zero_phase': ('butter', 0.8, 3.0, 8, True),        # stored form, fused backward states
    'cheby1_5s_causal': ('cheby1', 0.8, 3.0, 5, False),
}
TWO_SECTION = ('cheby1_2s_causal', 'butter_2s_zero_phase')
FORMS = {'nofuse': ('filter_nofuse',), 'nomfma': ('filter_nomfma',), 'nofuse_nomfma': ('filter_nofuse', 'filter_nomfma')}


def boundary_lengths(C, T, G):
    """Every trace length at or next to a seam of the scan: taper length 0 -> 1, the chunk, the LDS tile, the 16-chunk
    column tile of the matrix-core state kernel, the carry group / apply workgroup, three groups, and a long one."""
    out = [1, 15, 16, 17, 99, 100, 101,
           C - 1, C, C + 1, C + T - 1, C + T, C + T + 1, 2 * C,
           16 * C - 1, 16 * C, 16 * C + 1,
           (G - 1) * C, G * C - 1, G * C, G * C + 1, G * C + T, (G + 1) * C, (G + 1) * C + 1,
           2 * G * C - 1, 2 * G * C, 2 * G * C + 1, (2 * G + 1) * C + 7,
           203 * C + 229]
    assert len(set(out)) == len(out) and out[-1] >= 200 * C
    return out


def multiband_lengths(C, T, G):
    return [C + 1, G * C + 1, (2 * G + 1) * C + 7]


def crafted(npts, C, G):
    """Unit impulses at the samples C-1, C, G*C-1, G*C and npts-1 (those inside the trace) on a DC offset: a wrong
    start state at a seam shows up as a step, not as noise."""
    x = np.full(npts, 0.25)
    for p in (C - 1, C, G * C - 1, G * C, npts - 1):
        if 0 <= p < npts:
            x[p] += 1.0
    return x


MULTIBAND_EDGES = [(0.5 + 0.25 * i, 1.5 + 0.5 * i) for i in range(9)]      # nine different bands below Nyquist (10 Hz)
MULTIBAND_NBANDS = (1, 3, 5, 9)
# (type, order = sections, zero-phase): state sizes 2, 4 and 8 all take the matrix-core state kernel
MULTIBAND_FILTERS = [('butter', 1, True), ('butter', 2, True), ('butter', 4, True), ('cheby1', 2, False)]
MULTIBAND_NCHANS = (3, 8)


# ---- narrow bands: the bound is the reference's own float64 error times a margin measured on the CPU ----
# (type, low, high, order, fs): the narrow rows of the issue's table, then the first bands of cfg-5 and cfg-3
NARROW_BANDS = [
    ('butter', 0.1, 0.1049, 2, 100.0),
    ('butter', 0.1, 0.1037, 2, 200.0),
    ('butter', 0.02, 0.04, 4, 100.0),
    ('cheby1', 0.05, 0.1, 4, 200.0),
    ('butter', 0.1, 0.16, 2, 20.0),
    ('butter', 0.1, 0.1031, 2, 20.0),
    ('butter', 0.1, 0.11, 2, 40.0),
]
NARROW_LENGTHS = (70001, 300007)
NARROW_NCHANS = 3
# K of  e_gpu <= K * e_ref + 64 eps:  the worst e_emu / e_ref that tests/test_filter_truth.py measures over
# narrow_cases() on the CPU, doubled and rounded up to a power of two.  Never taken from what the kernel gives.
NARROW_K = 64.0


def narrow_cases():
    """(band index, zero_phase): Butterworth bands causal (one pass) and zero-phase (as the package applies them),
    Chebyshev bands causal (the package never runs them zero-phase)."""
    out = []
    for i, (ftype, _, _, _, _) in enumerate(NARROW_BANDS):
        out.append((i, False))
        if ftype == 'butter':
            out.append((i, True))
    return out


def narrow_input(i):
    ftype, lo, hi, order, fs = NARROW_BANDS[i]
    return noise_with_tone(1000 + i, NARROW_NCHANS, max(NARROW_LENGTHS), fs, lo, hi)


def narrow_bound(e_ref):
    return NARROW_K * e_ref + 64.0 * EPS
