"""Lag tables made of unit pulses, the paths the oracle takes on them, and an exact-rational OLS truth, for the solve
kernels (csrc/solve.hip, solve_bucket.inc, lts_bucket*.h).  CPU only: nothing here imports the GPU library.

**Pulse tables.**  A pre-filtered pass plans no filter section and no taper, so the correlators read the caller's
samples as they are.  A window that holds ONE unit pulse per channel, at sample ``p_i`` in channel i, correlates to
``lag_ij = p_j - p_i`` with ``cmax = 1`` exactly (one product 1 * 1, every other lag 0): the trace IS the lag table.
With hop = W = 64 samples every window is its own table.

**Geometry.**  ``grid_geometry(N)``: N distinct points whose coordinates are multiples of 0.25 km.  With fs = 20 Hz and a
slowness in multiples of 0.2 s/km, ``fs * x_ij . z = (4 x_ij) . (5 z)`` is an integer: an integer-delay plane wave is an
exact fit of the lag table (residuals of about 1e-17 s: 0.2 is not a binary fraction).

**Mistimed elements and the breakdown point.**  A mistimed element puts the same offset on all its N - 1 pairs, so those
pairs can never lie on the plane of the others: the pairs on one plane are the C(N - b, 2) pairs of the N - b clean
elements.  An exact fit (raw LTS scale below ``LTS_ZERO_SCALE``) needs h of them.  At ALPHA = 0.5 that holds for one
mistimed element from 5 elements on (6 >= 6) and for two from 8 on (15 >= 15, the breakdown edge), and for no N below.
``tables`` therefore names a row ``one_bad`` / ``two_bad`` only where C(N - b, 2) >= h(0.5) and ``one_bad_past_breakdown``
/ ``two_bad_past_breakdown`` where it is not (same pulses): the first kind must classify as exact fit, the second cannot.

**OLS truth.**  ``ols_truth`` evaluates, in ``fractions.Fraction`` on the very float64 values the kernel is given
(``xpinv``, ``xij``, ``tau_k = float(lag_k) / fs``),

    z*      = sum_k xpinv_k tau_k
    acc*(z) = sum_k tau_k (tau_k - x_k0 z_0 - x_k1 z_1)            for a given float64 z

and the rounding bounds of the kernel's (and the oracle's) un-fused sequential float64 sums.  With u = 2^-53 and
gamma_n = n u / (1 - n u) (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1 and lemma 3.3):

* z: every product is rounded once and the P terms are added in order, the classical inner-product bound
  ``|z - z*| <= gamma_P sum_k |xpinv_k tau_k|``.
* acc: ``m_k = fl(fl(x_k0 z_0) + fl(x_k1 z_1))`` has ``|m_k - m*_k| <= gamma_2 (|x_k0 z_0| + |x_k1 z_1|)``;
  ``r_k = fl(tau_k - m_k)`` adds one rounding of a value no larger than ``|tau_k| + (1 + gamma_2)(...)``, so with
  ``B_k = |tau_k| + |x_k0 z_0| + |x_k1 z_1|`` we have ``|r_k - r*_k| <= gamma_3 B_k`` and ``|r*_k| <= B_k``.  The sum
  ``fl(sum_k tau_k r_k)`` is an inner product of the computed r_k: ``gamma_P sum |tau_k| |r_k|`` more.  Together
  ``(gamma_P + gamma_3 + gamma_P gamma_3) sum |tau_k| B_k <= gamma_{P+3} sum_k |tau_k| B_k =: E_acc``.
* sigma_tau = fl(sqrt(fl(acc / (P - 2)))): one rounding each, so the exact square of the float64 sigma_tau times P - 2
  is within ``gamma_3 |acc|`` of the computed acc, and ``|acc| <= |acc*| + E_acc``:
  ``|sigma_tau^2 (P - 2) - acc*| <= E_acc + gamma_3 (|acc*| + E_acc) =: E_sigma``.

None of these is a measured number."""
import functools
import math
from fractions import Fraction

import numpy as np

FS = 20.0
W = 64
CENTRE = 32
DX_KM = 0.25                                     # grid step of the geometry
DZ = 0.2                                         # step of the slowness vectors (s/km)
SLOWNESS = ((1, 2), (-2, 1), (0, 0))             # in units of DZ: (0.2, 0.4), (-0.4, 0.2) s/km and vertical incidence
KINDS = ('exact', 'one_bad', 'two_bad', 'one_bad_by_1')
OFF_G, OFF_S = 17, 5                             # the off-closure row: gap between the two pulses, shift of channel c

# (N, ALPHA) of tests/test_gpu_solve.py: the register-resident LTS kernel, the bucket kernel, OLS
LTS_REGISTER = tuple((n, a) for n in (4, 5, 6, 7, 8) for a in (0.5, 0.75))
LTS_BUCKET = ((9, 0.5), (12, 0.75), (16, 0.5), (23, 0.5), (24, 0.5), (32, 0.5))
LTS_CASES = LTS_REGISTER + LTS_BUCKET
OLS_N = (3, 8, 11, 12, 32)


def half_h(P):
    """h of ALPHA = 0.5 for P pairs and two unknowns (robustbase h.alpha.n): 2 n2 - P + (P - n2), n2 = (P + 3) // 2."""
    n2 = (P + 3) // 2
    return 2 * n2 - P + (P - n2)


def within_breakdown(N, nbad):
    """Whether the pairs of the N - nbad clean elements alone are an h-subset at ALPHA = 0.5."""
    m = N - nbad
    return m * (m - 1) // 2 >= half_h(N * (N - 1) // 2)


@functools.lru_cache(maxsize=None)
def grid_units(N):
    """N distinct integer points (units of DX_KM) in [-6, 6]^2 -> (N, 2) int64.  The first four are a parallelogram: the
    pairs (0, 1), (2, 3) share one baseline vector and (0, 2), (1, 3) another, so equal lags on them give bit-equal
    residuals for ANY fit — the only way two |r| tie in floating point, and what the small arrays need for a tie across
    position h.  The rest come from a 16-bit linear congruential sequence whose seed counts up until the co-array has
    rank 2 and a non-zero median |x| on both axes (what the planner's ``lts_plan`` standardises with); nothing else is
    selected for."""
    for seed in range(1, 1000):
        s = seed * 7919 % 65536
        pts = [(0, 0), (3, 1), (1, 4), (4, 5)][:N]
        while len(pts) < N:
            s = (s * 5761 + 999) % 65536
            a = s % 13 - 6
            s = (s * 5761 + 999) % 65536
            b = s % 13 - 6
            if (a, b) not in pts:
                pts.append((a, b))
        q = np.array(pts, dtype=np.int64)
        d = np.array([q[i] - q[j] for i in range(N - 1) for j in range(i + 1, N)])
        if np.linalg.matrix_rank(d) == 2 and np.all(np.median(np.abs(d), axis=0) > 0):
            return q
    raise AssertionError('no geometry for %d elements' % N)


def grid_geometry(N):
    """rij (2, N) in km: multiples of 0.25 km, co-array of rank 2 with a non-zero MAD on both axes (asserted)."""
    rij = np.ascontiguousarray(grid_units(N).T * DX_KM)
    xij = np.array([rij[:, i] - rij[:, j] for i in range(N - 1) for j in range(i + 1, N)])
    assert len({tuple(c) for c in rij.T}) == N
    assert np.linalg.matrix_rank(xij) == 2
    assert np.all(1.4826 * np.median(np.abs(xij), axis=0) > 0)
    return rij


def pair_table(N):
    return [(i, j) for i in range(N - 1) for j in range(i + 1, N)]


def default_slowness(N):
    """The slowness vectors of the tables of an N-element case: the oracle's FAST-LTS takes seconds per window from 16
    elements on, so large arrays drop slowness vectors (never a table kind, see ``tables``)."""
    return SLOWNESS if N < 16 else (SLOWNESS[0], SLOWNESS[2]) if N < 20 else SLOWNESS[:1]


def tables(N, W=W, slowness=None, nrandom=None, short=None):
    """-> list of (name, rows): ``rows[i]`` is the list of (sample, amplitude) pulses of channel i in that window.

    Per slowness vector s (units of DZ; ``d_i = q_i . s`` samples, ``p_i = CENTRE - d_i``): ``exact``; ``one_bad`` (last
    element + 7); ``two_bad`` (last + 7, first - 5); ``one_bad_by_1`` (last + 1) — a mistimed row beyond the breakdown
    point of ALPHA = 0.5 carries ``_past_breakdown`` in its name (module docstring).  Then ``all_same``, ``all_but_one_same``,
    ``extreme`` (one element at 0, one at W - 1), seeded ``random`` rows and ``off_closure``: the first ``exact`` row with
    two pulses in two channels (a: 1.0 at p_a, 0.8 at p_a + g; c: 0.8 at p_c + s, 1.0 at p_c + s + g, nothing at p_c), so
    that the two 0.8 * 1.0 products meet at one lag (1.6 > 1) and the pair (a, c) alone misses closure, by -g.  With
    s = 5 channel c is a mistimed element as well (by s + g); ``off_closure_on_plane`` is the same with s = -g.

    ``short`` (default: N >= 32, where the oracle takes 8 s per window that is not MAD = 0) keeps ``exact``, ``two_bad``,
    ``off_closure`` and the three rows whose MAD(tau) is 0 there (``all_same``, ``all_but_one_same``, ``extreme``);
    ``nrandom`` defaults to 4 below 16 elements and 1 from there on."""
    q = grid_units(N)
    slowness = default_slowness(N) if slowness is None else slowness
    short = (N >= 32) if short is None else short
    nrandom = (4 if N < 16 else 1) if nrandom is None else nrandom
    out = []

    def single(p):
        p = [int(v) for v in p]
        assert min(p) >= 0 and max(p) < W, p
        return [[(v, 1.0)] for v in p]

    for s in slowness:
        d = q[:, 0] * s[0] + q[:, 1] * s[1]
        p = CENTRE - d
        tag = 'z(%d,%d)' % s
        for kind in KINDS:
            pk = p.copy()
            nbad = 0
            if kind in ('one_bad', 'two_bad'):
                pk[-1] += 7
                nbad = 1
            if kind == 'two_bad':
                pk[0] -= 5
                nbad = 2
            if kind == 'one_bad_by_1':
                pk[-1] += 1
            if short and kind not in ('exact', 'two_bad'):
                continue
            past = nbad and not within_breakdown(N, nbad)
            out.append(('%s%s %s' % (kind, '_past_breakdown' if past else '', tag), single(pk)))
    out.append(('all_same', single([CENTRE] * N)))
    out.append(('all_but_one_same', single([CENTRE] * (N - 1) + [CENTRE + 9])))
    out.append(('extreme', single([0] + [CENTRE] * (N - 2) + [W - 1])))
    if not short:
        rng = np.random.default_rng(1000 + N)
        for k in range(nrandom):
            out.append(('random %d' % k, single(rng.integers(0, W, size=N))))
    # off closure: channels a < c, the two earliest pulses of the first exact row (room for + s + g behind them)
    s = slowness[0]
    p = CENTRE - (q[:, 0] * s[0] + q[:, 1] * s[1])
    a, c = sorted(np.argsort(p, kind='stable')[:2].tolist())
    out.append(('off_closure (%d,%d)' % (a, c), _two_pulse_rows(single(p), p, a, c, OFF_S, W)))
    if short:
        return out
    # the same with s = -g: the 1.0 pulse of channel c stays at p_c, so EVERY element is on the plane and the one pair is
    # the only outlier of the table (P - 1 >= h clean pairs for every ALPHA < 1: an exact fit that drops one pair)
    a, c = int(np.argmin(p)), int(np.argmax(p))
    out.append(('off_closure_on_plane (%d,%d)' % (a, c), _two_pulse_rows(single(p), p, a, c, -OFF_G, W)))
    return out


def _two_pulse_rows(rows, p, a, c, s, W):
    assert a != c and p[a] + OFF_G < W and 0 <= p[c] + s and p[c] + s + OFF_G < W
    rows[a] = [(int(p[a]), 1.0), (int(p[a]) + OFF_G, 0.8)]
    rows[c] = [(int(p[c]) + s, 0.8), (int(p[c]) + s + OFF_G, 1.0)]
    return rows


def pulse_trace(tabs, W=W):
    """The tables as one trace (N, nwin * W + 1): window w is samples [w W, (w + 1) W), hop = W."""
    N = len(tabs[0][1])
    x = np.zeros((N, len(tabs) * W + 1))
    for w, (_, rows) in enumerate(tabs):
        for i, pulses in enumerate(rows):
            for pos, amp in pulses:
                x[i, w * W + pos] = amp
    return x


def _full_lag(a, b, W):
    """lag and cmax of one pair of windows from the FP64 full-lag correlation, as the oracle defines them."""
    c = np.correlate(a, b, 'full') / np.sqrt(np.sum(a * a) * np.sum(b * b))
    return (W - 1) - int(np.argmax(c)), float(np.max(c))


def designed_lags(tabs, W=W):
    """-> (lag (nwin, P) int64, cmax (nwin, P)): ``lag_ij = p_j - p_i`` of the 1.0 pulses and ``cmax = 1 / (|a| |b|)``;
    the pair of the two double-pulse channels of an ``off_closure`` row from an FP64 full-lag correlation of those two
    windows."""
    N = len(tabs[0][1])
    pairs = pair_table(N)
    lag = np.zeros((len(tabs), len(pairs)), dtype=np.int64)
    cmax = np.zeros((len(tabs), len(pairs)))
    for w, (_, rows) in enumerate(tabs):
        main = [max(pl, key=lambda t: t[1])[0] for pl in rows]
        nrm = [math.sqrt(sum(a * a for _, a in pl)) for pl in rows]
        double = [i for i, pl in enumerate(rows) if len(pl) > 1]
        for k, (i, j) in enumerate(pairs):
            if i in double and j in double:
                win = pulse_trace([('', [rows[i], rows[j]])], W)[:, :W]
                lag[w, k], cmax[w, k] = _full_lag(win[0], win[1], W)
            else:
                lag[w, k] = main[j] - main[i]
                cmax[w, k] = 1.0 / (nrm[i] * nrm[j])
    return lag, cmax


def off_closure_pairs(lag_row, N):
    """The one pair whose removal leaves a table that closes (``lag_ik = lag_ij + lag_jk`` on every triple i < j < k
    without it): the pair common to ALL triples that do not close -> [] if the row closes, [pair index], or None if no
    single pair (or, with three elements, more than one) accounts for every open triple."""
    idx = {p: k for k, p in enumerate(pair_table(N))}
    common = None
    for i in range(N):
        for j in range(i + 1, N):
            for k in range(j + 1, N):
                trip = (idx[(i, j)], idx[(j, k)], idx[(i, k)])
                if lag_row[trip[2]] != lag_row[trip[0]] + lag_row[trip[1]]:
                    common = set(trip) if common is None else common & set(trip)
    if common is None:
        return []
    return sorted(common) if len(common) == 1 else None


# ---- the oracle's paths ------------------------------------------------------------------------------------------

_lts_cache = {}


def oracle_lts(oracle, lag, xij, alpha, fs=FS):
    """``oracle.fast_lts`` + ``oracle.lts_post_process`` on ``lag / fs`` (lag (nwin, P) integers) -> dict(zraw (2, nwin),
    z (2, nwin), weights (P, nwin), sigma_tau (nwin,), tau (P, nwin)).  Kept per (lags, co-array, ALPHA): the CPU and the
    GPU tests of one session ask for the same tables, and FAST-LTS takes seconds per window on large arrays."""
    lag = np.ascontiguousarray(lag, dtype=np.int64)
    xij = np.ascontiguousarray(xij, dtype=np.float64)
    key = (lag.shape, lag.tobytes(), xij.tobytes(), float(alpha), float(fs))
    got = _lts_cache.get(key)
    if got is None:
        tau = np.ascontiguousarray(lag.T.astype(np.float64) / fs)
        zraw = oracle.fast_lts(tau, xij, alpha)
        z, weights, sig = oracle.lts_post_process(tau, xij, zraw, alpha)
        got = dict(zraw=zraw, z=z, weights=weights, sigma_tau=sig, tau=tau)
        for v in got.values():
            v.flags.writeable = False
        _lts_cache[key] = got
    return got


def classify(oracle, tau, xij, alpha, zraw=None):
    """Which path the oracle takes per window -> list of sets of names.  ``lts_post_process`` restated on the oracle's
    own ``fast_lts`` output (``zraw``; computed here when not given), with the oracle's constants:

    ``mad_zero``            MAD(tau) == 0: FAST-LTS is not run, z and sigma_tau are NaN, the weights all 1
    ``exact_fit``           raw scale < LTS_ZERO_SCALE: weights |r| < LTS_ZERO_SCALE, no re-fit
    ``ordinary``            raw scale >= LTS_ZERO_SCALE, finite raw fit, re-weighted scale > 0
    ``rew_scale_zero``      re-weighted scale exactly 0 (the first-stage weights are kept)
    ``few_kept``            fewer than 3 pairs kept (sigma_tau NaN by definition)
    ``dropped``             some final weight is 0
    ``tie_across_h``        the h-th and (h + 1)-th smallest |r| of FAST-LTS's final fit are EQUAL: the h-subset of the raw
                            scale hangs on the index order
    ``reweight_changed``    the second weighting changed the first stage's weights

    -> (paths, weights (P, nwin) by this restatement)."""
    P, nits = tau.shape
    if zraw is None:
        zraw = oracle.fast_lts(tau, xij, alpha)
    h, rawfac, rewtab = oracle.lts_scale_tables(P, alpha)
    paths = []
    wout = np.ones((P, nits), dtype=np.uint8)
    tmad = np.median(np.abs(tau), axis=0)
    for jj in range(nits):
        tags = set()
        paths.append(tags)
        if tmad[jj] == 0:
            tags.add('mad_zero')
        z0, z1 = zraw[0, jj], zraw[1, jj]
        if not (np.isfinite(z0) and np.isfinite(z1)):
            assert 'mad_zero' in tags, 'window %d: non-finite raw fit with MAD(tau) != 0' % jj
            continue
        assert 'mad_zero' not in tags
        t = tau[:, jj]
        r = (t - xij[:, 0] * z0) - xij[:, 1] * z1
        ar = np.abs(r)
        order = np.argsort(ar, kind='stable')
        if h < P and ar[order[h - 1]] == ar[order[h]]:
            tags.add('tie_across_h')
        ssq = 0.0
        inh = np.zeros(P, dtype=bool)
        inh[order[:h]] = True
        for k in range(P):
            if inh[k]:
                ssq = ssq + r[k] * r[k]
        s0 = math.sqrt(ssq / h) * rawfac
        if abs(s0) < oracle.LTS_ZERO_SCALE:
            tags.add('exact_fit')
            w = ar < oracle.LTS_ZERO_SCALE
        else:
            w1 = np.abs(r / s0) <= oracle.LTS_QUANTILE
            zf0, zf1 = oracle._fit_masked(xij, t, w1)
            rf = (t - xij[:, 0] * float(zf0)) - xij[:, 1] * float(zf1)
            nw = int(np.sum(w1))
            ssw = 0.0
            for k in range(P):
                if w1[k]:
                    ssw = ssw + rf[k] * rf[k]
            scale = math.sqrt(ssw / (nw - 1)) * rewtab[nw] if nw > 1 else 0.0
            w = w1
            if scale > 0:
                tags.add('ordinary')
                w = np.abs(rf / scale) <= oracle.LTS_QUANTILE
                if np.any(w != w1):
                    tags.add('reweight_changed')
            else:
                tags.add('rew_scale_zero')
        if int(np.sum(w)) < 3:
            tags.add('few_kept')
        if not np.all(w):
            tags.add('dropped')
        wout[:, jj] = w
    return paths, wout


# ---- OLS in exact rationals --------------------------------------------------------------------------------------

U = Fraction(1, 2 ** 53)


def gamma(n):
    return n * U / (1 - n * U)


def ols_truth(xij, xpinv, lag_row, fs=FS):
    """One window -> dict(tau (P,) float64 as the kernel forms it, z (2 Fractions), z_bound (2 Fractions))."""
    P = len(lag_row)
    tau = np.array([float(int(v)) / fs for v in lag_row])
    ft = [Fraction(float(v)) for v in tau]
    z, zb = [], []
    for c in range(2):
        terms = [Fraction(float(xpinv[c, k])) * ft[k] for k in range(P)]
        z.append(sum(terms, Fraction(0)))
        zb.append(gamma(P) * sum((abs(v) for v in terms), Fraction(0)))
    return dict(tau=tau, z=z, z_bound=zb)


def ols_acc(xij, tau, z):
    """acc*(z) for a float64 ``z`` (2,) -> (acc* Fraction, E_acc Fraction, E_sigma Fraction), module docstring."""
    P = len(tau)
    z0, z1 = Fraction(float(z[0])), Fraction(float(z[1]))
    acc = Fraction(0)
    tb = Fraction(0)
    for k in range(P):
        t = Fraction(float(tau[k]))
        a, b = Fraction(float(xij[k, 0])) * z0, Fraction(float(xij[k, 1])) * z1
        acc += t * (t - a - b)
        tb += abs(t) * (abs(t) + abs(a) + abs(b))
    e_acc = gamma(P + 3) * tb
    return acc, e_acc, e_acc + gamma(3) * (abs(acc) + e_acc)
