"""The cases of tests/test_gpu_unit_counts.py: every kernel that shares (band or recording row, window) *units* among
its waves, workgroups or XCD ranges, at the unit counts where that share-out changes, on periodic traces that make a
wrong unit anywhere in a pass visible.  CPU only; tests/test_unit_count_cases.py checks here, without a GPU, the premises
every case rests on.

**Share-outs.**  ``SOURCE`` holds the csrc lines that state how a launch deals its units (items per workgroup, waves per
workgroup, the 8 XCD ranges, the workgroup caps) as regular expressions with the values this file assumes; a changed
constant fails the host test instead of quietly un-aiming the GPU test.  The compute-unit count of a persistent grid is
the device's (``hipDeviceAttributeMultiprocessorCount``) and comes in as ``cus``.  ``unit_counts`` lists the counts to
run per kernel; ``*_occupancy`` restate the kernels' index arithmetic by brute force (how many units every workgroup,
wave or XCD range takes), which is what the host test holds the lists against.

**Periodic traces.**  A trace of N channels repeats a base block of ``m * inc`` samples (``m * inc >= W``) and has
``npts = W + (nu - 1) * inc + 1`` samples: ``planner.window_plan`` gives exactly ``nu`` windows and window w holds, byte for
byte, the samples of *template* window ``w mod m``.  The block is ``m`` segments of ``inc`` samples: even segments are
white noise (the arg-max of a pair falls anywhere among the 2W - 1 lags), odd ones a common signal delayed circularly per
channel plus noise.  Recording s of a batch is the base rotated by ``a_s * inc``: its window w is template
``(w + a_s) mod m``.  The first m units are held against the independent references of the suite; every other unit must
equal its template bit for bit.  A share-out bug moves a unit by one of ``distances``; m divides none of them
(``choose_m``), so the unit it lands on holds another template.  With an odd ``inc`` the 16-byte alignment of a window
alternates, and the quantiser and the DMA verifier take another code path per parity (another summation order): m is
even there, so a window and its template share the alignment class.  The cases whose templates are solved against the
oracle draw their block with ``solve_seed``: the first seed at which the oracle's sampled confidence intervals lie within
half their tolerance of its closed form (as tests/lts_h_cases.py chooses its noisy traces)."""
import functools
import os
import re

import numpy as np

from narrow_band_least_squares_amd import _hip, planner

from test_gpu_routes import GAP, _reference as reference      # the FFT + long-double reference, as it stands  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'narrow_band_least_squares_amd', 'csrc')

FS = 20.0
T0 = 17884.0729166667
XCDS = 8

# (name, file, regular expression, the captured values this file assumes)
SOURCE = (
    ('xcd_item', 'xcorr_screen.hip', r'const int xcd = block & (\d+), slot = block >> (\d+);', (7, 3)),
    ('xcd_share', 'xcorr_screen.hip', r'const int share = \(total \+ (\d+)\) >> (\d+);', (7, 3)),
    ('xcd_grid', 'xcorr_screen.hip', r'return (\d+) \* \(\(share \+ per_block - 1\) / per_block\);', (8,)),
    ('quant_lds_waves', 'xcorr_screen.hip', r'xcd_item\(blockIdx\.x, blockDim\.x >> (\d+), wv, a\.nu \* N\)', (6,)),
    ('quant_reg_waves', 'xcorr_screen.hip', r'xcd_item\(blockIdx\.x, (\d+), wv, a\.nu \* N\)', (4,)),
    ('quant_grid', 'xcorr_screen.hip', r'const dim3 qgrid\(xcd_grid\(r\.quant_waves, a\.nu \* N\)\);', ()),
    ('screen_unit', 'xcorr_screen.hip', r'const int ul = grp \* (\d+) \+ \(rem & (\d+)\);', (8, 7)),
    ('screen_grid', 'xcorr_screen.hip', r'const int ngrp = \(a\.nu \+ (\d+)\) / (\d+);', (7, 8)),
    ('dma_xcd', 'xcorr_screen.hip', r'const int xcd = blockIdx\.x & (\d+), nslot = gridDim\.x >> (\d+);', (7, 3)),
    ('dma_share', 'xcorr_screen.hip', r'const int share = \(a\.nu \+ (\d+)\) >> (\d+);', (7, 3)),
    ('dma_per_xcd', 'xcorr_screen.hip', r'const int per_xcd = h->num_cus > 0 \? \(h->num_cus \+ (\d+)\) / (\d+) : 32;', (7, 8)),
    ('dma_grid', 'xcorr_screen.hip', r'verify_dma_kernel, dim3\((\d+) \* \(share < per_xcd \? share : per_xcd\)\), dim3\((\d+)\)', (8, 1024)),
    ('dma_prefetch', 'xcorr_screen.hip', r'vmeta_load\(a, xcd, share, slot \+ (\d+) \* nslot, vz\);  // unit k\+(\d+)', (2, 3)),
    ('dma_buffers', 'xcorr_screen.hip', r'VERIFY_QUEUE\(mn, cur \^ (\d+)\)', (1,)),
    ('verify_lds', 'xcorr_screen.hip', r'const int ul = xcd_item\(blockIdx\.x, (\d+), (\d+), a\.nu\);', (1, 0)),
    ('verify_lds_grid', 'xcorr_screen.hip', r'verify_lds_kernel, dim3\(xcd_grid\((\d+), a\.nu\)\)', (1,)),
    ('verify_item', 'xcorr_screen.hip', r'const int item = blockIdx\.x \* (\d+) \+ \(threadIdx\.x >> 6\);', (4,)),
    ('verify_grid', 'xcorr_screen.hip', r'verify_kernel, dim3\(\(a\.nu \* h->npairs \+ (\d+)\) / (\d+)\), dim3\((\d+)\)', (3, 4, 256)),
    ('range_item', 'lag_pick.h', r'const int64_t item = \(int64_t\)blockIdx\.x \* (\d+) \+ \(threadIdx\.x >> 6\);', (4,)),
    ('bounded_grid', 'xcorr_bounded.hip', r'xcorr_bounded_simple_kernel, dim3\(\(unsigned\)\(\(a\.nitems \+ (\d+)\) / (\d+)\)\), dim3\((\d+)\)', (3, 4, 256)),
    ('seeded_grid', 'xcorr_seeded.hip', r'xcorr_seeded_simple_kernel, dim3\(\(unsigned\)\(\(a\.nitems \+ (\d+)\) / (\d+)\)\), dim3\((\d+)\)', (3, 4, 256)),
    ('lts_wave_unit', 'solve.hip', r'const int u = a\.u0 \+ blockIdx\.x \* (\d+) \+ wv;', (4,)),
    ('lts_wave_grid', 'solve.hip', r'solve_lts_wave_kernel<PT, H>\), dim3\(\(nunits \+ (\d+)\) / (\d+)\), dim3\((\d+)\)', (3, 4, 256)),
    ('ols_unit', 'solve.hip', r'const int ul = blockIdx\.x \* (\d+) \+ threadIdx\.x;', (64,)),
    ('ols_grid', 'solve.hip', r'solve_ols_kernel, dim3\(\(nunits \+ (\d+)\) / (\d+)\), dim3\((\d+)\)', (63, 64, 64)),
    ('uncert_grid', 'solve.hip', r'uncertainty_kernel, dim3\(\(unsigned\)\(\(nu \+ (\d+)\) / (\d+)\)\), dim3\((\d+)\)', (63, 64, 64)),
    ('pack_grid', 'solve.hip', r'pack_weights_kernel, dim3\(\(unsigned\)\(\(items \+ (\d+)\) / (\d+)\)\), dim3\((\d+)\)', (255, 256, 256)),
    ('gather_waves', 'solve.hip', r'constexpr int GATHER_WAVES = (\d+);', (4,)),
    ('gather_cap', 'solve.hip', r'const int64_t cap = \(int64_t\)\(h->num_cus > 0 \? h->num_cus : 256\) \* (\d+);', (8,)),
    ('gather_stride', 'solve.hip', r'base < nunits; base \+= gridDim\.x \* GATHER_WAVES\)', ()),
    ('kept_waves', 'kept.hip', r'constexpr int KEPT_WAVES = (\d+);', (4,)),
    ('kept_lanes', 'kept.hip', r'const int S = a\.N <= (\d+) \? (\d+) : \(a\.N <= (\d+) \? (\d+) : (\d+)\);', (8, 8, 16, 16, 32)),
    ('kept_per_wg', 'kept.hip', r'const int64_t per_wg = \(int64_t\)KEPT_WAVES \* \((\d+) / S\);', (64,)),
    ('closure_waves', 'closure.hip', r'constexpr int CLOSURE_WAVES = (\d+);', (4,)),
    ('closure_unit', 'closure.hip', r'const int ul = blockIdx\.x \* CLOSURE_WAVES \+ wave;', ()),
    ('beam_waves', 'beam.hip', r'constexpr int BEAM_WAVES = (\d+);', (4,)),
    ('beam_wave_w', 'beam.hip', r'constexpr int BEAM_WAVE_W = (\d+);', (512,)),
    ('beam_unit', 'beam.hip', r'const int base = blockIdx\.x \* BEAM_WAVES;', ()),
    ('batch_floor', 'xcorr_screen.hip', r'if \(bw < (\d+)\) bw = (\d+);', (64, 64)),
    ('batch_equal', 'xcorr_screen.hip', r'const int64_t eq = \(\(U \+ nb_ - 1\) / nb_ \+ (\d+)\) / (\d+) \* (\d+);', (7, 8, 8)),
    ('batch_bytes', 'xcorr_screen.hip', r'int64_t bw = \(int64_t\)\(batch_mb << 20\) / \(\(int64_t\)N \* (\d+) \* a\.WP\);', (2,)),
)

BEAM_WAVE_W = 512        # beam.hip: windows up to this length are summed by one wave per unit
QUANT_WAVES_MAX = 4
GATHER_WAVES, GATHER_CAP = 4, 8
SCREEN_GROUP = 8


def scrape():
    """-> {name: tuple of the integers the expression captures}; AssertionError where a line is gone or its copies in the
    file disagree."""
    out, text = {}, {}
    for name, fn, rx, _ in SOURCE:
        if fn not in text:
            with open(os.path.join(CSRC, fn)) as f:
                text[fn] = f.read()
        found = [mt.groups() for mt in re.finditer(rx, text[fn])]
        assert found and len(set(found)) == 1, '%s: %d matches of %r in %s: %s' % (name, len(found), rx, fn, sorted(set(found)))
        out[name] = tuple(int(v) for v in found[0])
    return out


def ceil_div(a, b):
    return -(-a // b)


def per_xcd(cus):
    """Workgroups of the persistent verifier per XCD: c = ceil(cus / 8)."""
    return ceil_div(cus, XCDS)


# ---- the counts ----------------------------------------------------------------------------------------------------------
def stride_counts(s):
    """A kernel with s units per workgroup or wave: 1, s - 1, s, s + 1 and 2 s + 1."""
    return sorted({n for n in (1, s - 1, s, s + 1, 2 * s + 1) if n >= 1})


def kept_lanes(N):
    return 8 if N <= 8 else (16 if N <= 16 else 32)


def unit_counts(kernel, cus=256, N=1, waves=1, mask_bytes=1):
    """The unit counts to run for ``kernel`` on a device of ``cus`` compute units."""
    c = per_xcd(cus)
    if kernel == 'verify_dma':
        return sorted({1, 2, 7, 8, 9, 17, 8 * c - 1, 8 * c, 8 * c + 1, 8 * c + 9, 16 * c - 1, 16 * c + 1, 24 * c + 1, 32 * c - 7})
    if kernel == 'xcd_item':
        # item totals 1, 7, 8, 9, 8 k +- 1; with ``waves`` per workgroup also around 8 * waves (a share of one full
        # workgroup) and 16 * waves + 1.  A unit is N items: the smallest count that reaches the total.
        totals = {1, 7, 8, 9, 15, 17}
        if waves > 1:
            totals |= {8 * waves - 1, 8 * waves, 8 * waves + 1, 16 * waves + 1}
        out = {ceil_div(t, N) for t in totals}
        if waves > 1 and all(ceil_div(n * N, XCDS) % waves == 0 for n in out):
            out.add(next(n for n in range(1, 64) if ceil_div(n * N, XCDS) % waves))
        return sorted(out)
    if kernel == 'screen':
        return stride_counts(SCREEN_GROUP)
    if kernel in ('verify_glob', 'range_pick'):                       # 4 (unit, pair) items per workgroup
        return [1, 2, 3, 5]
    if kernel == 'solve_lts_wave':
        return sorted(set(stride_counts(4)) | {2})
    if kernel in ('solve_ols', 'uncertainty'):
        return stride_counts(64)
    if kernel == 'pack_weights':
        return sorted({255 // mask_bytes, ceil_div(256, mask_bytes), ceil_div(257, mask_bytes)})
    if kernel == 'gather_pairs':
        trip = GATHER_WAVES * GATHER_CAP * cus
        return sorted(set(stride_counts(GATHER_WAVES)) - {9} | {trip - 1, trip, trip + 1, 2 * trip + 1})
    if kernel == 'kept_elements':
        upw = 64 // kept_lanes(N)
        return sorted({n for s in (upw, 4 * upw) for n in (s - 1, s, s + 1) if n >= 1})
    if kernel in ('closure', 'beam_fstat'):
        return stride_counts(4)
    raise KeyError(kernel)


# ---- the index arithmetic, restated ----------------------------------------------------------------------------------
def xcd_item(block, per_block, sub, total):
    xcd, slot = block & 7, block >> 3
    share = (total + 7) >> 3
    it = xcd * share + slot * per_block + sub
    return it if (slot * per_block + sub < share and it < total) else -1


def xcd_grid(per_block, total):
    return 8 * ceil_div((total + 7) >> 3, per_block)


def xcd_occupancy(total, per_block):
    """-> (live waves of every workgroup, items of every XCD range); every item is taken exactly once."""
    grid = xcd_grid(per_block, total)
    items = [[xcd_item(b, per_block, s, total) for s in range(per_block)] for b in range(grid)]
    flat = sorted(i for row in items for i in row if i >= 0)
    assert flat == list(range(total)), 'xcd_item does not deal %d items once each' % total
    per_range = [0] * XCDS
    for b, row in enumerate(items):
        per_range[b & 7] += sum(i >= 0 for i in row)
    return [sum(i >= 0 for i in row) for row in items], per_range


def dma_occupancy(nu, cus):
    """verify_dma_kernel -> [XCD][slot] the units the persistent workgroup walks (slot, slot + nslot, ... of its range)."""
    share = (nu + 7) >> 3
    nslot = min(share, per_xcd(cus))
    out, seen = [], []
    for xcd in range(XCDS):
        row = []
        for slot0 in range(nslot):
            units, slot = [], slot0
            while slot < share and xcd * share + slot < nu:
                units.append(xcd * share + slot)
                slot += nslot
            row.append(len(units))
            seen += units
        out.append(row)
    assert sorted(seen) == list(range(nu)), 'the persistent walk does not take %d units once each' % nu
    return out


def dma_patterns(nu, cus):
    """What a launch of nu units exercises: ('walk', k) a workgroup walking k units (0..), ('ragged', k) one XCD whose
    workgroups walk k and k - 1, 'short' / 'empty' a last XCD range short of the share / with no unit."""
    occ = dma_occupancy(nu, cus)
    share = (nu + 7) >> 3
    pats = set()
    for row in occ:
        for k in set(row):
            pats.add(('walk', k))
        if len(set(row)) > 1:
            assert max(row) - min(row) == 1
            pats.add(('ragged', max(row)))
        tot = sum(row)
        if tot == 0:
            pats.add('empty')
        elif tot < share:
            pats.add('short')
    return pats


def group_occupancy(nu, per_wg):
    """Consecutive units, ``per_wg`` per workgroup -> live units of every workgroup."""
    return [min(per_wg, nu - b * per_wg) for b in range(ceil_div(nu, per_wg))]


def gather_occupancy(nu, cus):
    """gather_pairs_kernel -> per workgroup the live waves of each of its grid-stride trips."""
    grid = min(ceil_div(nu, GATHER_WAVES), GATHER_CAP * cus)
    out, seen = [], 0
    for b in range(grid):
        trips, base = [], b * GATHER_WAVES
        while base < nu:
            trips.append(min(GATHER_WAVES, nu - base))
            base += grid * GATHER_WAVES
        seen += sum(trips)
        out.append(tuple(trips))
    assert seen == nu
    return out


def screen_batches(nu, N, WP, batch_mb, buffer_units=1 << 40):
    """The screening unit batches of nu units (nbls_launch_xcorr_screen_range) -> list of batch sizes."""
    bw = max(64, (batch_mb << 20) // (N * 2 * WP))
    batch = min(buffer_units, bw)
    if batch > nu:
        batch = max(nu, 1)
    if nu > batch:
        nb = ceil_div(nu, batch)
        batch = min(batch, ceil_div(ceil_div(nu, nb), 8) * 8)
    return [min(batch, nu - u0) for u0 in range(0, nu, batch)]


# ---- m ---------------------------------------------------------------------------------------------------------------
def distances(nu, N, cus):
    """The distances (in units) by which a share-out bug could move a unit."""
    c = per_xcd(cus)
    return sorted({1, 2, 4, 8, 16, 32, 64, 256, c, 8 * c, 8 * cus, 32 * cus, ceil_div(nu, 8), ceil_div(nu * N, 8)})


def choose_m(nu, N, cus, inc):
    """7, or 9 where this case's XCD share is a multiple of 7 (then 11, 13); twice that with an odd hop."""
    for m in (7, 9, 11, 13):
        if all(d % m for d in distances(nu, N, cus)):
            return m if inc % 2 == 0 else 2 * m
    raise AssertionError('no m for nu=%d N=%d cus=%d' % (nu, N, cus))


# ---- traces ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def base_block(N, W, inc, m, seed=0):
    """(N, m * inc): m segments of inc samples; even ones white noise, odd ones a common signal delayed circularly by
    channel plus noise."""
    assert m * inc >= W
    rng = np.random.default_rng(77000 + 1000 * N + 10 * W + inc + 100000 * m + seed)
    x = np.empty((N, m * inc))
    for j in range(m):
        seg = rng.standard_normal((N, inc))
        if j % 2:
            common = rng.standard_normal(inc)
            for ch in range(N):
                seg[ch] = np.roll(common, (ch * (j + 2)) % max(1, inc // 2) - inc // 4) + seg[ch]      # (another delay pattern per segment)
        x[:, j * inc:(j + 1) * inc] = seg
    x.flags.writeable = False
    return x


def npts_of(W, inc, nu):
    return W + (nu - 1) * inc + 1


def winlen(W):
    return (W + 0.5) / FS


def overlap(W, inc):
    return 1.0 - inc / float(W)


def trace(N, W, inc, m, nu, rot=0, seed=0):
    """-> (N, npts) whose window w (start w * inc) is template (w + rot) mod m."""
    base = base_block(N, W, inc, m, seed)
    npts = npts_of(W, inc, nu)
    x = np.roll(base, -rot * inc, axis=1)
    x = np.ascontiguousarray(np.tile(x, (1, ceil_div(npts, x.shape[1])))[:, :npts])
    assert planner.window_plan(npts, FS, winlen(W), overlap(W, inc)) == (W, inc, nu), (W, inc, nu)
    return x


@functools.lru_cache(maxsize=None)
def templates(N, W, inc, m, seed=0):
    """The m template windows side by side, hop W: (N, m * W) — the layout ``reference`` reads."""
    base = base_block(N, W, inc, m, seed)
    ext = np.tile(base, (1, 2 + W // base.shape[1]))
    t = np.ascontiguousarray(np.concatenate([ext[:, k * inc:k * inc + W] for k in range(m)], axis=1))
    t.flags.writeable = False
    return t


@functools.lru_cache(maxsize=None)
def template_reference(N, W, inc, m, seed=0):
    """-> lag (m, P), cmax (m, P) of the templates (``reference`` asserts the gap of every pair's best lag)."""
    lag, cmax = reference(templates(N, W, inc, m, seed), W, m, planner.pair_table(N))
    lag.flags.writeable = False
    cmax.flags.writeable = False
    return lag, cmax


def template_gaps(N, W, inc, m, seed=0):
    """Of every template and pair: (best - second best) / (|a| |b|) over all 2W - 1 lags, long double."""
    t = templates(N, W, inc, m, seed).astype(np.longdouble)
    pairs = planner.pair_table(N)
    gaps = np.empty((m, len(pairs)))
    for k in range(m):
        seg = t[:, k * W:(k + 1) * W]
        for p, (i, j) in enumerate(pairs):
            c = np.sort(np.correlate(seg[i], seg[j], 'full'))
            gaps[k, p] = float((c[-1] - c[-2]) / np.sqrt(np.sum(seg[i] ** 2) * np.sum(seg[j] ** 2)))
    return gaps


def geometry(N):
    from narrow_band_least_squares_amd import synthetic
    rij = synthetic.array_geometry(N, 1.0, seed=N)
    return rij - rij.mean(axis=1, keepdims=True)


def sampler_gap(N, W, inc, m, alpha, seed):
    """The templates' solve through the oracle alone (their lags: ``template_reference``) -> the worst distance between the
    oracle's sampled and closed-form confidence intervals, in units of the tolerance ``test_gpu_solve._check_against_oracle``
    has for the sampled ones (tests/lts_h_cases.py: sampler_gap).  An ellipse that passes the origin closely is sampled too
    coarsely by 20 000 points: a property of the reference, decided here on the CPU."""
    import nbls_oracle as oracle
    import solve_truth as st
    from lts_h_cases import sampler_gap as gap
    lag, _ = template_reference(N, W, inc, m, seed)
    xij = planner.co_array(geometry(N))[0]
    if alpha < 1.0:
        r = st.oracle_lts(oracle, lag, xij, alpha, FS)
        z, sig = r['z'], r['sigma_tau']
    else:
        z, _, _, sig = oracle.ols_solve(xij, np.ascontiguousarray(lag.T / FS))
    g = np.concatenate(gap(oracle, xij, z, sig))
    return float(np.nanmax(g)) if np.any(np.isfinite(g)) else 0.0


@functools.lru_cache(maxsize=None)
def solve_seed(N, W, inc, m, alpha):
    """The first seed whose templates the sampled confidence intervals can judge: gap at most half the tolerance."""
    for seed in range(32):
        if sampler_gap(N, W, inc, m, alpha, seed) <= 0.5:
            return seed
    raise AssertionError('no seed for N=%d W=%d inc=%d m=%d alpha=%g' % (N, W, inc, m, alpha))


# ---- shapes ----------------------------------------------------------------------------------------------------------
def first_window(N, want, W0=64, W1=13000, vrows=1):
    """The shortest window length in W0..W1 whose route has the fields ``want`` (host only: nbls_route_table)."""
    t = _hip.route_table(N, W0, W1, vrows=vrows)
    ok = np.ones(len(t), dtype=bool)
    for k, v in want.items():
        ok &= t[k] == v
    assert ok.any(), 'no window of %d elements with %s' % (N, want)
    return W0 + int(np.argmax(ok))


def hop_for(W, m=7, even=True):
    """The smallest hop with m * inc >= W of the wanted parity (at least 4 samples)."""
    inc = max(4, ceil_div(W, m))
    return inc + (inc % 2 if even else 1 - inc % 2)


# correlation shapes by the route they are named for: N, W, and the route fields the shape was chosen for
def correlation_shapes():
    short = first_window(3, dict(correlator=_hip.ROUTE_SCREEN, verifier=1))
    return {
        'dma_short': dict(N=3, W=short, expect=dict(verifier=1)),
        'dma': dict(N=3, W=600, expect=dict(verifier=1)),
        'dma8': dict(N=8, W=600, expect=dict(verifier=1)),
        'lds': dict(N=9, W=300, expect=dict(verifier=2)),
        'glob': dict(N=3, W=6742, expect=dict(verifier=3)),
    }


QUANT_INSTANCES = ((2, 4), (3, 4), (4, 4), (6, 4), (8, 4), (1, 3), (1, 2), (1, 1))     # (quant_inst, quant_waves), 3 elements


def quantiser_shapes(N=3):
    """One window length per reachable (quant_inst, quant_waves): the shortest that takes it."""
    t = _hip.route_table(N, 64, 13000)
    seen = sorted({(int(r['quant_inst']), int(r['quant_waves'])) for r in t if r['correlator'] == _hip.ROUTE_SCREEN})
    assert seen == sorted(QUANT_INSTANCES), seen
    return [(qi, qw, first_window(N, dict(correlator=_hip.ROUTE_SCREEN, quant_inst=qi, quant_waves=qw))) for qi, qw in QUANT_INSTANCES]
