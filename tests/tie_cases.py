"""The cases of tests/test_gpu_ties.py: integer traces that control what the int8 screening of csrc/xcorr_screen.hip
leaves in its candidate records — how many lags a record lists, which lane's slots they fill, which direction of a pair
holds them, where the true maximum sits among lags the screening cannot tell apart — with the designed records and the
exact reference.  CPU only; tests/test_tie_cases.py checks here, without a GPU, the premises every case rests on.

**Integer traces.**  A window holds, per channel, a few pulses of about A = 2^20 and zeros (the randomised family adds
integer noise of +-2^10).  Every product and partial sum of a correlation is an integer far below 2^53: FP64 is exact in
any summation order, with or without FMA.  The reference is ``np.correlate`` on int64, divided by the oracle's norm
BEFORE the first maximum is taken.  Exact ties are legitimate here; NumPy's first-index rule decides them.

**Channels.**  Channel 0 is the *profile*, channel 1 the *probe* (one pulse A at sample P), channels 2.. are further
probes (A/2 at P, A at a sample of their own).  ``np.correlate(profile, probe)`` is A times the profile shifted by P: a
design is a table {signed lag s: pulse value}, the profile holds the value at sample P + s, and index W - 1 + s of pair
(0, 1) is A times that value.  Lags s >= 0 are in the record of the ordered pair (0 slides over 1: sliding index below
its partner), lags s <= 0 in that of (1 over 0).  Window 1 of every case holds the mirrored table {-s: value} unless the
case names its own: both mirrorings of every design are run.  A direction the table leaves empty gets a half-amplitude
pulse at lag 0, and the further probes overlap every other channel at lag 0, so no record overflows merely because its
direction holds nothing.

**What the screening sees.**  The quantiser scales a channel by its max |x| to |q| <= 16256: pulses of 2^20 - 1, 2^20 and
2^20 + 1 all become 16256 and tie in the screening values I', a pulse of A/2 or a stair of A k/8 lies far below the
maximum less theta.  ``model_records`` evaluates the kernel's I' (three limb products recombined in f32) and theta in
NumPy for every ordered pair; the candidates of a record are the exact maxima of I' of its direction — test_tie_cases.py
asserts that nothing else comes within 2 theta of them.  (These windows are flat — zero at almost every lag — so a wave
that finishes a lag group before any maximum is published sees every lag of it tied at 0 and absorbs the surplus into its
interval; the designed flags hold because the merge filters that interval, like the slots, against the final maximum.)

**Lanes.**  Lag d >= 0 of an ordered pair is d = p span + t step + 16 s + 4 g + r (step = 16 S, span = TBV step, t < TBV,
r < 4): one lane sees, of lag group p, the lags whose d mod step falls in one aligned block of four.  A lane has
NSLOT = 6 slots, a record lists KOUT = 26 lags.  The first ``nw`` groups go to one wave each; later ones are dealt
dynamically, so designs that count on distinct lanes keep below group ``nw`` (``lane_loads``).

Constants the library does not export are stated below; test_tie_cases.py holds the source to them."""
import collections
import os

import numpy as np

from narrow_band_least_squares_amd import _hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'narrow_band_least_squares_amd', 'csrc')

QMAX = 16256             # xcorr_screen.hip   constexpr int QMAX = 16256;
KOUT = 26                # xcorr_screen.hip   constexpr int KOUT = 26;
NSLOT = 6                # xcorr_screen.hip   constexpr int NSLOT = 6;
CHDR = 6                 # xcorr_screen.hip   constexpr int CHDR = 6;
STATED = (('xcorr_screen.hip', r'constexpr int QMAX = (\d+);', QMAX),
          ('xcorr_screen.hip', r'constexpr int KOUT = (\d+);', KOUT),
          ('xcorr_screen.hip', r'constexpr int NSLOT = (\d+);', NSLOT),
          ('xcorr_screen.hip', r'constexpr int CHDR = (\d+);', CHDR),
          ('xcorr_screen.hip', r'const int dlane = D0 \+ (\d+) \* s \+ 4 \* g;', 16),
          ('xcorr_screen.hip', r'const int step = (\d+) \* S;', 16),
          ('xcorr_screen.hip', r'const int D0 = TBV \* p \* (step);', 'step'),
          ('xcorr_screen.hip', r'sinst == 3 \? \(const void\*\)screen_kernel<(\d+), 8>', 8),
          ('xcorr_screen.hip', r'const int nw = nwaves / (NSL);', 'NSL'),
          ('xcorr_screen.hip', r'dim3\((\d+)\), lds, h->stream, a\);', 512))
# the kernel's threshold, as test_tie_cases.py finds it in the source and ``theta_model`` evaluates it
THETA_SOURCE = ('theta = (float)(((mi[1] + mj[1]) * 1.001 + 0.5 * (double)W + 8.0 + 2.0 * lolo) * 1.0001 + 1.0e-6 * iabs);',
                '? (double)QMAX * (double)QMAX * sqrt(mi[0] * mj[0]) / (mi[2] * mj[2]) : 0.0;',
                'const double lolo = sqrt(mi[3] * mj[3]);')

A = 1 << 20              # the pulse every tie is made of
HALF = A >> 1            # a decoy: far below the maximum less theta
NOISE = 1 << 10          # the randomised family: uniform integer background in [-NOISE, NOISE]
WAVES = 8                # waves of a screening workgroup (512 threads)

Geom = collections.namedtuple('Geom', 'N W S TBV step span nw flags route')
OPTION_FLAGS = {'screen_nc4': _hip.ROUTE_OPT_NC4, 'screen_nsl1': _hip.ROUTE_OPT_NSL1, 'screen_tb8': _hip.ROUTE_OPT_TB8}

# The routes of test_gpu_ties.py: the smallest shapes that reach each verifier, screening instance and layout
# (``expect``: the route fields the shape was chosen for; test_tie_cases.py asserts them on the host).
ROUTES = {
    'dma': dict(N=3, W=600, opts=(), expect=dict(verifier=1, screen_inst=1, nsl=2)),        # persistent DMA verifier: the default route
    'lds': dict(N=9, W=300, opts=(), expect=dict(verifier=2, screen_inst=1, S=2)),          # LDS verifier, two lag blocks per tile step
    'glob': dict(N=3, W=6742, opts=(), expect=dict(verifier=3, nsl=1)),                     # global-memory verifier (run form): N W 8 > 158 KB
    'nc4': dict(N=3, W=600, opts=('screen_nc4',), expect=dict(screen_inst=2, ncopy=4)),     # four-copy instance
    'tb8': dict(N=17, W=300, opts=('screen_tb8',), expect=dict(screen_inst=3, S=1)),        # eight-tile instance
    'nsl1': dict(N=3, W=600, opts=('screen_nsl1',), expect=dict(screen_inst=1, nsl=1)),     # one sliding channel per workgroup
    'static': dict(N=3, W=600, opts=('screen_static', 'screen_pretest'), expect=dict(screen_inst=1, nsl=2)),
    'npg': dict(N=18, W=300, opts=(), expect=dict(G=16, S=1)),                              # two partner groups (17 partners)
    'seg': dict(N=3, W=600, opts=(), nseg=3, expect=dict(verifier=1)),                      # three recordings in one pass
}


def npts_of(W):
    return 2 * W + 1


def geometry(N, W, opts=(), vrows=1):
    """The screening geometry of windows of W samples of N elements under the options ``opts`` (host only)."""
    flags = 0
    for o in opts:
        flags |= OPTION_FLAGS.get(o, 0)
    r = _hip.route(N, W, vrows=vrows, npts_pad=(npts_of(W) + 63) // 64 * 64, flags=flags)
    assert r['correlator'] == _hip.ROUTE_SCREEN and r['impl'] == 3, 'N=%d W=%d does not screen: %s' % (N, W, r)
    S, TBV = r['S'], 8 if r['screen_inst'] == 3 else 4
    return Geom(N, W, S, TBV, 16 * S, TBV * 16 * S, WAVES // r['nsl'], flags, r)


def route_geometry(name, W=None):
    r = ROUTES[name]
    return geometry(r['N'], r['W'] if W is None else W, r['opts'], r.get('nseg', 1))


def end_windows(name):
    """Window lengths with W mod span in {0, 1, step - 1, step, step + 1}: the mask against the window end never runs,
    runs in a group that holds one lag, in a tile short of one lag, in an exactly full tile, in a tile of one lag."""
    g = route_geometry(name)
    k = -(-max(2 * g.step, 65) // g.span)
    return [k * g.span + r for r in (0, 1, g.step - 1, g.step, g.step + 1)]


# ---- lags by lane ------------------------------------------------------------------------------------------------------
def lane_of(d, S, TBV):
    step = 16 * S
    return d // (TBV * step), (d % step) // 4


def lane_loads(lags, S, TBV, nw):
    """Of lags d >= 0: (the most that certainly share one lane, the most that may).  Groups below ``nw`` run on a wave of
    their own; a later group may follow any of them on the same wave."""
    lags = list(lags)
    if not lags:
        return 0, 0
    sure = max(collections.Counter(lane_of(d, S, TBV) for d in lags).values())
    if all(lane_of(d, S, TBV)[0] < nw for d in lags):
        return sure, sure
    return sure, max(collections.Counter(lane_of(d, S, TBV)[1] for d in lags).values())


def spread(m, W, S, TBV, start=1, stride=3, nw=4):
    """m lags, ``stride`` apart where the lanes allow, no more than NSLOT of them in any lane, all below group ``nw``."""
    out, load = [], collections.Counter()
    for d in range(start, min(W, nw * TBV * 16 * S), stride):
        if load[lane_of(d, S, TBV)] < NSLOT:
            load[lane_of(d, S, TBV)] += 1
            out.append(d)
            if len(out) == m:
                return out
    raise AssertionError('no %d spread lags in windows of %d samples (S=%d TBV=%d)' % (m, W, S, TBV))


def one_lane(k, W, S, TBV, p=0, block=1):
    """The first k lags of the lane (group p, block) in the order the epilogue walks them: tile t, then register r."""
    step = 16 * S
    out = [p * TBV * step + t * step + 4 * block + r for t in range(TBV) for r in range(4)][:k]
    assert len(out) == k and out[-1] < W
    return out


# ---- cases -------------------------------------------------------------------------------------------------------------
class Case:
    """``tables``: one {signed lag: pulse value} per window.  ``ties``: per window the signed lags designed to tie in the
    screening.  ``kind``: 'spread' (no lane holds more than NSLOT), 'lane' (the ties of a direction share one lane),
    None.  ``seed``: integer background noise (records are then only checked for soundness)."""

    def __init__(self, family, name, table, ties=None, kind=None, second=None, second_ties=None, seed=None):
        self.family, self.name, self.kind, self.seed = family, name, kind, seed
        ties = sorted(table) if ties is None else sorted(ties)
        if second is None:
            second, second_ties = {-s: v for s, v in table.items()}, [-s for s in ties]
        self.tables = (dict(table), dict(second))
        self.ties = (ties, sorted(sorted(second) if second_ties is None else second_ties))

    def __repr__(self):
        return '%s/%s' % (self.family, self.name)


def _flat(lags, v=A):
    return {int(d): v for d in lags}


def list_length(W, S, TBV, ms=(1, 2, 6, 7, 25, 26, 27, 40, 64)):
    """m exact ties, no lane more than six: count m, no flag, the list is the designed set up to 26; flag 2 from 27."""
    return [Case('list', 'm%d' % m, _flat(spread(m, W, S, TBV)), kind='spread') for m in ms]


def lane_slots(W, S, TBV, ks=(6, 7, 8, 16)):
    """k ties in one lane of one group: six fill its slots, the rest is absorbed into the interval (flag 1)."""
    return [Case('lane', 'k%d' % k, _flat(one_lane(k, W, S, TBV)), kind='lane') for k in ks]


def stale_slots(W, S, TBV):
    """Stairs A k/8 (each more than theta above the last) and seven ties at the top.  In one lane, rising and falling;
    stairs in group 0 and the ties in group 1, where another wave finds the maximum: the slots the first wave filled
    are filtered against the final maximum at the merge."""
    lane = one_lane(14, W, S, TBV)
    stairs = [A * k // 8 for k in range(1, 8)]
    up = dict(zip(lane, stairs + [A] * 7))
    down = dict(zip(lane, [A] * 7 + stairs[::-1]))
    cases = [Case('stale', 'rising', up, ties=lane[7:], kind='lane'), Case('stale', 'falling', down, ties=lane[:7], kind='lane')]
    # (a short last group: the seven ties take the lags it has, block by block)
    span = TBV * 16 * S
    later = [d for b in range(1, 4 * S) for d in one_lane(4 * TBV, 2 * span, S, TBV, p=1, block=b) if d < W][:7]
    assert len(later) == 7
    split = dict(zip(lane[:7], stairs))
    split.update(_flat(later))
    cases.append(Case('stale', 'ties_in_a_later_group', split, ties=later))
    return cases


def stale_across_groups(W, S, TBV, nw):
    """Six equal pulses in the same block of EVERY lag group, each group's level above the last one's by more than theta
    (rising), or below it (falling).  There are more groups than waves: whichever wave takes a second group finds its six
    slots filled by the earlier one — rising, they are stale and must all be reused (a slot wrongly kept sends a tie to
    the interval: flag 1, where the design expects none)."""
    span = TBV * 16 * S
    groups = min(W // span, 14)
    assert groups > nw
    levels = [A * (16 - groups + 1 + p) // 16 for p in range(groups)]
    cases = []
    for name, lv in (('rising', levels), ('falling', levels[::-1])):
        table, top = {}, []
        for p in range(groups):
            lags = one_lane(6, W, S, TBV, p=p, block=2)
            table.update({d: lv[p] for d in lags})
            if lv[p] == A:
                top = lags
        cases.append(Case('regroup', name, table, ties=top, kind='lane'))
    return cases


def true_maximum(W, S, TBV):
    """One pulse of 2^20 + 1 among equal 2^20 (it must win wherever it sits), one of 2^20 - 1 among them (the first of
    the equal ones must win): all tie in the screening, only the FP64 verifier can tell them apart."""
    cases = []
    five = spread(5, W, S, TBV, start=2, stride=7)
    lane = one_lane(8, W, S, TBV)
    other = [-d for d in spread(3, W, S, TBV, start=3, stride=5)]
    for tag, special in (('plus', A + 1), ('minus', A - 1)):
        for pos, idx in (('first', 0), ('last', -1)):
            t = _flat(five)
            t[five[idx]] = special
            cases.append(Case('truth', '%s_%s' % (tag, pos), t, kind='spread'))
        t = _flat(lane)
        t[lane[7]] = special                              # the eighth of a lane: in the interval, not in the list
        cases.append(Case('truth', '%s_absorbed' % tag, t, kind='lane'))
        if tag == 'minus':                                # ... and the first of the equal ones is the absorbed one
            t = _flat(lane, A - 1)
            t[lane[6]] = t[lane[7]] = A
            cases.append(Case('truth', 'minus_all_but_the_absorbed', t, kind='lane'))
        for m in (27, 64):                                # flag 2: every lag in FP64
            lags = spread(m, W, S, TBV)
            t = _flat(lags)
            t[lags[m // 2]] = special
            cases.append(Case('truth', '%s_m%d' % (tag, m), t, kind='spread'))
        t = _flat(five)
        t[other[1]] = special                             # in the opposite direction from all the others
        t[other[0]] = t[other[2]] = HALF
        cases.append(Case('truth', '%s_opposite' % tag, t, ties=five + [other[1]], kind='spread'))
    return cases


def both_directions(W, S, TBV):
    """Ties in both records of a pair: mirrored lags, a tie at d = 0 (which both records list), runs of consecutive lags
    (the global-memory verifier shares loads along runs of up to four and must neither skip nor repeat a lag)."""
    cases = []
    three = spread(3, W, S, TBV, start=5, stride=11)
    cases.append(Case('both', 'mirrored', _flat(three + [-d for d in three]), kind='spread'))
    t = _flat(three + [-d for d in three])
    t[-three[-1]] = A + 1
    cases.append(Case('both', 'mirrored_plus_in_the_far_record', t, kind='spread'))
    cases.append(Case('both', 'zero_and_two', _flat([0, 5, -7]), kind='spread'))
    cases.append(Case('both', 'zero_and_neighbours', _flat([-1, 0, 1]), kind='spread'))
    t = _flat([-1, 0, 1])
    t[1] = A + 1
    cases.append(Case('both', 'zero_beaten_by_its_neighbour', t, kind='spread'))
    for n in (2, 3, 4, 5, 9):
        run = list(range(6, 6 + n))
        cases.append(Case('both', 'run%d' % n, _flat(run), kind='spread'))
        t = _flat(run)
        t[run[-1]] = A + 1
        cases.append(Case('both', 'run%d_last_wins' % n, t, kind='spread'))
    cases.append(Case('both', 'two_runs_one_lag_apart', _flat([10, 11, 12, 14, 15, 16]), kind='spread'))
    t = _flat([10, 11, 12, 14, 15, 16], A - 1)
    t[14] = A
    cases.append(Case('both', 'two_runs_second_starts_with_the_maximum', t, kind='spread'))
    for n in (5, 9):
        run = list(range(-(n // 2), n // 2 + 1))
        cases.append(Case('both', 'run%d_across_zero' % n, _flat(run), kind='spread'))
        t = _flat(run, A - 1)
        t[1] = A
        cases.append(Case('both', 'run%d_across_zero_maximum_behind_zero' % n, t, kind='spread'))
    return cases


def direction_drop(W, S, TBV):
    """Three ties in one direction; the other direction's maximum is (a) a half-amplitude decoy: the direction is dropped,
    (b) 2^20 - 1: kept, and loses in FP64, (c) 2^20 + 1: kept, and wins."""
    three = spread(3, W, S, TBV, start=4, stride=9)
    cases = []
    for name, v in (('decoy_dropped', HALF), ('minus_kept_loses', A - 1), ('plus_kept_wins', A + 1)):
        t = _flat(three)
        t[-9] = v
        cases.append(Case('drop', name, t, ties=three if v == HALF else three + [-9], kind='spread'))
    return cases


def window_ends(W, S, TBV):
    """Candidates at the last lags of the window (d = W - 1, W - 2: the mirrored window 1 holds -(W - 1), -(W - 2)), alone
    and beside a tie in the first group."""
    cases = []
    for name, table in (('last_two', {W - 1: A, W - 2: A}),
                        ('last_wins', {W - 2: A, W - 1: A + 1}),
                        ('last_but_one_wins', {W - 2: A + 1, W - 1: A}),
                        ('first_group_and_last', {3: A, W - 2: A, W - 1: A + 1}),
                        ('first_group_wins_over_last', {3: A, W - 2: A - 1, W - 1: A - 1})):
        cases.append(Case('end', name, table, kind='spread'))
    return cases


def randomised(W, S, TBV, seeds=(0, 1, 2)):
    """Designs of the families above over integer noise of +-2^10: the low limbs are non-zero, theta grows, some designed
    lags are candidates and some are not.  The truth stays exact; the records are only checked for soundness."""
    base = [list_length(W, S, TBV, ms=(26,))[0], list_length(W, S, TBV, ms=(27,))[0], lane_slots(W, S, TBV, ks=(8,))[0],
            both_directions(W, S, TBV)[-2], window_ends(W, S, TBV)[0], true_maximum(W, S, TBV)[0]]
    return [Case('noise', '%s_%s_seed%d' % (c.family, c.name, s), c.tables[0], ties=c.ties[0], kind=None, second=c.tables[1],
                 second_ties=c.ties[1], seed=s) for c in base for s in seeds]


# ---- traces ------------------------------------------------------------------------------------------------------------
def probe_sample(table, W):
    P = max(0, -min(table))
    assert P + max(max(table), 0) <= W - 1, 'the table does not fit a window of %d samples' % W
    return P


def window(table, W, N):
    """-> (N, W) int64: the profile (channel 0), the probe (1) and N - 2 further probes."""
    table = dict(table)
    P = probe_sample(table, W)
    if min(table) > 0 or max(table) < 0:
        table[0] = HALF                                   # the direction the table leaves empty
    x = np.zeros((N, W), dtype=np.int64)
    for s, v in table.items():
        x[0, P + s] = v
    x[1, P] = A
    own = [(P + W // 2 + 3 * (k - 2)) % W for k in range(2, N)]
    assert P not in own and len(set(own)) == len(own)
    for k, pk in zip(range(2, N), own):
        x[k, P] = HALF
        x[k, pk] = A
    return x


def traces(case, W, N):
    """-> (N, 2 W + 1) int64: two windows at hop W and one sample behind them."""
    x = np.concatenate([window(t, W, N) for t in case.tables] + [np.zeros((N, 1), dtype=np.int64)], axis=1)
    if case.seed is not None:
        rng = np.random.default_rng(1000 * case.seed + W + N)
        x = x + rng.integers(-NOISE, NOISE + 1, size=x.shape)
    return x


# ---- the exact reference -----------------------------------------------------------------------------------------------
def correlate_exact(a, b):
    """``np.correlate(a, b, 'full')`` of int64 vectors, exactly; pulse trains are correlated pulse by pulse."""
    ia, ib = np.flatnonzero(a), np.flatnonzero(b)
    if len(ia) * len(ib) > 4096:
        return np.correlate(a, b, 'full')
    c = np.zeros(len(a) + len(b) - 1, dtype=np.int64)
    if len(ia) and len(ib):
        np.add.at(c, (len(b) - 1 + ia[:, None] - ib[None, :]).ravel(), (a[ia][:, None] * b[ib][None, :]).ravel())
    return c


def pair_truth(a, b):
    """-> (kk, quotient at kk, the exact correlation, the quotients): the oracle's first maximum of c / norm."""
    c = correlate_exact(a, b)
    norm = np.sqrt(float(np.sum(a * a)) * float(np.sum(b * b)))
    quot = c.astype(np.float64) / norm
    kk = int(np.argmax(quot))
    return kk, quot[kk], c, quot


def reference(x, W, pairs, nwin=2):
    """-> lag (nwin, P) int64, cmax (nwin, P), kk (nwin, P): the exact reference of windows at hop W."""
    lag = np.empty((nwin, len(pairs)), dtype=np.int64)
    cmax = np.empty((nwin, len(pairs)))
    for w in range(nwin):
        seg = x[:, w * W:(w + 1) * W]
        for p, (i, j) in enumerate(pairs):
            kk, q, _, _ = pair_truth(seg[i], seg[j])
            lag[w, p], cmax[w, p] = (W - 1) - kk, q
    return lag, cmax, (W - 1) - lag


# ---- the screening, in NumPy ---------------------------------------------------------------------------------------------
def quantise(x):
    """One channel window -> (q, hi, lo, sum x^2, sum |q|, max |x|, sum lo^2) as quantize_kernel leaves them."""
    xf = x.astype(np.float64)
    mx = float(np.max(np.abs(xf)))
    q = np.clip(np.rint(xf * (QMAX / mx)), -QMAX, QMAX).astype(np.int64) if mx > 0 else np.zeros(len(x), dtype=np.int64)
    lo = ((q + 64) & 127) - 64
    hi = (q - lo) >> 7
    return q, hi, lo, float(np.sum(xf * xf)), float(np.sum(np.abs(q))), mx, float(np.sum(lo * lo))


def theta_model(mi, mj, W):
    """The kernel's candidate threshold (THETA_SOURCE) from the two channels' quantiser records."""
    iabs = QMAX * QMAX * np.sqrt(mi[3] * mj[3]) / (mi[5] * mj[5]) if mi[5] > 0 and mj[5] > 0 else 0.0
    lolo = np.sqrt(mi[6] * mj[6])
    return float(np.float32(((mi[4] + mj[4]) * 1.001 + 0.5 * W + 8.0 + 2.0 * lolo) * 1.0001 + 1.0e-6 * iabs))


Record = collections.namedtuple('Record', 'v theta ties near kk sure may slots')


def model_records(seg, geom):
    """Of one window (N, W): {(sliding i, partner j): Record} — the screening values I'[d] of lags d >= 0 (three limb
    products, recombined in f32 as the epilogue does), theta, the lags that tie at the maximum, the lags within 2 theta
    below it, the ties as np.correlate indices of the unordered pair, their lane loads, and the slots they fill where every
    group of theirs has a wave of its own (else None)."""
    N, W = seg.shape
    qs = [quantise(seg[i]) for i in range(N)]
    out = {}
    for i in range(N):
        for j in range(N):
            if i == j:
                continue
            (_, hi, lo, *_), (_, hj, lj, *_) = qs[i], qs[j]
            hh = correlate_exact(hi, hj)[W - 1:]
            mid = (correlate_exact(hi, lj) + correlate_exact(lo, hj))[W - 1:]
            v = np.float32(16384.0) * hh.astype(np.float32) + np.float32(128.0) * mid.astype(np.float32)
            assert v.dtype == np.float32
            theta = theta_model(qs[i], qs[j], W)
            top = v.max()
            ties = np.flatnonzero(v == top)
            near = np.flatnonzero((v < top) & (v.astype(np.float64) >= float(top) - 2.0 * theta))
            kk = (W - 1 + ties) if i < j else (W - 1 - ties)
            sure, may = lane_loads(ties, geom.S, geom.TBV, geom.nw)
            lanes = collections.Counter(lane_of(d, geom.S, geom.TBV) for d in ties)
            slots = sum(min(n, NSLOT) for n in lanes.values()) if all(p < geom.nw for p, _ in lanes) else None
            out[i, j] = Record(v, theta, ties, near, set(int(k) for k in kk), sure, may, slots)
    return out


def designed_record(rec):
    """What a record of a clean design must hold -> dict(count, flags, listed) with None for what the design leaves open.
    No lane over NSLOT: every tie is listed (count m, no flag; from KOUT + 1 ties on flag 2 and a full list).  A lane
    certainly over NSLOT: flag 1, and where every group has a wave of its own the count is the slots the ties fill."""
    m = len(rec.ties)
    if rec.may <= NSLOT:
        return dict(count=min(m, KOUT), flags=0 if m <= KOUT else 2, listed=rec.kk if m <= KOUT else None)
    if rec.sure > NSLOT and rec.slots is not None:
        return dict(count=min(rec.slots, KOUT), flags=1 | (2 if rec.slots > KOUT else 0), listed=None)
    if rec.sure > NSLOT:
        return dict(count=None, flags=None, listed=None, interval=True)
    return dict(count=None, flags=None, listed=None)


def covers(record32, kk):
    """Soundness of one 32-int record for the index kk: listed, inside a flagged interval, or flag 2."""
    n, fl = int(record32[0]), int(record32[1])
    return bool(fl & 2) or kk in set(int(k) for k in record32[CHDR:CHDR + n]) or \
        bool(fl & 1 and int(record32[2]) <= kk <= int(record32[3]))


# ---- which family runs where -------------------------------------------------------------------------------------------
# list, lane and truth on every verifier; end and stale on every screening instance; the rest on the default route — and
# both (the run form exists only there) and regroup (more lag groups than waves) on the global-memory verifier.
FAMILIES = {'list': list_length, 'lane': lane_slots, 'stale': stale_slots, 'truth': true_maximum, 'both': both_directions,
            'drop': direction_drop, 'end': window_ends, 'noise': randomised}
PLAN = (('dma', ('list', 'lane', 'truth', 'end', 'stale', 'both', 'drop', 'noise')),
        ('lds', ('list', 'lane', 'truth')),
        ('glob', ('list', 'lane', 'truth', 'both', 'regroup')),
        ('nc4', ('end', 'stale')),
        ('tb8', ('end', 'stale')),
        ('nsl1', ('lane', 'stale')),
        ('static', ('lane', 'stale')),
        ('npg', ('list', 'lane')),
        ('seg', ('lane',)))
TRIMMED = {('npg', 'list'): dict(ms=(26, 27)), ('npg', 'lane'): dict(ks=(7,)), ('seg', 'lane'): dict(ks=(6, 7, 16))}


def cases_for(route, family):
    """-> [(Geom, Case)] of one family on one route (the window-end family: at every length of ``end_windows``)."""
    out = []
    for W in (end_windows(route) if family == 'end' else [ROUTES[route]['W']]):
        g = route_geometry(route, W)
        if family == 'regroup':
            cases = stale_across_groups(g.W, g.S, g.TBV, g.nw)
        else:
            cases = FAMILIES[family](g.W, g.S, g.TBV, **TRIMMED.get((route, family), {}))
        out += [(g, c) for c in cases]
    return out
