"""How every result follows the amplitude of the input: the table, the transformations, the comparison and the input sets
of tests/test_scale_cases.py (CPU) and tests/test_gpu_scale.py (GPU); DESIGN.md section 27.  CPU only: nothing here opens the
GPU library.

**Transformations.**  T1 multiplies every sample by 2^k, T2 channel i by 2^(k_i) with the k_i of ``GAINS`` cycled, T3
negates every sample.  All three are exact in IEEE arithmetic as long as nothing overflows or becomes subnormal, and they
commute with every rounding, so the pipeline — linear filter, quadratic beams and matrices, relative thresholds — follows
them exactly: no comparison here has a tolerance.

**The table.**  ``TABLE[field] = (T1, T2, T3)``, each ``SAME`` (bit for bit), ``times(e)`` (the exact factor 2^(e k)),
``NEGATED`` or ``UNDEFINED`` (the definition depends on the relative gains of the elements: not compared).  The entries are
read off the definitions of include/nbls.h, not off a run:

- a lag is the arg-max over the lags of c_ij(l) / sqrt(E_i E_j): c_ij carries 2^(k_i + k_j), E_i E_j its square, the
  quotient nothing; cmax, MdCCM, the sub-sample fraction (a ratio of three c_ij of ONE pair) and everything solved from the
  lags (z, vel, baz, sigma_tau, the weights, the confidence intervals, the closures, the kept elements, the families) are
  ``SAME`` under all three;
- beam, grid and spectra sum over elements: T2 weights the elements differently, which is another beam (``UNDEFINED``); their
  powers carry 2^(2k) under T1, their ratios (F, the peak offsets, the MUSIC pseudo-spectrum, a normalised correlation), the
  indices and the counts nothing; the Jacobi rotations and every floor (peaks, CLEAN, eigenvalues, loading) are ratios;
- the filtered samples and the beam trace are linear: 2^k under T1, the sign under T3; a filtered channel follows its own
  gain under T2 (``times(1)`` with k = k_i);
- a plan with a lag seed searches the lags around the delay its grid maximum predicts, a beam: there the lags and what
  follows from them are ``UNDEFINED`` under T2 (``behaviour(..., seeded=True)``).

``CONFIG`` are the fields that restate the call (window plan, geometry, times): ``SAME``."""
import functools
import importlib
import re

import numpy as np

from narrow_band_least_squares_amd import engine, lts_array, planner, synthetic

import music_cases

SAME, NEGATED, UNDEFINED = 'same', 'negated', 'undefined'
T1, T2, T3 = 'T1', 'T2', 'T3'
TRANSFORMATIONS = (T1, T2, T3)


def times(e):
    return ('times', int(e))


GAINS = (0, -30, 24, 7, -3, 11)
K_PHYSICAL = (-30, 24)                 # 1e-9 m/s against unit scale; 2^24 digitiser counts: the contract
K_WIDE = (-100, 100)                   # far outside the float range, every fourth-order product inside 2^+-450
K_ALL = (-100, -30, 24, 100)
T0 = 17884.0729166667

_LAGS = (SAME, SAME, SAME)
_RATIO = (SAME, UNDEFINED, SAME)
_POWER = (times(2), UNDEFINED, SAME)
_LINEAR = (times(1), UNDEFINED, NEGATED)

CONFIG = ('nwin', 't', 'sos', 'W', 'inc', 'pair_idx', 'xij', 'nchans', 'alpha', 'handle', 'lts', 'fs', 'families_in_pass')
LAG_FIELDS = ('lag', 'lag_frac', 'cmax', 'mask', 'weights', 'grids', 'z', 'vel', 'baz', 'mdccm', 'sigma_tau', 'vel_uncert',
              'baz_uncert', 'consistency', 'closure_max', 'element_consistency', 'dropped_mask', 'kept_count',
              'dropped_elements', 'family', 'family_table')
RATIO_FIELDS = ('fstat', 'grid_index', 'grid_fstat', 'grid_map', 'capon_index', 'bartlett_index', 'element_delay', 'element_cc',
                'element_shift', 'clean_count', 'clean_index', 'music_sources', 'music_sweeps', 'music_index', 'music_power',
                'music_map', 'music_vectors', 'music_peak_power',
                'capon_vel', 'capon_baz', 'bartlett_vel', 'bartlett_baz', 'clean_vel', 'clean_baz', 'music_vel', 'music_baz',
                'source_slowness', 'source_vel', 'source_baz') + tuple(
    w + f for w in ('capon', 'bartlett', 'music') for f in ('_peak_count', '_peak_index', '_peak_offset', '_peak_slowness',
                                                             '_peak_vel', '_peak_baz'))
POWER_FIELDS = ('beam_power', 'grid_power', 'capon_power', 'bartlett_power', 'capon_map', 'bartlett_map', 'capon_csdm',
                'clean_csdm', 'clean_power', 'clean_total', 'clean_residual', 'capon_peak_power', 'bartlett_peak_power',
                'music_eigenvalues', 'source_power')
LINEAR_FIELDS = ('beam_trace', 'filtered')

TABLE = {}
TABLE.update({k: _LAGS for k in CONFIG + LAG_FIELDS})
TABLE.update({k: _RATIO for k in RATIO_FIELDS})
TABLE.update({k: _POWER for k in POWER_FIELDS})
TABLE['beam_trace'] = _LINEAR
TABLE['filtered'] = (times(1), times(1), NEGATED)          # (T2: channel i by its own 2^(k_i))

NOT_ARRAYS = ('handle', 'sos', 'families_in_pass')        # declared, but objects of the call: not compared


def behaviour(field, T, seeded=False):
    """How ``field`` answers transformation ``T``; ``seeded``: of a plan with a lag seed (``seed_halfwidths``)."""
    if field not in TABLE:
        raise KeyError('tests/scale_cases.py declares no behaviour for %r: add it to the table (DESIGN.md section 27)' % (field,))
    b = TABLE[field][TRANSFORMATIONS.index(T)]
    if seeded and T == T2 and field in LAG_FIELDS:
        return UNDEFINED
    return b


# ---- the transformations ---------------------------------------------------------------------------------------------
def gains(nchans):
    """k_i of T2, one per channel."""
    return np.array([GAINS[i % len(GAINS)] for i in range(nchans)], dtype=np.int64)


def transform(x, T, k=0):
    """The trace ``x`` (nchans, npts) under T -> a new C-contiguous float64 array; ``k``: the exponent of T1."""
    x = np.asarray(x, dtype=np.float64)
    if T == T1:
        return np.ascontiguousarray(np.ldexp(x, int(k)))
    if T == T2:
        return np.ascontiguousarray(np.ldexp(x, gains(x.shape[0])[:, None]))
    if T == T3:
        return np.ascontiguousarray(-x)
    raise KeyError(T)


def cases(ks=K_ALL, t2=True, t3=True):
    """-> [(label, T, k)]."""
    out = [('T1 k=%+d' % k, T1, k) for k in ks]
    if t2:
        out.append(('T2', T2, 0))
    if t3:
        out.append(('T3', T3, 0))
    return out


def _ldexp(a, e):
    a = np.asarray(a)
    if a.dtype.kind == 'c':
        out = np.empty_like(a)
        out.real, out.imag = np.ldexp(a.real, e), np.ldexp(a.imag, e)
        return out
    return np.ldexp(a, e)


def _no_sign_of_zero(a):
    """+0.0 for either zero (a cell nothing was added to stays +0.0 whatever the sign of the input)."""
    a = np.array(a, copy=True)
    for part in ((a.real, a.imag) if a.dtype.kind == 'c' else (a,)):
        part[part == 0] = 0.0
    return a


def expected(field, ref, T, k=0, seeded=False):
    """What ``field`` must be after T when it was ``ref`` before -> an array, or None where it is not compared.  A ``times``
    field under T2 takes ``k`` per channel, broadcast against the array (the filtered samples: ``k[:, None]``)."""
    b = behaviour(field, T, seeded)
    if b == UNDEFINED:
        return None
    ref = np.asarray(ref)
    if b == SAME or ref.dtype.kind not in 'fc':
        assert b == SAME or ref.dtype.kind in 'fc', (field, b, ref.dtype)
        return ref
    if b == NEGATED:
        return -ref
    e = b[1] * (gains(ref.shape[0])[:, None] if T == T2 else int(k) if T == T1 else 0)
    return _ldexp(ref, e)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def check_field(field, ref, got, T, k=0, seeded=False, label=''):
    """Assert one field against the table -> the number of cells compared (0: not compared)."""
    if field in NOT_ARRAYS:
        return 0
    if ref is None or got is None:
        assert ref is None and got is None, '%s %s: there in one run only' % (label, field)
        return 0
    exp = expected(field, ref, T, k, seeded)
    if exp is None:
        return 0
    got = np.asarray(got)
    if behaviour(field, T, seeded) == NEGATED:
        exp, got = _no_sign_of_zero(exp), _no_sign_of_zero(got)
    if not same_bits(exp, got):
        assert exp.shape == got.shape and exp.dtype == got.dtype, (label, field, exp.shape, got.shape, exp.dtype, got.dtype)
        bad = np.flatnonzero(~((exp == got) | ((exp != exp) & (got != got))).ravel())
        where = bad[:4].tolist()
        raise AssertionError('%s %s (%s under %s, k=%s): %d of %d cells differ, first at flat %s: expected %r, got %r'
                             % (label, field, behaviour(field, T, seeded), T, k, max(len(bad), 1), exp.size, where,
                                exp.ravel()[where].tolist(), got.ravel()[where].tolist()))
    return int(exp.size)


def fields_of(res):
    """The public attributes of a ``BandBatch`` (or the keys of a result dictionary)."""
    if isinstance(res, dict):
        return sorted(res)
    return sorted(k for k in vars(res) if not k.startswith('_'))


def compare(ref, got, T, k=0, seeded=False, label='', skip=()):
    """Every field two ``BandBatch`` (or two result dictionaries) carry, by the table -> (fields compared, cells).  A field
    without an entry is an error, not a gap."""
    names = fields_of(ref)
    assert names == fields_of(got), (label, sorted(set(names) ^ set(fields_of(got))))
    get = (lambda r, f: r[f]) if isinstance(ref, dict) else getattr
    nf = nc = 0
    for f in names:
        behaviour(f, T, seeded)
        if f in skip:
            continue
        n = check_field(f, get(ref, f), get(got, f), T, k, seeded, label)
        nf, nc = nf + (n > 0), nc + n
    return nf, nc


# ---- what has to be in the table -------------------------------------------------------------------------------------
def batch_fields():
    """Every field a ``BandBatch`` can carry: those of ``engine.new_result`` with every request on, and what ``process``
    adds behind the pass (the families)."""
    res = engine.new_result(4, 0.5, 20.0, np.array([32]), np.array([16]), np.array([3]), 3, True, True, True, True, True, True, 9,
                            True, True, 9, True, True, 2, True, 64, True, clean_iterations=2, want_clean_csdm=True, want_music=True,
                            want_music_maps=True, want_music_vectors=True, want_music_peaks=True)
    names = set(fields_of(res)) | {'weights', 'family', 'family_table', 'families_in_pass'}
    names |= set(engine.CLEAN_FIELDS) | set(engine.MUSIC_FIELDS)
    names |= {w + f for w in ('capon', 'bartlett', 'music') for f in engine.PEAK_FIELDS}
    missing = [k for k, v in vars(res).items() if v is None and not k.startswith('_') and k not in CONFIG]
    assert not missing, 'new_result left %s unset with every request on' % missing
    return sorted(names), res


def result_keys():
    """Every key of the result dictionaries of the public calls: the dictionaries ``lts_array._returns_*`` build from a
    ``BandBatch`` with every request on, and every key the two modules of the public calls write into an ``out`` dictionary."""
    _, res = batch_fields()
    grid = planner.slowness_grid(3.0, 3)
    keys = set()
    keys |= set(lts_array._returns_capon(res, grid, True))
    keys |= set(lts_array._returns_kept(res, 4, True, dict(capon_grid=grid, want_capon_maps=True)))
    keys |= set(lts_array._returns_clean(res, grid, 1.0, 2))
    keys |= set(lts_array._returns_music(res, grid))
    # (the package attribute of that name is the function: fetch the module by name)
    for mod in (lts_array, importlib.import_module('narrow_band_least_squares_amd.narrow_band_least_squares')):
        with open(mod.__file__.replace('.pyc', '.py')) as f:
            text = f.read()
        keys |= set(re.findall(r"\bout\['(\w+)'\]", text))
        for call in re.findall(r'\bout(?: = dict|\.update)\(([^()]*=res\.[^()]*)\)', text):
            keys |= set(re.findall(r'(\w+)=res\.', call))
    return sorted(keys)


# ---- the input sets --------------------------------------------------------------------------------------------------
def centred(rij):
    return rij - rij.mean(axis=1, keepdims=True)


def _frozen(x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    x.flags.writeable = False
    return x


@functools.lru_cache(maxsize=None)
def prefiltered(name):
    """-> dict(data (N, npts), fs, winlen, rij, W): the prefiltered sets, by the route they are named for.
    'screen': 6 elements, fs 20, W 600, a plane wave plus noise (the shape of the hostile-input tests);
    'long': 4 elements, fs 200, W 5000 (the slab quantiser); 'groups': 8 elements, fs 100, W 6000 (two partner groups);
    'general': 4 elements, W 257; 'plans': 8 elements, W 257 (bounded, seeded and refined plans)."""
    if name == 'screen':
        N, fs, winlen, npts, band, seed = 6, 20.0, 30.0, 3120, (0.5, 8.0), 5
    elif name == 'long':
        N, fs, winlen, npts, band, seed = 4, 200.0, 25.0, 26000, (0.5, 8.0), 5
    elif name == 'groups':
        N, fs, winlen, npts, band, seed = 8, 100.0, 60.0, 15600, (0.2, 4.0), 9
    elif name == 'general':
        N, fs, winlen, npts, band, seed = 4, 20.0, 257.5 / 20.0, 900, (0.5, 4.0), 21
    elif name == 'plans':
        N, fs, winlen, npts, band, seed = 8, 20.0, 257.5 / 20.0, 900, (0.5, 4.0), 22
    else:
        raise KeyError(name)
    rij = synthetic.array_geometry(N, 1.0, seed=40 + N)
    data = synthetic.plane_wave(rij, npts, fs, band[0], band[1], seed=seed)
    return dict(data=_frozen(data), fs=fs, winlen=winlen, rij=centred(rij), W=int(winlen * fs), N=N)


RAW_EDGES = [(0.1, 0.1031), (0.5, 2.0)]          # the narrowest band of tests/filter_truth.py at 20 Hz beside a wide one
RAW_WINLENS = [60.0, 30.0]
RAW_FILTER = ('butter', 2, 0.01)


@functools.lru_cache(maxsize=None)
def raw():
    """The raw trace of the filter case: 6 elements, fs 20, 3120 samples; two zero-phase bands of W = 1200 and 600."""
    N, fs, npts = 6, 20.0, 3120
    rij = synthetic.array_geometry(N, 1.0, seed=46)
    data = synthetic.plane_wave(rij, npts, fs, 0.05, 4.0, seed=31)
    return dict(data=_frozen(data), fs=fs, rij=centred(rij), N=N)


EXTRAS_SHAPE = (65, 16, 8)                       # (W, Ls, Hs)
EXTRAS_GRID = 129


@functools.lru_cache(maxsize=None)
def extras(N):
    """The set of the opt-in results: ``music_cases.traces(N, 65, 2)`` (two plane waves at 40 dB, 132 samples, three
    windows), the 129-point grid, Ls 16, Hs 8.  The grid is a random draw, no lattice: ``cells`` lays its points out 13 to a
    row, the neighbourhood a peak request then works on."""
    W = EXTRAS_SHAPE[0]
    data, rij = music_cases.traces(N, W, 2)
    g = np.arange(EXTRAS_GRID)
    return dict(data=_frozen(data), fs=music_cases.FS, winlen=(W + 0.5) / music_cases.FS, rij=rij, W=W, N=N,
                grid=music_cases.grid(EXTRAS_GRID), freq=music_cases.FREQ,
                cells=np.ascontiguousarray(np.stack([g % 13, g // 13], axis=1).astype(np.int32)))


GAIN_STEP = 40


@functools.lru_cache(maxsize=None)
def gain_step():
    """'screen' with the second half of the trace times 2^40 -> (data, first sample of the second half)."""
    c = prefiltered('screen')
    half = c['data'].shape[1] // 2
    data = np.array(c['data'])
    data[:, half:] = np.ldexp(data[:, half:], GAIN_STEP)
    return _frozen(data), half


def window_sides(npts, fs, winlen, overlap, half):
    """-> (windows wholly before ``half``, windows wholly from ``half`` on, windows that straddle it)."""
    W, inc, nwin = planner.window_plan(npts, fs, winlen, overlap)[:3]
    start = np.arange(int(nwin)) * int(inc)
    before, after = start + int(W) <= half, start >= half
    return np.flatnonzero(before), np.flatnonzero(after), np.flatnonzero(~before & ~after)


def counts_int32():
    """'screen' as raw digitiser counts: int32, up to 2^23."""
    x = prefiltered('screen')['data']
    return np.rint(x * (2.0 ** 23 / np.abs(x).max())).astype(np.int32)


# ---- the condition on the inputs -------------------------------------------------------------------------------------
TINY = np.finfo(np.float64).tiny                 # the smallest normal double
HUGE_LOG2 = 450                                  # every fourth-order product stays inside 2^+-HUGE_LOG2


def exponent_range(x):
    """(lowest, highest) binary exponent of the non-zero samples."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    e = np.frexp(a[a > 0])[1]
    return int(e.min()) - 1, int(e.max()) - 1


def window_energies(x, W, inc):
    """Sum of squares of every window of every channel (the norms of the correlators, the S_t of the beams) -> (N, nwin)."""
    x = np.asarray(x, dtype=np.float64)
    start = np.arange(0, x.shape[1] - W, inc)
    return np.array([[np.sum(x[i, s:s + W] ** 2) for s in start] for i in range(x.shape[0])])


def check_condition(x, W, inc, label=''):
    """No sample and no window's sum of squares is subnormal, none overflows, and the product of two window energies — the
    fourth-order quantity under the square root of a correlation's norm — stays inside 2^+-450.  Zeros are fine: they scale
    exactly.  -> (lowest, highest) log2 of a product of two energies."""
    x = np.asarray(x, dtype=np.float64)
    assert np.isfinite(x).all(), label
    nz = np.abs(x[x != 0])
    assert nz.size and nz.min() >= TINY, '%s: a subnormal sample' % label
    E = window_energies(x, W, inc)
    assert E.size and np.isfinite(E).all() and (E > 0).all() and E.min() >= TINY, '%s: a window energy out of range' % label
    lo, hi = 2.0 * np.log2(E.min()), 2.0 * np.log2(E.max())
    assert -HUGE_LOG2 <= lo and hi <= HUGE_LOG2, '%s: fourth-order products reach 2^%.0f .. 2^%.0f' % (label, lo, hi)
    return lo, hi
