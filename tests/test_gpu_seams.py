"""beam_fstat_kernel (csrc/beam.hip), beam_grid_kernel (csrc/beam_grid.hip) and refine_lag_kernel (csrc/refine.hip) at
the window lengths, halos and array sizes where their loops change: one short of, at and one past every edge of a t
loop, both sides of every LDS switch, a workgroup that holds one-wave and cooperative units, the last lag that is
refined, and arrays of 16, 17 and 32 elements.  The cases come from the kernels' constants (tests/seam_cases.py;
tests/test_seam_cases.py checks on the CPU that they reach their seams and that the references meet the conditions
below).  Every comparison is the one of test_gpu_beam.py, test_gpu_grid.py and test_gpu_subsample.py, through their
helpers: the long-double truths of beam_truth / grid_truth / refine_truth with their derived rounding bounds, the index
under the total order, NaN / inf in exactly the reference's cells, zeros behind ``nwin``.  The conditions that keep a
comparison from hiding a failure are theirs too: at most 1 % of a beam case's cells within 1e-6 of a delay tie (none
here), F compared on at least half the windows, no ``power_only`` cell in a grid case, every pair of a refinement case
with |D| >= 2^20 E.  Traces hold eleven windows at half overlap (about 6 W samples) and have odd lengths."""
import numpy as np
import pytest

import refine_truth as rt
import seam_cases as sc
import test_gpu_beam as tb
import test_gpu_grid as tg
import test_gpu_subsample as ts
from narrow_band_least_squares_amd import engine, planner, _hip

pytestmark = pytest.mark.gpu

FS = sc.FS
T0 = tb.T0
GRID5 = tg.GRID5


def _beam_against_reference(res, filt, band=0, label=''):
    """test_gpu_beam's comparison, and F on at least half the windows -> the reference."""
    ref, on_f = tb._against_reference(res, filt, band=band, label=label)
    n = int(res.nwin[band])
    assert on_f >= n // 2, '%s: F compared on %d of %d windows' % (label, on_f, n)
    cmp_f = ~ref['skip'] & ~ref['power_only'] & np.isfinite(ref['fstat'])
    worst = np.max(np.abs(res.fstat[band, :n] - ref['fstat'])[cmp_f] / ref['tol_fstat'][cmp_f])
    print('%s: worst |d fstat| / bound = %.3g on %d windows' % (label, worst, on_f))
    return ref


# ---- 1. beam: window-length seams -------------------------------------------------------------------------------------

@pytest.mark.parametrize('W', sc.BEAM_SEAMS)
def test_beam_window_length_seams(W):
    """4 elements under LTS, the last one mistimed.  Up to BEAM_WAVE_W = 512 samples one wave sums a unit in trips of 256
    samples (255 and 256: one trip with and without a partial quarter, 511 and 512: two), beyond it the four waves in
    trips of 1024 (513 and 1023: one partial trip, 1024: one whole, 1025: a second trip of one sample).  Elements 0 and
    1 are swapped so that the delays have both signs: the first window reads before the trace's start, the last behind
    its end."""
    data, rij = sc.plane_wave(4, W, mistimed=True, swap=True)
    res = tb._process(data, rij, W, 0.5)
    n = int(res.nwin[0])
    assert n == 11
    _beam_against_reference(res, data, label='beam seams W=%d' % W)
    before, behind = sc.reads_outside(res.xij, res.z[0], W, int(res.inc[0]), n, data.shape[1], 4)
    assert before >= 1 and behind >= 1, (before, behind)
    assert np.all(np.isfinite(res.fstat[0, :n])) and np.all(res.beam_power[0, :n] > 0)


# ---- 2. beam: a workgroup of one-wave and cooperative units ----------------------------------------------------------

@pytest.mark.parametrize('order', [(0, 1), (1, 0)], ids=['cooperative_band_first', 'one_wave_band_first'])
def test_beam_workgroup_across_a_band_seam(monkeypatch, order):
    """Two bands filtered on the GPU, windows of 513 samples (the four waves sum a unit and meet at two barriers) and
    of 65 (wave j sums unit j, no barrier).  ``nbls_plan`` numbers the units band by band, windows ascending
    (api.hip: plan_windows, unit_off), an unstreamed pass solves them in one launch from unit 0 (nbls_launch_solve) and
    a workgroup takes BEAM_WAVES consecutive units: the first band's window count is not a multiple of BEAM_WAVES, so
    one workgroup holds units of both kinds — in either order of the bands.  Each band against the reference on the
    filtered samples the kernel read, and the whole result bit for bit against the two bands as single-band calls."""
    monkeypatch.setenv('NBLS_STREAM_RESULTS', '0')
    data, rij = sc.plane_wave(4, None, npts=sc.MIXED_NPTS)
    edges, Ws = [sc.MIXED_BANDS[k] for k in order], [sc.MIXED_W[k] for k in order]

    def call(e, w, vector_len=None):
        return engine.process(data, FS, T0, rij, e, [sc.winlen(x) for x in w], 0.5, 1.0, 'butter', 2, 0.01,
                              vector_len=vector_len, want_z=True, want_beam=True)
    res = call(edges, Ws)
    assert [int(w) for w in res.W] == Ws
    assert int(res.nwin[0]) % sc.BEAM_WAVES != 0                     # a workgroup straddles the seam between the bands ...
    assert (Ws[0] > sc.BEAM_WAVE_W) != (Ws[1] > sc.BEAM_WAVE_W)      # ... and its units differ in who sums them
    assert not engine.stream_pays(1.0, res.nwin, 6)
    for b in range(2):
        _beam_against_reference(res, res.handle.fetch_filtered(b), band=b, label='mixed workgroup, band %d W=%d' % (b, Ws[b]))
    for b in range(2):
        single = call([edges[b]], [Ws[b]], vector_len=res.vel.shape[1])
        for k in ('vel', 'baz', 'z', 'beam_power', 'fstat'):
            np.testing.assert_array_equal(getattr(single, k)[0], getattr(res, k)[b], err_msg='%s of band %d' % (k, b))


# ---- 3. grid: step seams --------------------------------------------------------------------------------------------

def _grid_pass(data, rij, W, grid, label, alpha=1.0):
    """One pass against the truth; the fetched delay table must be the float64 expression's."""
    N = data.shape[0]
    d = tg._fit_for_exact_delays(planner.co_array(rij)[0], grid, N)
    res = tg._process(data, rij, W, alpha, grid=grid)
    np.testing.assert_array_equal(res.handle.fetch_beam_grid_delays(), d)
    ref = tg._against_reference(res, data, grid, label=label)
    n = int(res.nwin[0])
    assert np.all(res.grid_index[0, :n] >= 0) and np.all(np.isfinite(res.grid_fstat[0, :n])) and np.all(res.grid_power[0, :n] > 0)
    return res, ref, d


def _same_bits_on_shared_columns(a, b, G=len(GRID5)):
    """Two passes whose grids share their first G points: those map columns are the same bits, and so are index, F and P
    of every window whose maximum lies among them in both."""
    np.testing.assert_array_equal(a.grid_map[..., :G], b.grid_map[..., :G])
    n = int(a.nwin[0])
    same = (a.grid_index[0, :n] < G) & (b.grid_index[0, :n] < G)
    assert same.sum() >= n // 2
    for k in ('grid_index', 'grid_fstat', 'grid_power'):
        np.testing.assert_array_equal(getattr(a, k)[0, :n][same], getattr(b, k)[0, :n][same], err_msg=k)


@pytest.mark.parametrize('W', sc.GRID_SEAMS)
def test_grid_step_seams_in_both_forms(W):
    """A wave steps through GRID_BLOCK = 256 samples: 255 is the partial step alone, 256 and 512 whole steps alone, 511
    and 513 both.  Each length staged in LDS (GRID5) and read from global memory (GRID5 and one point whose delay is past
    the LDS cap): every map cell against the truth, the 25 shared columns bit for bit."""
    N = 4
    data, rij = sc.plane_wave(N, W)
    xij = planner.co_array(rij)[0]
    far = sc.far_grid(xij, N, W)
    lib = _hip.load_library()
    staged, _, d = _grid_pass(data, rij, W, GRID5, 'grid steps W=%d staged' % W)
    plain, _, d_far = _grid_pass(data, rij, W, far, 'grid steps W=%d global' % W)
    assert lib.nbls_beam_grid_lds_bytes(N, W, int(np.abs(d).max())) == N * (W + 2 * int(np.abs(d).max())) * 8
    assert lib.nbls_beam_grid_lds_bytes(N, W, int(np.abs(d_far).max())) == 0
    assert d.min() < 0                                               # window 0 reads before the trace's start
    _same_bits_on_shared_columns(plain, staged)


# ---- 4. grid: the exact LDS cap -------------------------------------------------------------------------------------

@pytest.mark.parametrize('N,W,nwin', sc.GRID_CAP_SHAPES)
def test_grid_at_the_exact_lds_cap(N, W, nwin):
    """H is the largest halo ``nbls_beam_grid_lds_bytes`` still stages for N x W samples (2367 at 4 x 257, 279 at 32 x 65).
    GRID5 and one point along the axis of the largest co-array component whose delay is exactly H: the last staged plan,
    its block the whole cap or 8 N bytes less; the same with H + 1: the first plan that reads global memory."""
    data, rij = sc.plane_wave(N, W, nwin=nwin)
    xij = planner.co_array(rij)[0]
    H, (at_cap, past_cap) = sc.cap_grids(xij, N, W)
    lib = _hip.load_library()
    assert lib.nbls_beam_grid_lds_bytes(N, W, H) == N * (W + 2 * H) * 8 and lib.nbls_beam_grid_lds_bytes(N, W, H + 1) == 0
    staged, _, d0 = _grid_pass(data, rij, W, at_cap, 'grid cap N=%d W=%d H=%d staged' % (N, W, H))
    assert int(staged.nwin[0]) == nwin and int(np.abs(d0).max()) == H
    plain, _, d1 = _grid_pass(data, rij, W, past_cap, 'grid cap N=%d W=%d H=%d global' % (N, W, H + 1))
    assert int(np.abs(d1).max()) == H + 1
    _same_bits_on_shared_columns(plain, staged)


# ---- 5. refinement: step seams and LDS switches ---------------------------------------------------------------------------

@pytest.mark.parametrize('W', sc.REFINE_SEAMS)
def test_refinement_step_seams(W):
    """The lanes of a wave stride over n by 64: 63 (one trip, one lane idle), 64, 127, 128 and 129 (a third trip of one
    lane).  4 elements under LTS, the last one mistimed; the LDS form."""
    data, rij = sc.sinusoids(4, W, mistimed=True)
    assert _hip.refine_lds_bytes(4, W) == 4 * W * 8
    res = ts._process(data, rij, W, 0.5)
    ts._check_fractions(res, data, 'refine seams N=4 W=%d' % W)


@pytest.mark.parametrize('side', [0, 1], ids=['lds', 'global'])
@pytest.mark.parametrize('N', sc.REFINE_SWITCH_N)
def test_refinement_on_either_side_of_the_lds_switch(N, side):
    """The longest window whose N rows are staged in LDS (eight waves; 3413 samples at 3 elements, 320 at 32) and the
    next one (global memory, four waves dealing the pairs: 3 pairs on 4 waves, 496 on 4)."""
    W = sc.refine_switch(N) + side
    assert (_hip.refine_lds_bytes(N, W) > 0) == (side == 0)
    data, rij = sc.sinusoids(N, W)
    res = ts._process(data, rij, W, 1.0)
    ts._check_fractions(res, data, 'refine switch N=%d W=%d' % (N, W))


# ---- 6. refinement: the last refined lag ---------------------------------------------------------------------------------

def _crafted_pass(x, W, n):
    res = engine.process(x, FS, T0, sc.CRAFTED_GEOMETRY, [(None, None)], [sc.winlen(W)], 0.0, 1.0, prefiltered=True,
                         want_lag=True, want_subsample=True)
    assert (int(res.W[0]), int(res.inc[0]), int(res.nwin[0])) == (W, W, n)
    assert [tuple(p) for p in res.pair_idx] == sc.CRAFTED_PAIRS
    return res


def _crafted_reference(x, W, lag):
    return rt.refine_windows(x, W, [w * W for w in range(len(lag))], sc.CRAFTED_PAIRS, lag)


@pytest.mark.parametrize('W', sc.CRAFTED_W)
def test_refinement_at_the_last_refined_lag(W):
    """Windows of two-sample pulses of unequal height (tests/seam_cases.py: PLUS, MINUS): pair (0, 1) is picked at
    +(W-2) and at -(W-2), where R(l+1) has one term, R(l) two and R(l-1) three and the fraction is -+1/12; pair (2, 3) at
    +-(W-1), which is not refined: exactly 0.  The neighbouring windows hold pulses at their edges, so a term read outside
    the window would not be a zero."""
    kinds = sc.CRAFTED_KINDS
    x = sc.crafted_trace(W, kinds)
    n = len(kinds)
    res = _crafted_pass(x, W, n)
    np.testing.assert_array_equal(res.lag[0, :n], sc.crafted_lags(kinds, W),
                                  err_msg='a finding about the correlator, not the refinement: the lags picked on the crafted '
                                          'windows are not the designed ones')
    ref = _crafted_reference(x, W, res.lag[0, :n])
    got = res.lag_frac[0, :n]
    assert np.all(np.isfinite(ref['bound']))
    err = np.abs(got - ref['frac'])
    print('refine last lag W=%d: worst |d frac| / bound = %.3g; pair (0, 1): %r' % (W, np.max(err / ref['bound']), got[:, 0].tolist()))
    assert np.all(err <= ref['bound'])
    for w, kind in enumerate(kinds):
        sign = 1 if kind == '+' else -1
        assert res.lag[0, w, 0] == sign * (W - 2) and abs(got[w, 0] + sign / 12.0) <= ref['bound'][w, 0] and got[w, 0] != 0.0
        assert abs(res.lag[0, w, 5]) == W - 1 and got[w, 5] == 0.0 and not np.signbit(got[w, 5])
    assert not res.lag_frac[0, n:].any()


@pytest.mark.parametrize('W', sc.CRAFTED_W)
def test_refinement_with_a_nan_where_a_left_out_term_would_read(W):
    """The same windows with a NaN in channel 0 (``a`` of pair (0, 1)) one sample before the window picked at +(W-2) and
    one sample behind the window picked at -(W-2): the terms of R(l+1) and R(l-1) that fall outside the window would
    read exactly those samples.  They are left out, not added as zeros: the fractions stay the finite values of the
    reference.  (Inside a window a NaN makes the pick W-1 by NumPy's semantics, and that lag is not refined: the two
    windows that hold the NaN samples show it, every pair of channel 0 there has fraction 0.)"""
    x = sc.crafted_nan_trace(W)
    n = len(sc.NAN_KINDS)
    res = _crafted_pass(x, W, n)
    np.testing.assert_array_equal(res.lag[0, 1:3], sc.crafted_lags(sc.NAN_KINDS[1:3], W),
                                  err_msg='a finding about the correlator, not the refinement: the lags picked on the two '
                                          'clean windows are not the designed ones')
    ref = _crafted_reference(x, W, res.lag[0, :n])
    got = res.lag_frac[0, :n]
    assert np.all(np.isfinite(got))
    touched = ~np.isfinite(ref['D']) | (ref['D'] >= 0)
    assert not touched[1, [0, 1, 3, 4]].any() and not touched[2, [0, 1, 2, 4]].any()        # the refined pairs of the clean windows
    assert touched[0, :3].all() and touched[3, :3].all()                                    # channel 0's pairs where it holds a NaN
    assert not got[touched].any()
    assert np.all(np.isfinite(ref['bound'][~touched])) and np.all(np.abs(got - ref['frac'])[~touched] <= ref['bound'][~touched])
    assert abs(got[1, 0] + 1 / 12.0) <= ref['bound'][1, 0] and abs(got[2, 0] - 1 / 12.0) <= ref['bound'][2, 0]


# ---- 7. array sizes ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('N,alpha,W', sc.BEAM_SIZE_CASES)
def test_array_sizes_beam(N, alpha, W):
    """16 and 32 elements under LTS (the bucket kernel) with the last one mistimed, 17 under OLS; one wave per unit (65
    samples) and the four waves (513).  Lane i of a wave holds element i's delay and row, read back with ``readlane``."""
    data, rij = sc.plane_wave(N, W, mistimed=alpha < 1.0)
    res = tb._process(data, rij, W, alpha)
    n = int(res.nwin[0])
    _beam_against_reference(res, data, label='beam sizes N=%d W=%d' % (N, W))
    assert np.all(np.isfinite(res.fstat[0, :n])) and np.all(res.beam_power[0, :n] > 0)


@pytest.mark.parametrize('N,alpha,W', sc.OTHER_SIZE_CASES)
def test_array_sizes_grid(N, alpha, W):
    data, rij = sc.plane_wave(N, W, mistimed=alpha < 1.0)
    res, ref, d = _grid_pass(data, rij, W, GRID5, 'grid sizes N=%d W=%d' % (N, W), alpha=alpha)
    n = int(res.nwin[0])
    print('grid sizes N=%d W=%d: LDS bytes %d' % (N, W, _hip.load_library().nbls_beam_grid_lds_bytes(N, W, int(np.abs(d).max()))))
    assert np.count_nonzero(res.grid_index[0, :n] == ref['index']) >= n // 2


@pytest.mark.parametrize('N,alpha,W', sc.OTHER_SIZE_CASES)
def test_array_sizes_refinement(N, alpha, W):
    """120, 136 and 496 pairs dealt to the eight waves of the LDS form (16 and 17 elements, 32 x 65 samples) — 16 and 17
    elements x 513 samples are staged too."""
    data, rij = sc.sinusoids(N, W, mistimed=alpha < 1.0)
    assert _hip.refine_lds_bytes(N, W) == N * W * 8
    res = ts._process(data, rij, W, alpha)
    ts._check_fractions(res, data, 'refine sizes N=%d W=%d' % (N, W))


def test_sub_array_of_30_of_32_elements_equals_the_call_on_the_sub_array():
    """``process_multi``: the full array of 32 and an estimator without elements 3 and 17, both under LTS.  The sub-array's
    beam results are those of the single call on its 30 rows, bit for bit, and match the reference at that call's z."""
    W = sc.SIZE_W[0]
    data, rij = sc.plane_wave(32, W, mistimed=True)
    ests = engine.normalize_estimators([(0.5, ()), (0.5, sc.SUB_REMOVE)], 32)
    kept = engine.kept_elements(32, sc.SUB_REMOVE)
    rij_k = np.ascontiguousarray(rij[:, kept])
    multi = engine.process_multi(list(data), FS, [T0] * 2, [rij, rij_k], [(None, None)], [sc.winlen(W)], 0.5, ests, prefiltered=True,
                                 want_beam=True)
    single = tb._process(np.ascontiguousarray(data[kept]), rij_k, W, 0.5)
    full = tb._process(data, rij, W, 0.5)
    for got, exp in ((multi[1], single), (multi[0], full)):
        for k in ('vel', 'baz', 'sigma_tau', 'beam_power', 'fstat'):
            np.testing.assert_array_equal(getattr(got, k), getattr(exp, k), err_msg=k)
    assert not np.array_equal(single.fstat, full.fstat)
    _beam_against_reference(single, data[kept], label='beam sub-array 30 of 32 W=%d' % W)
