"""CPU reference of the refinement of the slowness-grid maximum between grid points (``nbls_set_beam_grid_refinement``;
DESIGN.md section 28), written from the definition of include/nbls.h and nothing else, on tests/steer_truth.py:

(a) ``replay(grid_point, step, path)``: the centres of every level in float64 — ``e = ldexp(step, -l)``, ``s_j = (c0 + a e0,
    c1 + b e1)`` with ``a = j // 3 - 1``, ``b = j % 3 - 1``, one rounded addition per axis; ``j = 4`` leaves the centre as it is;
(b) per level the long-double F, P and bounds of the 8 non-centre candidates by ``steer_truth.cell`` (``level_cells``);
(c) ``check_cell``, which judges the GPU's own trail level by level from the GPU's own centre.

The bounds are those of steer_truth: derived, none fitted.  The chosen j* is accepted if
``F(j*) + tol(j*) >= max_j (F(j) - tol(j))`` and must equal the truth's leader where that one leads by more than both bounds
(the rule of ``grid_truth.check_window``); the centre takes the value and the tolerance of the candidate chosen on the level
before (on level 1: of the grid point).  A level with a candidate whose bound is ``power_only`` (or whose F is not finite) is
skipped for the path check only; ``check_cell`` returns how many levels it skipped.

``greedy64`` is the float64 restatement of the whole search (steer_truth's operation order for x, NumPy's sums): what the
CPU tests and the demonstration run, not a reference for bits."""
import numpy as np

import steer_truth as stt

CENTRE = 4
MAX_LEVELS = 12


def offsets(j):
    """Candidate j -> (a, b)."""
    return j // 3 - 1, j % 3 - 1


def candidates(c, step, level):
    """The nine slowness vectors of a level around the centre ``c`` -> (9, 2) float64; row 4 is computed like the others (it
    is never evaluated)."""
    c = np.asarray(c, dtype=np.float64)
    e = np.ldexp(np.asarray(step, dtype=np.float64), -int(level))
    out = np.empty((9, 2))
    for j in range(9):
        a, b = offsets(j)
        out[j, 0] = c[0] + np.float64(a) * e[0]
        out[j, 1] = c[1] + np.float64(b) * e[1]
    return out


def replay(grid_point, step, path):
    """(a) -> the centres (R + 1, 2) float64: row 0 the grid point, row l the centre after level l.  A path of -1 (no grid
    maximum) gives NaN everywhere."""
    path = np.asarray(path, dtype=np.int64)
    out = np.full((len(path) + 1, 2), np.nan)
    if np.all(path < 0):
        return out
    assert np.all((path >= 0) & (path <= 8)), path
    out[0] = np.asarray(grid_point, dtype=np.float64)
    for l, j in enumerate(path, start=1):
        out[l] = out[l - 1] if j == CENTRE else candidates(out[l - 1], step, l)[j]
    return out


def reach(grid_point, step, levels):
    """The bound of |c - grid point| per axis: step (1 - 2^-R) of the exact sums, and one rounding of each of the R additions
    (2^-53 relative to a centre that is no larger than |grid point| + step) — derived, not fitted."""
    g, step = np.abs(np.asarray(grid_point, dtype=np.float64)), np.asarray(step, dtype=np.float64)
    return step * (1.0 - 2.0 ** -levels) + levels * 2.0 ** -53 * (g + step) + 2.0 ** -52 * step


def delays_of(xij, s, fs, N):
    """-> (n (N,) int64, mu (N,) float64) of the slowness ``s``: tau_0 = 0, the pairs (0, i) the first N - 1 co-array rows."""
    tau = np.concatenate(([0.0], stt.taus_of(np.asarray(xij)[:N - 1], s, fs)))
    assert np.all(np.abs(tau) < 2.0 ** 30)
    return stt.split(tau)


def cell_at(filt, fs, xij, s0, W, taps, s):
    """(b) for one slowness: ``steer_truth.cell``'s dict."""
    n, mu = delays_of(xij, s, fs, len(filt))
    return stt.cell(filt, int(s0), int(W), n, mu, taps)


def level_cells(filt, fs, xij, s0, W, taps, c, step, level):
    """(b) -> the list of nine cells of a level (entry 4 None: the centre is not evaluated)."""
    cand = candidates(c, step, level)
    return [None if j == CENTRE else cell_at(filt, fs, xij, s0, W, taps, cand[j]) for j in range(9)]


def fstat64(filt, fs, xij, s0, W, taps, s):
    """F and P of one slowness in float64: x in the contract's operation order (``steer_truth.rows64``), NumPy's sums."""
    filt = np.asarray(filt, dtype=np.float64)
    N = len(filt)
    n, mu = delays_of(xij, s, fs, N)
    x = stt.rows64(filt, int(s0), int(W), n, stt.coefficients(taps, mu))
    b = x.sum(axis=0)
    S_b, S_t = np.dot(b, b), np.sum(x * x)
    if np.isnan(S_b) or np.isnan(S_t) or S_t == 0.0:
        return np.nan, (np.nan if np.isnan(S_b) or np.isnan(S_t) else 0.0)
    D = N * S_t - S_b
    P = S_b / (np.float64(N) * N * W)
    return (np.inf if D <= 0.0 and S_b > 0.0 else (N - 1.0) * S_b / D), P


def choose(F, Fc):
    """j* under "F descending (+inf first); the centre before any other candidate; then j ascending"; NaN is no candidate.
    ``F``: the nine values (entry 4 ignored), ``Fc``: the centre's."""
    best, fbest = CENTRE, Fc
    for j in range(9):
        if j != CENTRE and F[j] > fbest:
            best, fbest = j, F[j]
    return best


def greedy64(evaluate, grid_point, F0, P0, step, levels):
    """The search of the definition with ``evaluate(s) -> (F, P)`` -> dict: ``slowness`` (2,), ``fstat``, ``power``, ``path``
    (R,) int32, ``stencil`` (9,), ``centres`` (R + 1, 2)."""
    c, Fc, Pc = np.array(grid_point, dtype=np.float64), F0, P0
    path, centres, stencil = [], [c.copy()], np.full(9, np.nan)
    for l in range(1, levels + 1):
        cand = candidates(c, step, l)
        vals = [(Fc, Pc) if j == CENTRE else evaluate(cand[j]) for j in range(9)]
        F = [v[0] for v in vals]
        j = choose(F, Fc)
        path.append(j)
        if l == levels:
            stencil = np.array(F, dtype=np.float64)
        if j != CENTRE:
            c, Fc, Pc = cand[j].copy(), vals[j][0], vals[j][1]
        centres.append(c.copy())
    return dict(slowness=c, fstat=Fc, power=Pc, path=np.array(path, dtype=np.int32), stencil=stencil, centres=np.array(centres))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _within(got, c, label):
    """One value against one truth cell's F: NaN where NaN, large where +inf, within the bound where finite."""
    F, tol = c['fstat'], c['tol_fstat']
    if np.isnan(F):
        assert np.isnan(got), (label, got)
    elif not np.isfinite(F):
        assert got > 1e6, (label, got)
    else:
        assert not np.isnan(got) and (abs(got - F) <= tol), (label, got, F, tol)


def check_cell(filt, fs, xij, s0, W, taps, grid_point, step, levels, grid_fstat, slowness, fstat, power, path, stencil, label=''):
    """(c): assert the refined results of one (row, window) whose grid maximum is ``grid_point`` (``grid_index >= 0``) ->
    (levels skipped for the path check, worst |dF| / bound of the compared values)."""
    path = np.asarray(path)
    assert path.shape == (levels,) and np.all((path >= 0) & (path <= 8)), (label, path)
    centres = replay(grid_point, step, path)
    assert same_bits(slowness, centres[-1]), (label, slowness, centres[-1])        # bit-equal to the replay
    assert np.all(np.abs(centres[-1] - np.asarray(grid_point)) <= reach(grid_point, step, levels)), (label, centres[-1], grid_point)
    assert fstat >= grid_fstat or (np.isnan(fstat) and np.isnan(grid_fstat)), (label, fstat, grid_fstat)
    if np.all(path == CENTRE):
        assert same_bits(fstat, grid_fstat), (label, fstat, grid_fstat)
    centre = cell_at(filt, fs, xij, s0, W, taps, grid_point)                       # value and tolerance of the level before
    skipped, worst = 0, 0.0
    for l in range(1, levels + 1):
        cells = level_cells(filt, fs, xij, s0, W, taps, centres[l - 1], step, l)
        cells[CENTRE] = centre
        j = int(path[l - 1])
        assert not np.isnan(cells[j]['fstat']), (label, l, j)                      # a NaN F is no candidate
        cand = [k for k in range(9) if not np.isnan(cells[k]['fstat'])]
        if any(cells[k]['power_only'] for k in cand):
            skipped += 1
        else:
            F = np.array([cells[k]['fstat'] for k in cand])
            tol = np.array([cells[k]['tol_fstat'] for k in cand])
            assert cells[j]['fstat'] + cells[j]['tol_fstat'] >= np.max(F - tol), (label, l, j, cells[j]['fstat'], np.max(F - tol))
            lead = choose([cells[k]['fstat'] if k in cand else np.nan for k in range(9)], centre['fstat'])
            others = [k for k in cand if k != lead]
            if not others or cells[lead]['fstat'] - cells[lead]['tol_fstat'] > max(cells[k]['fstat'] + cells[k]['tol_fstat'] for k in others):
                assert j == lead, (label, l, j, lead)                              # the truth's leader leads by more than both bounds
        if l == levels:
            for k in range(9):
                _within(stencil[k], cells[k], (label, 'stencil', k))
                if np.isfinite(cells[k]['fstat']) and np.isfinite(cells[k]['tol_fstat']) and cells[k]['tol_fstat'] > 0:
                    worst = max(worst, abs(stencil[k] - cells[k]['fstat']) / cells[k]['tol_fstat'])
        centre = cells[j]
    _within(fstat, centre, (label, 'fstat'))
    if not np.isnan(centre['power']):
        assert abs(power - centre['power']) <= centre['tol_power'], (label, power, centre['power'], centre['tol_power'])
    if np.isfinite(centre['fstat']) and np.isfinite(centre['tol_fstat']) and centre['tol_fstat'] > 0:
        worst = max(worst, abs(fstat - centre['fstat']) / centre['tol_fstat'])
    return skipped, worst


def check_row(filt, fs, xij, W, inc, nwin, taps, grid, step, levels, grid_index, grid_fstat, refined, first=0, label=''):
    """(c) for the windows [first, first + nwin) of one result row; ``refined``: the five arrays of the fetch, cut to the row
    -> (levels skipped, levels in all, worst |dF| / bound).  A window without a grid maximum: NaN and -1."""
    slow, fstat, power, path, stencil = refined
    skipped = total = 0
    worst = 0.0
    for k in range(nwin):
        w = first + k
        if grid_index[w] < 0:
            assert np.all(np.isnan(slow[w])) and np.isnan(fstat[w]) and np.isnan(power[w]) and np.all(np.isnan(stencil[w])), (label, w)
            assert np.all(path[w] == -1), (label, w, path[w])
            continue
        s, wr = check_cell(filt, fs, xij, w * int(inc), W, taps, np.asarray(grid)[grid_index[w]], step, levels, grid_fstat[w], slow[w],
                           fstat[w], power[w], path[w], stencil[w], label='%s window %d' % (label, w))
        skipped, total, worst = skipped + s, total + levels, max(worst, wr)
    return skipped, total, worst


# ---- the cases of the GPU test against the truth (tests/test_gpu_grid_refine.py), and what the CPU test checks of them ----
FS = 20.0
AXIS = np.array([-3.07, -1.535, 0.0, 1.535, 3.07])
GRID5 = np.array([[a, b] for a in AXIS for b in AXIS])            # 5 x 5 points, s = 0 among them; step 1.535 s/km
GRID3 = GRID5.reshape(5, 5, 2)[::2, ::2].reshape(-1, 2)           # 3 x 3 points, step 3.07 s/km
# (N, W, taps, levels, noise only, grid): every N of {3, 4, 8, 9, 32}, W of {16, 255, 256, 257, 513}, tap count and level
# count of {1, 2, 5, 12}; the trace ends one sample behind its last window, so the first and the last windows read taps off
# both ends
CASES = [(3, 16, 4, 12, True, 'GRID5'), (4, 255, 6, 5, False, 'GRID5'), (8, 256, 8, 2, False, 'GRID5'), (9, 257, 4, 1, True, 'GRID3'),
         (32, 513, 8, 1, False, 'GRID3'), (4, 513, 6, 2, True, 'GRID5'), (8, 257, 8, 5, False, 'GRID5'), (3, 256, 6, 12, False, 'GRID3'),
         (9, 16, 8, 5, True, 'GRID5'), (32, 255, 4, 2, False, 'GRID3')]
GRIDS = dict(GRID5=GRID5, GRID3=GRID3)


def case_inputs(N, W, noise, seed=None):
    """The trace of a case -> (data (N, npts), rij centred, inc): a plane wave at 6 dB over an array of 300 m, or noise alone,
    four windows at half overlap and one sample more."""
    from narrow_band_least_squares_amd import planner, synthetic
    inc = int(planner.window_plan(10 ** 6, FS, (W + 0.5) / FS, 0.5)[1])
    npts = W + 3 * inc + 1
    seed = 700 + N + W if seed is None else seed
    rij = synthetic.array_geometry(N, 0.15)
    if noise:
        data = np.random.default_rng(seed).standard_normal((N, npts))
    else:
        data = synthetic.plane_wave(rij, npts, FS, 0.5, 4.0, baz_deg=60.0, snr_db=6.0, seed=seed)
    return np.ascontiguousarray(data), rij - rij.mean(axis=1, keepdims=True), inc


def lattice_step(grid):
    from narrow_band_least_squares_amd import planner
    return planner.grid_cells(grid)[1]
