"""Designed lattices for the family labelling: every case is a dict with the request ``par`` and the
arguments of ``families_truth.label`` / ``Handle.label_families``.  Values come from small sets of exactly representable
numbers, so every compare is exact on both sides."""
import numpy as np

PAR = dict(mdccm_min=0.5, vel_min=0.2, vel_max=0.6, sigma_tau_max=None, baz_tol=5.0, vel_tol=0.03125, band_reach=1, time_reach=1,
           min_pixels=1)
BAZ_SET = np.array([10.0, 14.0, 18.0, 200.0, 204.0, 355.0, 359.0, 1.0])
VEL_SET = np.array([0.3125, 0.34375, 0.375, 0.5])


def nwin_of(winlen, wininc, npts):
    return np.array([(npts - W) // i + 1 for W, i in zip(winlen, wininc)], dtype=np.int32)


def case(name, par, winlen, wininc, nwin, vel, baz, mdccm, sigma_tau=None, nseg=1):
    vel, baz, mdccm = (np.ascontiguousarray(g, dtype=np.float64) for g in (vel, baz, mdccm))
    if sigma_tau is not None:
        sigma_tau = np.ascontiguousarray(sigma_tau, dtype=np.float64)
    return dict(name=name, par=dict(PAR, **par), nseg=nseg, winlen=np.asarray(winlen, dtype=np.int32),
                wininc=np.asarray(wininc, dtype=np.int32), nwin=np.asarray(nwin, dtype=np.int32), vel=vel, baz=baz, mdccm=mdccm,
                sigma_tau=sigma_tau)


def from_mask(name, par, winlen, wininc, mask, nwin=None, baz=10.0, vel=0.34375, nseg=1):
    """Eligible where ``mask``; everything else has an MdCCM below the gate."""
    mask = np.asarray(mask, dtype=bool)
    rows, vl = mask.shape
    return case(name, par, winlen, wininc, np.full(rows, vl) if nwin is None else nwin, np.full(mask.shape, vel),
                np.broadcast_to(np.asarray(baz, dtype=np.float64), mask.shape), np.where(mask, 0.75, 0.25), nseg=nseg)


def random_case(name, par, winlen, wininc, nwin, vl, density, seed, nseg=1, baz_set=BAZ_SET, vel_set=VEL_SET):
    rng = np.random.default_rng(seed)
    rows = len(winlen) * nseg
    ok = rng.random((rows, vl)) < density
    return case(name, par, winlen, wininc, nwin, rng.choice(vel_set, (rows, vl)), rng.choice(baz_set, (rows, vl)),
                np.where(ok, rng.choice([0.5, 0.625, 0.75, 0.875], (rows, vl)), 0.25), nseg=nseg)


def window_mix(band_reach, time_reach):
    """3 bands of different window length and hop over 1200 samples."""
    W, inc = [40, 60, 200], [20, 30, 50]
    nwin = nwin_of(W, inc, 1200)
    # few values, so that the components are large and cross the bands
    c = random_case('mix_b%d_t%d' % (band_reach, time_reach), dict(band_reach=band_reach, time_reach=time_reach, min_pixels=2), W, inc,
                    nwin, int(nwin.max()), 0.6, 100 + 10 * band_reach + time_reach)
    c['baz'] = np.where(c['baz'] < 100.0, 10.0, np.where(c['baz'] < 300.0, 200.0, 14.0))
    return c


def serpentine():
    """8 x 300: the even bands full, the odd bands one cell at alternating ends.  One component; its smallest cell is more
    than 1000 links from its far end."""
    m = np.zeros((8, 300), dtype=bool)
    m[0::2] = True
    m[1, 299] = m[5, 299] = m[3, 0] = m[7, 0] = True
    return from_mask('serpentine', {}, [40] * 8, [20] * 8, m)


def spiral(nb=13, vl=41):
    """A rectangular spiral of pitch 2 that starts in the last band and winds inwards: the walk reaches band 0, where the
    component's smallest cell (the root) lies, only after the whole last band and a whole column, so the hooks made before
    that all have to be carried on towards it."""
    m = np.zeros((nb, vl), dtype=bool)
    inside = lambda b, w: 0 <= b < nb and 0 <= w < vl
    dirs = [(0, 1), (-1, 0), (0, -1), (1, 0)]                       # along the band, up, back, down
    b, w, d = nb - 1, 0, 0
    m[b, w] = True
    moved = True
    while moved:
        moved = False
        for turn in (0, 1):
            db, dw = dirs[(d + turn) % 4]
            if inside(b + db, w + dw) and not m[b + db, w + dw] and not (inside(b + 2 * db, w + 2 * dw) and m[b + 2 * db, w + 2 * dw]):
                d, b, w = (d + turn) % 4, b + db, w + dw
                m[b, w] = moved = True
                break
    return from_mask('spiral', {}, [40] * nb, [20] * nb, m)


def exact_edges():
    """One band, time_reach 1; groups separated by a cell below the MdCCM gate.  Expected components are in ``expect``."""
    lo = np.nextafter(0.5, 0.0)
    v = 0.34375
    groups = [  # (baz, vel, mdccm, sigma) per cell
        [(10.0, v, 0.75, 0.0), (15.0, v, 0.75, 0.0)],                       # 5.0 apart, tol 5.0: linked
        [(10.0, v, 0.75, 0.0), (15.5, v, 0.75, 0.0)],                       # 5.5 apart: not
        [(359.0, v, 0.75, 0.0), (1.0, v, 0.75, 0.0)],                       # 358 -> 2.0 <= 5.0: linked
        [(10.0, v, 0.5, 0.0), (10.0, v, lo, 0.0), (10.0, v, 0.75, 0.0)],   # mdccm == mdccm_min is eligible, one ulp less is not
        [(10.0, 0.2, 0.75, 0.0), (10.0, 0.6, 0.75, 0.0)],                   # the velocity bounds are inclusive; 0.4 apart: not linked
        [(10.0, np.nextafter(0.2, 0.0), 0.75, 0.0), (10.0, np.nextafter(0.6, 1.0), 0.75, 0.0)],      # just outside
        [(np.nan, v, 0.75, 0.0), (10.0, np.nan, 0.75, 0.0), (10.0, v, np.nan, 0.0), (10.0, v, 0.75, np.nan)],
        [(np.inf, v, 0.75, 0.0), (10.0, np.inf, 0.75, 0.0), (10.0, v, np.inf, 0.0), (10.0, v, 0.75, np.inf)],
        [(10.0, -np.inf, 0.75, 0.0), (-np.inf, v, 0.75, 0.0), (10.0, v, -np.inf, 0.0), (10.0, v, 0.75, 1.0), (10.0, v, 0.75, 1.5)],
        [(10.0, v, 0.75, -np.inf), (10.0, v, 0.75, 0.0)],                   # -inf passes the sigma gate
    ]
    cells = []
    for g in groups:
        cells += g + [(10.0, v, 0.25, 0.0)]
    a = np.array(cells).T
    n = a.shape[1]
    c = case('exact_edges', dict(sigma_tau_max=1.0), [40], [20], [n], a[1][None], a[0][None], a[2][None], a[3][None])
    sizes, k = [], 0
    for g in groups:
        sizes.append((k, len(g)))
        k += len(g) + 1
    c['groups'] = sizes
    return c


def wrap_tol2():
    """359.0 / 1.0 with tol exactly 2.0 links; 358.5 / 1.0 does not."""
    baz = np.array([[359.0, 1.0, 50.0, 358.5, 1.0]])
    mask = np.array([[True, True, False, True, True]])
    return from_mask('wrap_tol2', dict(baz_tol=2.0), [40], [20], mask, baz=baz)


def vel_tol_zero():
    """vel_tol = 0: equal values link, one ulp apart does not."""
    v = 0.34375
    c = from_mask('vel_tol_zero', dict(vel_tol=0.0), [40], [20], np.array([[True, True, False, True, True]]))
    c['vel'] = np.array([[v, v, v, v, np.nextafter(v, 1.0)]])
    return c


def beyond_nwin():
    """Zeros beyond nwin would pass every gate of this request, and do not count."""
    z = np.zeros((2, 8))
    return case('beyond_nwin', dict(mdccm_min=0.0, vel_min=0.0, baz_tol=0.0, vel_tol=0.0), [40, 80], [20, 40], [5, 3], z, z, z)


def min_pixels_case():
    """Runs of 3, 4 and 5 cells under min_pixels = 4."""
    m = np.zeros((1, 16), dtype=bool)
    m[0, 0:3] = m[0, 4:8] = m[0, 9:14] = True
    return from_mask('min_pixels', dict(min_pixels=4), [40], [20], m)


def degenerate():
    none = from_mask('no_family', {}, [40, 40], [20, 20], np.zeros((2, 70), dtype=bool))
    one = from_mask('one_family', {}, [40, 40], [20, 20], np.ones((2, 70), dtype=bool))
    own = from_mask('own_family', dict(baz_tol=0.0), [40, 40], [20, 20], np.ones((2, 70), dtype=bool),
                    baz=np.arange(140, dtype=np.float64).reshape(2, 70))
    return [none, one, own]


def cell_counts():
    out = []
    for n in (63, 64, 65, 255, 256, 257):
        out.append(random_case('cells_%d' % n, dict(min_pixels=2), [40], [20], [n], n, 0.7, n, baz_set=BAZ_SET[:3]))
    # 2 bands x 32 769 windows, the second band one window short: 65 537 cells with a window, past one scan block squared
    out.append(random_case('cells_65537', dict(min_pixels=2), [40, 40], [20, 20], [32769, 32768], 32769, 0.9, 65537,
                           baz_set=BAZ_SET[:2], vel_set=VEL_SET[:3]))
    return out


def segments():
    """nseg = 3 with identical grids: three disjoint copies of the families."""
    W, inc = [40, 60, 200], [20, 30, 50]
    c = random_case('segments', dict(min_pixels=2, band_reach=2), W, inc, nwin_of(W, inc, 1200), 59, 0.6, 7)
    for k in ('vel', 'baz', 'mdccm', 'nwin'):
        c[k] = np.ascontiguousarray(np.repeat(c[k], 3, axis=0))      # row b * 3 + s = band b of every recording
    c['baz'] = np.where(c['baz'] < 100.0, 10.0, 200.0)
    c['nseg'] = 3
    return c


def random_grids():
    W, inc = [40, 40, 60, 60, 120, 200], [20, 20, 30, 30, 40, 50]
    nwin = nwin_of(W, inc, 2000)
    out = []
    for density in (0.3, 0.6, 0.9):
        c = random_case('random_%d' % round(10 * density), dict(min_pixels=3, sigma_tau_max=0.5), W, inc, nwin, int(nwin.max()) + 3, density,
                        int(100 * density))
        c['baz'] = np.where(c['baz'] < 100.0, c['baz'], 14.0)               # 10 / 14 / 18: chains of agreeing neighbours
        c['sigma_tau'] = np.random.default_rng(5).choice([0.25, 0.5, 0.75], c['vel'].shape, p=[0.6, 0.3, 0.1])
        out.append(c)
    return out


def all_cases():
    out = [window_mix(b, t) for b in (0, 1, 2) for t in (1, 2, 3)]
    out += [serpentine(), spiral(), exact_edges(), wrap_tol2(), vel_tol_zero(), beyond_nwin(), min_pixels_case()]
    out += degenerate() + cell_counts() + [segments()] + random_grids()
    return out


def args_of(c):
    return (c['par'], c['nseg'], c['winlen'], c['wininc'], c['nwin'], c['vel'], c['baz'], c['mdccm'], c['sigma_tau'])
