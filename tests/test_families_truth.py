"""The truth of the family labelling (tests/families_truth.py) against a second, independent statement of the definition
(DESIGN.md section 26): a dense adjacency matrix over every pair of eligible cells, the four link conditions written out
with broadcasting, and ``scipy.sparse.csgraph.connected_components`` (a transitive closure without SciPy); the designed
cases' own expectations; and the demonstration of section 26.4 on the oracle's rows.  CPU only."""
import numpy as np
import pytest

import families_cases as fc
import families_truth as ft

try:
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import connected_components, shortest_path
except ImportError:                                    # pragma: no cover
    csr_matrix = None

CASES = fc.all_cases()
DENSE_MAX = 3000          # eligible cells up to which the dense matrix is formed
TRUTH = {c['name']: ft.label(*fc.args_of(c)) for c in CASES}


def _dense(c):
    """-> (eligible cells ascending, bool adjacency (U, U)) straight from the four conditions."""
    par, nseg = c['par'], c['nseg']
    rows, vl = c['vel'].shape
    cell = np.arange(rows * vl)
    r, w = cell // vl, cell % vl
    b, s = r // nseg, r % nseg
    with np.errstate(invalid='ignore'):
        ok = w < c['nwin'][r]
        for g in ('vel', 'baz', 'mdccm'):
            ok &= np.isfinite(c[g].reshape(-1))
        ok &= c['mdccm'].reshape(-1) >= par['mdccm_min']
        ok &= (par['vel_min'] <= c['vel'].reshape(-1)) & (c['vel'].reshape(-1) <= par['vel_max'])
        if par['sigma_tau_max'] is not None:
            ok &= c['sigma_tau'].reshape(-1) <= par['sigma_tau_max']
    u = cell[ok]
    inc = c['wininc'].astype(np.int64)[b[u]]
    c2 = 2 * w[u] * inc + c['winlen'].astype(np.int64)[b[u]]
    baz, vel = c['baz'].reshape(-1)[u], c['vel'].reshape(-1)[u]
    A = s[u][:, None] == s[u][None, :]
    A &= np.abs(b[u][:, None] - b[u][None, :]) <= par['band_reach']
    A &= np.abs(c2[:, None] - c2[None, :]) <= 2 * par['time_reach'] * np.maximum(inc[:, None], inc[None, :])
    d = np.abs(baz[:, None] - baz[None, :])
    d = np.where(d > 180.0, 360.0 - d, d)
    A &= (d <= par['baz_tol']) & (np.abs(vel[:, None] - vel[None, :]) <= par['vel_tol'])
    np.fill_diagonal(A, False)
    return u, A


def _components(A):
    if csr_matrix is not None:
        return connected_components(csr_matrix(A), directed=False)[1]
    R = A | np.eye(len(A), dtype=bool)
    while True:
        R2 = (R.astype(np.int32) @ R.astype(np.int32)) > 0
        if (R2 == R).all():
            return np.unique(R, axis=0, return_inverse=True)[1].reshape(-1)
        R = R2


def _family_from_labels(c, u, lab):
    """Component labels of the eligible cells -> (family, nfamilies, first cells, counts) by the definition's numbering."""
    rows, vl = c['vel'].shape
    fam = np.full(rows * vl, -1, dtype=np.int32)
    first = {}
    for cell, k in zip(u.tolist(), lab.tolist()):
        first.setdefault(k, cell)
    count = np.bincount(lab, minlength=len(first)) if len(u) else np.zeros(0, dtype=int)
    keep = sorted(first[k] for k in first if count[k] >= c['par']['min_pixels'])
    ident = {f: i for i, f in enumerate(keep)}
    for cell, k in zip(u.tolist(), lab.tolist()):
        fam[cell] = ident.get(first[k], -2)
    return fam.reshape(rows, vl), len(keep), np.array(keep, dtype=np.int64), np.array([count[k] for k in first if first[k] in ident])


@pytest.mark.parametrize('c', [c for c in CASES if c['vel'].size <= DENSE_MAX], ids=lambda c: c['name'])
def test_truth_equals_the_dense_statement(c):
    fam, n, tab = TRUTH[c['name']]
    u, A = _dense(c)
    efam, en, first, count = _family_from_labels(c, u, _components(A) if len(u) else np.zeros(0, dtype=int))
    assert n == en and np.array_equal(fam, efam)
    assert np.array_equal(tab[:, 1], first) and sorted(tab[:, 0]) == sorted(count)
    # the table against the members, column by column
    rows, vl = fam.shape
    for k in range(n):
        mem = np.flatnonzero(fam.reshape(-1) == k)
        r, w = mem // vl, mem % vl
        b = r // c['nseg']
        md = c['mdccm'].reshape(-1)[mem]
        s0 = w * c['wininc'].astype(np.int64)[b]
        assert tab[k].tolist() == [len(mem), mem[0], mem[np.flatnonzero(md == md.max())[0]], b.min(), b.max(), r[0] % c['nseg'],
                                   s0.min(), (s0 + c['winlen'][b]).max()]
        assert len(set((r % c['nseg']).tolist())) == 1


def test_uniform_lattice_of_65537_cells_against_offset_adjacency():
    """Two bands of one window length and hop, band_reach = time_reach = 1: the links are the eight lattice neighbours whose
    values agree — a sparse adjacency built from the offsets, no candidate ranges."""
    c = next(c for c in CASES if c['name'] == 'cells_65537')
    fam, n, tab = TRUTH[c['name']]
    rows, vl = c['vel'].shape
    ok = ft.eligible_cells(c['par'], c['nwin'], c['vel'], c['baz'], c['mdccm'])
    ii, jj = [], []
    idx = np.arange(rows * vl).reshape(rows, vl)
    for db in (0, 1):
        for dw in (-1, 0, 1):
            if (db, dw) <= (0, 0):
                continue
            a = idx[:rows - db, max(0, -dw):vl - max(0, dw)]
            b = idx[db:, max(0, dw):vl - max(0, -dw)]
            m = ok.reshape(-1)[a] & ok.reshape(-1)[b] & ft.values_agree(c['par'], c['baz'].reshape(-1)[a], c['vel'].reshape(-1)[a],
                                                                        c['baz'].reshape(-1)[b], c['vel'].reshape(-1)[b])
            ii.append(a[m]); jj.append(b[m])
    ii, jj = np.concatenate(ii), np.concatenate(jj)
    lab = connected_components(csr_matrix((np.ones(len(ii), dtype=bool), (ii, jj)), shape=(rows * vl, rows * vl)), directed=False)[1]
    u = np.flatnonzero(ok.reshape(-1))
    efam, en, first, _ = _family_from_labels(c, u, np.unique(lab[u], return_inverse=True)[1])
    assert n == en == 2106 and np.array_equal(fam, efam) and np.array_equal(tab[:, 1], first)
    assert n > 256 and rows * vl > 256 * 256


def test_designed_expectations():
    fam, n, tab = TRUTH['serpentine']
    assert n == 1 and tab[0].tolist()[:6] == [1204, 0, 0, 0, 7, 0]
    u, A = _dense(next(c for c in CASES if c['name'] == 'serpentine'))
    dist = shortest_path(csr_matrix(A), unweighted=True, indices=0)
    assert dist.max() >= 1000                          # the smallest cell is that many links from the far end
    fam, n, tab = TRUTH['spiral']
    c = next(c for c in CASES if c['name'] == 'spiral')
    assert n == 1 and tab[0, 1] == 0 and tab[0, 3] == 0 and tab[0, 4] == 12 and tab[0, 0] == (c['mdccm'] > 0.5).sum()
    u, A = _dense(c)
    start = np.flatnonzero(u == 12 * 41)[0]            # the walk starts in the last band ...
    assert shortest_path(csr_matrix(A), unweighted=True, indices=start)[0] >= 12 + 40     # ... and meets cell 0 a band and a column later
    fam, n, tab = TRUTH['exact_edges']
    c = next(c for c in CASES if c['name'] == 'exact_edges')
    got = [fam[0, k:k + m].tolist() for k, m in c['groups']]
    assert got == [[0, 0], [1, 2], [3, 3], [4, -1, 5], [6, 7], [-1, -1], [-1] * 4, [-1] * 4, [-1, -1, -1, 8, -1], [9, 9]]
    assert TRUTH['wrap_tol2'][0].tolist() == [[0, 0, -1, 1, 2]]
    assert TRUTH['vel_tol_zero'][0].tolist() == [[0, 0, -1, 1, 2]]
    fam, n, tab = TRUTH['beyond_nwin']
    assert n == 1 and (fam >= 0).sum() == 8 and (fam[0, 5:] == -1).all() and (fam[1, 3:] == -1).all()
    fam, n, tab = TRUTH['min_pixels']
    assert fam[0].tolist() == [-2] * 3 + [-1] + [0] * 4 + [-1] + [1] * 5 + [-1, -1] and tab[:, 0].tolist() == [4, 5]
    assert TRUTH['no_family'][1] == 0 and (TRUTH['no_family'][0] == -1).all()
    assert TRUTH['one_family'][1] == 1 and (TRUTH['one_family'][0] == 0).all()
    assert TRUTH['own_family'][1] == 140 and np.array_equal(TRUTH['own_family'][0].reshape(-1), np.arange(140))
    fam, n, tab = TRUTH['segments']
    f3 = fam.reshape(3, 3, -1)
    assert n % 3 == 0 and n > 0
    for s in (1, 2):                                   # three disjoint copies: the same partition in every recording
        a, b = f3[:, 0].reshape(-1), f3[:, s].reshape(-1)
        assert np.array_equal(a < 0, b < 0) and np.array_equal(a[a < 0], b[b < 0])
        assert len(set(zip(a[a >= 0].tolist(), b[b >= 0].tolist()))) == n // 3
        assert not set(a[a >= 0].tolist()) & set(b[b >= 0].tolist())
    assert sorted(tab[:, 5].tolist()) == sorted([0, 1, 2] * (n // 3))


def test_the_peak_tie_goes_to_the_smallest_cell_and_signed_zeros_are_equal():
    z = np.zeros((1, 4))
    par = dict(fc.PAR, mdccm_min=-1.0, vel_min=0.0, baz_tol=0.0, vel_tol=0.0)
    md = np.array([[0.25, 0.75, 0.75, 0.5]])
    assert ft.label(par, 1, [40], [20], [4], z, z, md)[2][0, 2] == 1
    md = np.array([[-0.5, -0.0, 0.0, -0.25]])
    assert ft.label(par, 1, [40], [20], [4], z, z, md)[2][0, 2] == 1


# ---- the demonstration on the oracle's rows ----

import families_demo as demo


@pytest.fixture(scope='module')
def oracle_rows(oracle):
    out = {}
    for name, (sources, seed) in demo.RECORDINGS.items():
        st = oracle.make_stream(demo.traces(sources, seed), demo.FS, starttime=demo.T0)
        out[name] = oracle.narrow_band_least_squares(*demo.call_args(st), rij=demo.RIJ)
    return out


def test_demonstration_on_the_oracle_rows(oracle_rows):
    vel, baz, mdccm, t, _, sig, nwin = oracle_rows['signal'][:7]
    fam, n, tab = ft.label(demo.PAR, 1, demo.W, demo.INC, nwin, vel, baz, mdccm)
    demo.check_signal(fam, tab, vel, baz, mdccm, sig)
    vel, baz, mdccm, t, _, sig, nwin = oracle_rows['noise'][:7]
    assert ft.label(demo.PAR, 1, demo.W, demo.INC, nwin, vel, baz, mdccm)[1] == 0
