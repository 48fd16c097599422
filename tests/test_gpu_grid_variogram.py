"""GPU: per-grid-cell variograms in one pass (rdr_cell_variogram, csrc/cell_variogram_kernels.h; raider_amd/variogram.py: grid_variograms).

Every stage is pinned on a yardstick that is not the code under test:
  a. deramp off, default bins: per cell the EXISTING pair_variogram (parent code, pinned by tests/test_gpu_variogram.py) on the cell's
     slice, with the values NaN-ed where the slice has fewer than min_valid valid stations - nvalid, count, hmax and edges identical bit
     for bit; lag_sum and gamma_sum within a relative (m + 4) * 2^-52 (m the bin's count: the bound of test_gpu_variogram.py) of math.fsum
     in a NumPy all-pairs restatement copied into this file.  Before a device result is looked at, NumPy alone asserts that no pair's h
     lies within a relative 1e-12 of any edge made from NumPy's own hmax.
  b. residuals: r* = the plane removal by CENTRED normal equations in np.longdouble (in this file).  e_ref = max|r_lstsq - r*| is how far
     the reference's own arithmetic - np.linalg.lstsq on uncentred UTM metres, raider_amd.variogram.deramp - lies from r* on the same
     slice; the device must satisfy max|r_dev - r*| <= max(4 e_ref, 8 ulp of max|v|) per slice.  Both distances are printed.
  c. binning with the plane removed: on the residuals the device returned, (a)'s bounds against the NumPy restatement.
  d. totals: the given-edges call equals the NumPy restatement in the per-cell rows over the status-0 slices, counts exact, sums within
     the bound with m the total count; skipped slices contribute nothing.
  e. golden g21 (tools/gen_golden_grid_variogram.py): the reference's own _append_variogram per cell.
  f. a cell of 12 collinear stations takes the host path (status 2) and equals station_variograms on that cell.
  g. the C ABI: every invalid argument is refused with the outputs untouched; two calls give identical counts.

Shapes: cells of 1, 2, 9, 10, 63, 64, 65, 255, 256, 257, 0 (an empty cell between full ones), 512 (the largest staged in LDS) and 513
(the first that runs from global memory; it ends exactly at n), all in ONE call; D = 1, 4, 5, 9 (date groups 1, 4, 4 + 1, 4 + 4 + 1; 2 and
3 in the ABI test); B = 1, 19, 64; a station missing on alternate dates, a date all NaN, a slice with one valid station, two stations at
one place; float32 values; host arrays, device pointers and tensors.
"""
import functools
import math
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import raider_amd as R                                     # noqa: E402
from raider_amd import _lib as L                           # noqa: E402
from raider_amd import variogram as V                      # noqa: E402

GOLDEN = Path(__file__).resolve().parent / 'golden' / 'g21_grid_variogram.npz'
SIZES = (1, 2, 9, 10, 63, 64, 65, 255, 256, 257, 0, 512, 513)
MIN_VALID = 10


# ---- the yardsticks (NumPy; copied from tests/test_gpu_variogram.py where they are the same) ---------------------------------------
def pair_lags(x, y):
    i, j = np.triu_indices(x.size, 1)
    dx = x[i] - x[j]; dy = y[i] - y[j]
    return i, j, np.sqrt(dx * dx + dy * dy)


def numpy_hmax(lags, v):
    i, j, h = lags
    out = np.full(v.shape[0], np.nan)
    for d in range(v.shape[0]):
        ok = ~np.isnan(v[d][i]) & ~np.isnan(v[d][j])
        if ok.any():
            out[d] = h[ok].max()
    return out


def numpy_variogram(lags, v, edges):
    """count, lag_sum, gamma_sum [D, B] of float64 values v [D, N] by the masks of statsPlot.py:644 and math.fsum; edges [1 or D, B + 1]"""
    i, j, h = lags
    D, B = v.shape[0], edges.shape[1] - 1
    count = np.zeros((D, B), dtype=np.int64); lag = np.zeros((D, B)); gam = np.zeros((D, B))
    for d in range(D):
        e = edges[d if edges.shape[0] > 1 else 0]
        ok = ~np.isnan(v[d][i]) & ~np.isnan(v[d][j])
        hd = h[ok]
        g = 0.5 * np.square(v[d][i][ok] - v[d][j][ok])
        for b in range(B):
            m = np.logical_and(e[b] < hd, hd <= e[b + 1])
            count[d, b] = m.sum(); lag[d, b] = math.fsum(hd[m]); gam[d, b] = math.fsum(g[m])
    return count, lag, gam


def assert_off_edges(h, edges):
    """the condition on the INPUTS that makes counts exact: no h within a relative 1e-12 of an edge (an edge of exactly 0 aside)"""
    if h.size:
        for e in np.unique(edges[np.isfinite(edges)]):
            if e != 0.0:
                assert np.abs(h - e).min() > 1e-12 * abs(e), f'the test inputs put a pair on the edge {e!r}'


def assert_sums(got_count, got_lag, got_gam, want, where=''):
    count, lag, gam = want
    assert got_count.dtype == np.int64 and np.array_equal(got_count, count), where
    tol = (count + 4) * 2.0 ** -52
    for got, ref, name in ((got_lag, lag, 'lag_sum'), (got_gam, gam, 'gamma_sum')):
        assert np.all(got[count == 0] == 0.0), (name, where)
        err = np.abs(got - ref)
        assert np.all(err <= tol * np.abs(ref)), (name, where, (err / np.maximum(np.abs(ref), 1e-300) / 2.0 ** -52).max(), count.max())


def same_bits(a, b):
    """NaN where the other is, and elsewhere the same bytes"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and a[~np.isnan(a)].tobytes() == b[~np.isnan(b)].tobytes()


def longdouble_residuals(x, y, v):
    """v [N] minus the least-squares plane over its valid entries: centred normal equations in np.longdouble"""
    ld = np.longdouble
    ok = ~np.isnan(v)
    xs, ys, vs = x[ok].astype(ld), y[ok].astype(ld), v[ok].astype(ld)
    dx, dy, dv = xs - xs.mean(), ys - ys.mean(), vs - vs.mean()
    sxx, sxy, syy, sxv, syv = (dx * dx).sum(), (dx * dy).sum(), (dy * dy).sum(), (dx * dv).sum(), (dy * dv).sum()
    det = sxx * syy - sxy * sxy
    a, b = (syy * sxv - sxy * syv) / det, (sxx * syv - sxy * sxv) / det
    out = np.full(v.shape, np.nan, dtype=ld)
    out[ok] = dv - (a * dx + b * dy)
    return out


# ---- the scene: thirteen cells in one call ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def geometry():
    """stations of the SIZES cells at distinct nodes of an integer-metre lattice, 40 km x 30 km per cell, sorted by cell; the pairs of
    every cell.  Shared by every case and never written to."""
    rng = np.random.default_rng(26)
    xs, ys = [], []
    for c, m in enumerate(SIZES):
        nodes = rng.choice(40000 * 30000, size=m, replace=False)
        x = (nodes % 40000).astype(np.float64) + 412000.0 + 50000.0 * (c % 4)
        y = (nodes // 40000).astype(np.float64) + 3765000.0 + 40000.0 * (c // 4)
        if m == 257:
            x[-1], y[-1] = x[0], y[0]                                   # two stations at one place
        xs.append(x); ys.append(y)
    start = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    x, y = np.concatenate(xs), np.concatenate(ys)
    lags = [pair_lags(x[start[c]:start[c + 1]], y[start[c]:start[c + 1]]) for c in range(len(SIZES))]
    for a in (x, y, start):
        a.setflags(write=False)
    return x, y, start, lags


@functools.lru_cache(maxsize=None)
def scene(nd, nbins, mv=MIN_VALID):
    """values with holes, and everything NumPy says about them (computed once per (D, B))"""
    x, y, start, lags = geometry()
    rng = np.random.default_rng(100 * nd + nbins)
    n = x.size
    v = 2.4 + 3e-7 * (x - x.mean()) - 2e-7 * (y - y.mean()) + 0.05 * rng.standard_normal((nd, n))
    v[::2, start[3] + 1] = np.nan                        # the 10-station cell: 9 valid on alternate dates (skipped), 10 on the others
    v[::2, start[5] + 7] = np.nan                        # a station of the 64-cell missing on alternate dates (still good)
    if nd >= 4:
        v[1, :] = np.nan                                 # a date all NaN
        v[2, start[6]:start[7]] = np.nan; v[2, start[6] + 30] = 1.0          # the 65-cell on date 2: one valid station
    nvalid = np.stack([(~np.isnan(v[:, start[c]:start[c + 1]])).sum(axis=1) for c in range(len(SIZES))])
    used = v.copy()                                      # what takes part: slices below min_valid are out
    for c in range(len(SIZES)):
        used[nvalid[c] < mv, start[c]:start[c + 1]] = np.nan
    hmax = np.stack([numpy_hmax(lags[c], used[:, start[c]:start[c + 1]]) for c in range(len(SIZES))])
    edges = np.stack([V.default_edges(hmax[c], nbins) for c in range(len(SIZES))])
    for c in range(len(SIZES)):
        assert_off_edges(lags[c][2], edges[c])
    v.setflags(write=False); used.setflags(write=False)
    return dict(v=v, used=used, nvalid=nvalid, hmax=hmax, edges=edges, status=(nvalid < mv).astype(np.int32))


def call(v, nbins, deramp=False, edges=None, residuals=False, totals=False, device=False, mv=MIN_VALID):
    x, y, start, _ = geometry()
    ctx = R.Context.default()
    if device:
        import torch
        dev = lambda a: None if a is None else torch.from_numpy(np.array(a)).cuda()
        o = V._cell_call(ctx, dev(x), dev(y), dev(start), dev(v), deramp, mv, dev(edges), nbins, residuals, totals, True)
        ctx.synchronize()
        return {k: (a.cpu().numpy() if a is not None else None) for k, a in o.items()}
    return V._cell_call(ctx, x, y, start, np.array(v), deramp, mv, edges, nbins, residuals, totals, False)


def check_binning(o, values, sc, nbins, where):
    """(a) / (c): counts exact, sums within the bound, against the NumPy restatement on `values` in rows made from NumPy's hmax"""
    x, y, start, lags = geometry()
    for c in range(len(SIZES)):
        sl = slice(start[c], start[c + 1])
        want = numpy_variogram(lags[c], values[:, sl], V._usable_rows(sc['edges'][c]))
        assert_sums(o['count'][c], o['lag_sum'][c], o['gamma_sum'][c], want, f'{where}, cell {c} of {SIZES[c]}')


CASES = [(1, 19, MIN_VALID), (4, 1, MIN_VALID), (5, 64, MIN_VALID), (9, 19, MIN_VALID), (4, 19, 1)]       # (min_valid 1: slices of ONE valid station run)


# ---- a. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nd, nbins, mv', CASES)
def test_a_no_deramp_default_edges_against_pair_variogram(nd, nbins, mv):
    x, y, start, lags = geometry()
    sc = scene(nd, nbins, mv)                                                 # (asserts the off-edge condition on the inputs first)
    o = call(sc['v'], nbins, mv=mv)
    assert np.array_equal(o['nvalid'], sc['nvalid']) and o['nvalid'].dtype == np.int64
    assert np.array_equal(o['status'], sc['status']) and (mv > 1 or (sc['nvalid'][sc['status'] == 0] == 1).any())
    for c, m in enumerate(SIZES):
        sl = slice(start[c], start[c + 1])
        if m >= 2:
            pv = V.pair_variogram(x[sl], y[sl], sc['used'][:, sl], nbins=nbins)
            assert same_bits(o['hmax'][c], pv.hmax), (c, m)
            assert same_bits(o['edges'][c], pv.edges), (c, m)
            assert np.array_equal(o['count'][c], pv.count), (c, m)
        else:
            assert np.isnan(o['hmax'][c]).all() and np.isnan(o['edges'][c]).all() and not o['count'][c].any()
    assert np.array_equal(np.isnan(o['hmax']), np.isnan(sc['hmax']))
    check_binning(o, sc['used'], sc, nbins, f'D{nd} B{nbins}')
    assert o['count'][11].sum() > 0 and o['count'][12].sum() > 0 and not o['count'][10].any()      # LDS, global, the empty cell between them


def test_a_device_pointers_give_the_same():
    sc = scene(5, 64)
    a = call(sc['v'], 64); b = call(sc['v'], 64, device=True)
    for k in ('nvalid', 'status', 'count'):
        assert np.array_equal(a[k], b[k]), k
    assert same_bits(a['hmax'], b['hmax']) and same_bits(a['edges'], b['edges'])
    check_binning(b, sc['used'], sc, 64, 'device pointers')
    again = call(sc['v'], 64)
    assert again['count'].tobytes() == a['count'].tobytes()                    # two identical calls: identical counts


# ---- b. and c. -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nd, nbins', [(5, 19), (9, 64)])
def test_b_c_residuals_and_their_binning(nd, nbins, capsys):
    x, y, start, lags = geometry()
    sc = scene(nd, nbins)
    o = call(sc['v'], nbins, deramp=True, residuals=True)
    assert np.array_equal(o['nvalid'], sc['nvalid'])
    want_status = sc['status']
    assert np.array_equal(o['status'], want_status)                           # (no singular plane in this scene: 10 scattered stations at least)
    r = o['residuals']
    worst_dev = worst_ref = worst_ratio = 0.0
    for c, m in enumerate(SIZES):
        sl = slice(start[c], start[c + 1])
        for d in range(nd):
            if want_status[c, d]:
                assert np.isnan(r[d, sl]).all() and np.isnan(o['hmax'][c, d]) and not o['count'][c, d].any()
                continue
            vs = sc['v'][d, sl]
            assert np.array_equal(np.isnan(r[d, sl]), np.isnan(vs))
            star = longdouble_residuals(x[sl], y[sl], vs)
            e_ref = float(np.nanmax(np.abs(V.deramp(x[sl], y[sl], vs) - star)))
            e_dev = float(np.nanmax(np.abs(r[d, sl] - star)))
            bound = max(4 * e_ref, 8 * np.spacing(np.nanmax(np.abs(vs))))
            worst_dev, worst_ref, worst_ratio = max(worst_dev, e_dev), max(worst_ref, e_ref), max(worst_ratio, e_dev / bound)
            assert e_dev <= bound, (c, m, d, e_dev, e_ref)
    with capsys.disabled():
        print(f'\n  residuals, D{nd}: largest distance from the long-double plane: device {worst_dev:.3g}, np.linalg.lstsq {worst_ref:.3g}; '
              f'device / bound at most {worst_ratio:.3g}', end='')
    # c. the residuals the device returned, binned in rows from NumPy's own hmax (validity is the values')
    check_binning(o, r, sc, nbins, f'deramp D{nd} B{nbins}')
    assert same_bits(o['edges'], sc['edges'])


# ---- d. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nd, nbins, device', [(5, 19, False), (9, 64, True), (4, 1, False)])
def test_d_totals_over_good_dates(nd, nbins, device):
    x, y, start, lags = geometry()
    sc = scene(nd, nbins)
    with np.errstate(invalid='ignore'):
        top = np.array([np.nanmax(h) if not np.isnan(h).all() else np.nan for h in sc['hmax']])
    rows = V._usable_rows(V.default_edges(top, nbins))
    for c in range(len(SIZES)):
        assert_off_edges(lags[c][2], rows[c])
    o = call(sc['v'], nbins, edges=rows, totals=True, device=device)
    assert np.array_equal(o['status'], sc['status'])
    assert o['edges'].tobytes() == np.repeat(rows[:, None, :], nd, axis=1).tobytes()
    ok = ~np.isnan(sc['hmax'])
    assert np.array_equal(np.isnan(o['hmax']), ~ok) and np.all(np.abs(o['hmax'][ok] - sc['hmax'][ok]) <= 2 * np.spacing(sc['hmax'][ok]))
    for c in range(len(SIZES)):
        sl = slice(start[c], start[c + 1])
        per = numpy_variogram(lags[c], sc['used'][:, sl], rows[c:c + 1])
        assert_sums(o['count'][c], o['lag_sum'][c], o['gamma_sum'][c], per, f'cell {c}')
        # all good dates together: one fsum over every pair of every date (any order of the dates' sums lies within the bound)
        i, j, h = lags[c]
        hs, gs = [], []
        for d in range(nd):
            u = sc['used'][d, sl]
            okp = ~np.isnan(u[i]) & ~np.isnan(u[j])
            hs.append(h[okp]); gs.append(0.5 * np.square(u[i][okp] - u[j][okp]))
        hs, gs = np.concatenate(hs), np.concatenate(gs)
        e = rows[c]
        masks = [np.logical_and(e[b] < hs, hs <= e[b + 1]) for b in range(nbins)]
        want = (np.array([m.sum() for m in masks], dtype=np.int64), np.array([math.fsum(hs[m]) for m in masks]), np.array([math.fsum(gs[m]) for m in masks]))
        assert_sums(o['total_count'][c], o['total_lag'][c], o['total_gamma'][c], want, f'totals, cell {c}')
        assert np.array_equal(o['total_count'][c], o['count'][c][o['status'][c] == 0].sum(axis=0))


# ---- e. the reference's own run --------------------------------------------------------------------------------------------------------
def test_e_against_the_reference(capsys):
    """g21: VariogramAnalysis._append_variogram of the reference per cell (3 x 2 cells of 0, 9, 10, 12, 30, 45 stations, 5 dates; every
    slice kept all its pairs).  Good and skipped slices, edges, counts and sparse_grids agree exactly; hmax within 2 ulp (printed);
    hExp / vExp within a relative 1e-9; the total fit per parameter within 10 x fit_spread and the rmse within 10 x its spread (+ 4 ulp:
    the sqrt and the mean round, too) - the rule and the constant of tests/test_gpu_variogram.py for g20; the maps are NaN exactly where
    the reference's are.  The metres the reference worked in are the package's own device transform of lon / lat: checked first."""
    g = np.load(GOLDEN)
    gv = V.grid_variograms(g['lon'], g['lat'], g['values'])
    sg = gv.grid
    assert np.array_equal(sg.cell, g['gridnode'])
    assert gv.x.tobytes() == g['x'][sg.order].tobytes() and gv.y.tobytes() == g['y'][sg.order].tobytes()
    state = g['slice_state']
    good = state == 1
    assert np.array_equal(gv.status == 0, good)
    assert sorted(gv.skipped_slices) == sorted(map(tuple, g['skipped_slices'].tolist()))
    assert gv.sparse_grids == g['sparse_grids'].tolist()
    ulps = np.abs(gv.hmax[good] - g['slice_hmax'][good]) / np.spacing(g['slice_hmax'][good])
    with capsys.disabled():
        print(f'\n  g21 hmax: largest difference from the reference {ulps.max():g} ulp', end='')
    assert np.all(ulps <= 2) and np.isnan(gv.hmax[~good]).all()
    assert gv.edges[good].tobytes() == g['slice_edges'][good].tobytes()
    assert np.array_equal(gv.count[good], g['slice_count'][good]) and not gv.count[~good].any()
    for c, d in zip(*np.nonzero(good)):
        h, gam = gv.binned(c, d)
        keep = g['slice_count'][c, d] > 0
        assert np.all(np.abs(h - g['slice_hexp'][c, d][keep]) <= 1e-9 * h) and np.all(np.abs(gam - g['slice_vexp'][c, d][keep]) <= 1e-9 * gam)
    cells = np.flatnonzero(good.any(axis=1))
    assert cells.tolist() == g['tot_grids'].tolist()
    assert gv.total_edges[cells].tobytes() == g['tot_edges'][cells].tobytes()
    assert np.array_equal(gv.total_count[cells], g['tot_count'][cells]) and g['tot_count'][cells].sum() > 5000
    for c in cells:
        h, gam = gv.total_binned(c)
        keep = g['tot_count'][c] > 0
        assert np.all(np.abs(h - g['tot_hexp'][c][keep]) <= 1e-9 * h) and np.all(np.abs(gam - g['tot_vexp'][c][keep]) <= 1e-9 * gam)
        assert np.all(np.abs(gv.params[c] - g['tot_fit'][c]) <= 10 * g['tot_fit_spread'][c]), (c, gv.params[c], g['tot_fit'][c], g['tot_fit_spread'][c])
        assert abs(gv.rmse[c] - g['tot_rmse'][c]) <= 10 * g['tot_rmse_spread'][c] + 4 * np.spacing(g['tot_rmse'][c]), (c, gv.rmse[c], g['tot_rmse'][c])
    rest = np.setdiff1d(np.arange(6), cells)
    assert np.isnan(gv.params[rest]).all() and np.isnan(gv.rmse[rest]).all()
    for got, want in ((gv.grid_range, g['map_range']), (gv.grid_variance, g['map_variance']), (gv.grid_variogram_rmse, g['map_rmse'])):
        assert got.shape == want.shape == (2, 3) and np.array_equal(np.isnan(got), np.isnan(want))
        assert np.allclose(got[~np.isnan(want)], want[~np.isnan(want)], rtol=1e-6, atol=0)
    assert np.isnan(V.grid_variograms(g['lon'], g['lat'], g['values'], errlimit=1e-9, binned=True).rmse).all()      # (:810-814)


# ---- f. and the routes of the Python layer -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def network():
    """two 1-degree cells of UTM zone 11: 40 scattered stations, and 12 on the zone's central meridian - one line in metres"""
    rng = np.random.default_rng(7)
    lon = np.concatenate([rng.uniform(-118.9, -118.1, 40), np.full(12, -117.0)])
    lat = np.concatenate([rng.uniform(33.1, 33.9, 40), np.sort(rng.uniform(33.1, 33.9, 12))])
    v = 2.3 + 0.04 * (lon + 118.0) + 0.02 * rng.standard_normal((3, 52))
    v[1, 5] = np.nan
    return lon, lat, v


def test_f_collinear_cell_takes_the_host_path():
    lon, lat, v = network()
    gv = V.grid_variograms(lon, lat, v, fit=False)
    sg = gv.grid
    assert sg.grid_dim == [2, 1] and np.diff(sg.start).tolist() == [40, 12]
    assert gv.status.tolist() == [[0, 0, 0], [2, 2, 2]]
    line = sg.order[sg.start[1]:]
    sv = V.station_variograms(lon[line], lat[line], v[:, line], fit=False)
    assert gv.x[40:].tobytes() == sv.x.tobytes()
    pv = sv.variogram
    assert np.array_equal(gv.count[1], pv.count) and pv.count.sum() > 100
    assert same_bits(gv.hmax[1], pv.hmax) and same_bits(gv.edges[1], pv.edges) and np.isfinite(pv.edges).all()
    tol = 2 * (pv.count + 4) * 2.0 ** -52                     # each of the two lies within (a)'s bound of the exact sum
    assert np.all(np.abs(gv.lag_sum[1] - pv.lag_sum) <= tol * pv.lag_sum) and np.all(np.abs(gv.gamma_sum[1] - pv.gamma_sum) <= tol * pv.gamma_sum)
    # the patched residuals reach the totals: the cell's total counts are its three dates' pairs in the cell's own row
    lags = pair_lags(sv.x, sv.y)
    r = V.deramp(sv.x, sv.y, v[:, line])
    assert_off_edges(lags[2], gv.total_edges[1:2])
    want = numpy_variogram(lags, r, gv.total_edges[1:2])
    assert np.array_equal(gv.total_count[1], want[0].sum(axis=0))
    assert gv.sparse_grids == [] and gv.skipped_slices == []


def test_routes_arrays_tensors_and_float32():
    import torch
    lon, lat, v = network()
    v32 = v.astype(np.float32)
    a = V.grid_variograms(lon, lat, v32, fit=False)
    b = V.grid_variograms(lon, lat, v32.astype(np.float64), fit=False)
    t = V.grid_variograms(torch.from_numpy(lon).cuda(), torch.from_numpy(lat).cuda(), torch.from_numpy(v32).cuda(), fit=False)
    for k in ('count', 'lag_sum', 'gamma_sum', 'edges', 'hmax', 'nvalid', 'total_count', 'total_lag', 'total_gamma', 'total_edges'):
        assert isinstance(getattr(a, k), np.ndarray) and torch.is_tensor(getattr(t, k)) and getattr(t, k).is_cuda, k
    assert t.count.dtype == torch.int64 and t.lag_sum.dtype == torch.float64
    for other in (b, t):
        host = lambda q: q.cpu().numpy() if torch.is_tensor(q) else q
        assert np.array_equal(a.count, host(other.count)) and np.array_equal(a.total_count, host(other.total_count))
        assert same_bits(a.hmax, host(other.hmax)) and same_bits(a.edges, host(other.edges))
        assert np.allclose(a.lag_sum, host(other.lag_sum), rtol=1e-12, atol=0) and np.allclose(a.gamma_sum, host(other.gamma_sum), rtol=1e-12, atol=0)
    assert a.count.sum() > 0 and np.array_equal(a.status, t.status)
    h, gam = t.total_binned(0)
    assert torch.is_tensor(h) and h.numel() == int((a.total_count[0] > 0).sum())
    f = V.grid_variograms(lon, lat, v, per_date_fits=True)
    assert np.isfinite(f.params).all() and np.isfinite(f.rmse).all() and f.grid_range.shape == (1, 2)
    assert sorted(f.date_fits) == [(c, d) for c in range(2) for d in range(3)] and f.date_fits[(0, 0)].params.shape == (3,)


# ---- g. the C ABI ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loc', [L.RDR_HOST, L.RDR_DEVICE], ids=['host', 'device'])
def test_g_refusals_leave_the_outputs_untouched(loc):
    import torch
    ctx = R.Context.default()
    n, nd, nb, nc = 7, 3, 4, 3
    rng = np.random.default_rng(3)
    host = dict(x=np.array([0.0, 3.0, 1.0, 7.0, 2.0, 9.0, 4.0]), y=np.array([0.0, 1.0, 5.0, 2.0, 8.0, 3.0, 6.0]), v=rng.standard_normal((nd, n)),
                cs=np.array([0, 4, 4, 7], dtype=np.int64), cs_first=np.array([1, 4, 4, 7], dtype=np.int64), cs_last=np.array([0, 4, 4, 6], dtype=np.int64),
                cs_down=np.array([0, 5, 4, 7], dtype=np.int64), edges=np.tile(np.linspace(0.25, 12.25, nb + 1), (nc, 1)),
                bad_edges=np.tile(np.linspace(0.25, 12.25, nb + 1), (nc, 1)), inf_edges=np.tile(np.linspace(0.25, 12.25, nb + 1), (nc, 1)),
                nvalid=np.full((nc, nd), -7, dtype=np.int64), hmax=np.full((nc, nd), -7.0), status=np.full((nc, nd), -7, dtype=np.int32),
                count=np.full((nc, nd, nb), -7, dtype=np.int64), lag=np.full((nc, nd, nb), -7.0), gam=np.full((nc, nd, nb), -7.0),
                eout=np.full((nc, nd, nb + 1), -7.0), resid=np.full((nd, n), -7.0), tc=np.full((nc, nb), -7, dtype=np.int64),
                tl=np.full((nc, nb), -7.0), tg=np.full((nc, nb), -7.0))
    host['bad_edges'][2, 3] = host['bad_edges'][2, 2]; host['inf_edges'][1, 4] = np.inf
    if loc == L.RDR_DEVICE:
        bufs = {k: torch.from_numpy(a).cuda() for k, a in host.items()}
        torch.cuda.synchronize()
        read = lambda k: bufs[k].cpu().numpy()
    else:
        bufs = {k: a.copy() for k, a in host.items()}
        read = lambda k: bufs[k]
    p = lambda k: None if k is None else L.ptr(bufs[k])

    def cv(x='x', cs='cs', v='v', n_=n, nc_=nc, nd_=nd, deramp=0, mv=2, e='edges', nb_=nb, nvalid='nvalid', count='count', resid=None,
           tc='tc', tl='tl', tg='tg', loc_=loc):
        return ctx.lib.rdr_cell_variogram(ctx.handle, p(x), p('y'), n_, p(cs), nc_, p(v), nd_, deramp, mv, p(e), nb_, p(nvalid), p('hmax'), p('status'),
                                          p(count), p('lag'), p('gam'), p('eout'), p(resid), p(tc), p(tl), p(tg), loc_)
    for kw, text in ((dict(x=None), 'NULL argument'), (dict(cs=None), 'NULL argument'), (dict(v=None), 'NULL argument'), (dict(nvalid=None), 'NULL argument'),
                     (dict(count=None), 'NULL argument'), (dict(n_=1), 'n must be 2 .. 2^20 points (got 1)'), (dict(n_=(1 << 20) + 1), 'n must be 2'),
                     (dict(nd_=0), 'nd must be 1 .. 4096 dates (got 0)'), (dict(nd_=4097), 'nd must be 1 .. 4096 dates (got 4097)'),
                     (dict(nb_=0), 'nbins must be 1 .. 64 (got 0)'), (dict(nb_=65), 'nbins must be 1 .. 64 (got 65)'),
                     (dict(nc_=0), 'ncells must be 1 .. 2^20 cells (got 0)'), (dict(mv=-1), 'min_valid must not be negative (got -1)'),
                     (dict(deramp=2), 'deramp must be 0 or 1 (got 2)'), (dict(resid='resid'), 'residuals are written only with deramp = 1'),
                     (dict(tl=None), 'come together or not at all'), (dict(e=None), 'totals need given edges'),
                     (dict(cs='cs_first'), 'cell_start[0] must be 0 (got 1)'), (dict(cs='cs_last'), 'cell_start[ncells] must be n = 7 (got 6)'),
                     (dict(cs='cs_down'), 'cell_start is not ascending at index 2'),
                     (dict(e='bad_edges'), 'edge row 2 is not strictly ascending at index 3'), (dict(e='inf_edges'), 'edge row 1 holds a value that is not finite'),
                     (dict(loc_=2), 'loc must be RDR_HOST or RDR_DEVICE'), (dict(loc_=-1), 'loc must be RDR_HOST or RDR_DEVICE')):
        assert cv(**kw) == L.RDR_ERR_INVALID, kw
        assert text in L.last_error(ctx.handle), (text, L.last_error(ctx.handle))
    ctx.synchronize()
    outs = ('nvalid', 'hmax', 'status', 'count', 'lag', 'gam', 'eout', 'resid', 'tc', 'tl', 'tg')
    for k in outs:                                                  # the sentinels are still there
        assert np.array_equal(read(k), host[k]), k
    # and the same buffers make valid calls: given rows with totals; then default rows with the plane removed (D = 3: the groups 2 + 1)
    assert cv() == L.RDR_OK
    ctx.synchronize()
    lags = [pair_lags(host['x'][a:b], host['y'][a:b]) for a, b in ((0, 4), (4, 4), (4, 7))]
    for c, (a, b) in enumerate(((0, 4), (4, 4), (4, 7))):
        want = numpy_variogram(lags[c], host['v'][:, a:b], host['edges'][c:c + 1])
        assert_sums(read('count')[c], read('lag')[c], read('gam')[c], want)
        assert np.array_equal(read('tc')[c], want[0].sum(axis=0))
    assert np.array_equal(read('nvalid'), [[4] * 3, [0] * 3, [3] * 3]) and np.array_equal(read('status'), [[0] * 3, [1] * 3, [0] * 3])
    first = read('count').copy()
    assert cv() == L.RDR_OK
    ctx.synchronize()
    assert read('count').tobytes() == first.tobytes()
    assert cv(deramp=1, mv=3, e=None, resid='resid', tc=None, tl=None, tg=None) == L.RDR_OK
    ctx.synchronize()
    r = read('resid')
    for a, b in ((0, 4), (4, 7)):
        star = np.stack([longdouble_residuals(host['x'][a:b], host['y'][a:b], host['v'][d, a:b]) for d in range(nd)])
        assert np.abs(r[:, a:b] - star).max() <= 1e-13
    assert np.array_equal(read('status'), [[0] * 3, [1] * 3, [0] * 3])
    hm = np.array([lags[0][2].max(), np.nan, lags[2][2].max()])
    assert np.array_equal(read('hmax'), np.repeat(hm[:, None], 3, axis=1), equal_nan=True)
    assert read('eout')[0, 0].tobytes() == np.linspace(0, hm[0] * 0.67, nb + 1).tobytes() and np.isnan(read('eout')[1]).all()
