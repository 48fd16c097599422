#!/usr/bin/env python3
"""tests/golden/g21_grid_variogram.npz: the reference's own per-grid-cell variogram chain (cli/statsPlot.py
VariogramAnalysis._append_variogram, :721-844, driven WHOLE per cell on a pandas DataFrame, matplotlib on the Agg backend, a
temporary workdir) and RaiderStats._get_extent (:1291-1368), recorded on a scene small enough that every slice keeps EVERY pair.

Two stages, because the reference's WGS84_to_UTM needs PROJ, which is absent, and the metres the package works in come from its
device transform:

    python tools/gen_golden_grid_variogram.py --metres-out metres.npz          (on a GPU: raider_amd.variogram.utm_common_center
                                                                                of the scene's lon / lat; nothing of the reference)
    python tools/gen_golden_grid_variogram.py --metres metres.npz [--out ...]  (no GPU: the reference run)

In the second stage RAiDER.cli.statsPlot.WGS84_to_UTM is replaced at run time by a look-up of those metres (recorded in `_meta`);
everything else that runs is the reference's code: _emp_vario (the lstsq plane, _get_samples, _get_XY, _get_distances,
_get_variogram), _binned_vario, _fit_vario, the TOT binning and fit, the rmse and the errlimit rule, sparse_grids, skipped_slices.
_binned_vario and _fit_vario are wrapped only to RECORD their arguments and results.  The reference is imported through
oracle/refharness/ref_import.import_reference() with an empty placeholder for shapely.strtree, as tools/gen_golden_variogram.py does.
The harness's shapely stand-in has no Polygon.intersects: _get_extent is recorded with bbox = None only, and the bbox branch is pinned
by a restatement in tests/test_grid_variogram_host.py.  Stations are assigned to the reference's gridpoints by containment in
centre +- spacing / 2 (the reference uses an R-tree; the stations lie off every cell edge, so there is one answer).

The scene: a 3 x 2 grid of 1-degree cells (lon -118 .. -115, lat 33 .. 35, UTM zone 11) holding 0, 9, 10, 12, 30 and 45 stations at
integer-metre UTM lattice nodes mapped back to lon / lat; 5 dates; one station of the 10-station cell is missing on dates 0 and 2 (the
cell is skipped there and good on dates 1 and 3); date 4 is all NaN (no rows at all).  45 stations are 990 pairs, fewer than the 1000
at which _get_samples starts to drop pairs: the tool asserts that every slice kept all its pairs, and - with NumPy alone - that no
pair distance lies within a relative 1e-12 of any edge it records.

Recorded: lon, lat, x, y, values [5, N], gridnode [N]; ext<s>_extent / _grid_dim / _gridpoints for spacings 0.5, 1, 2 (s = 05, 1, 2);
slice_state [G, D] (0 no rows, 1 good, 2 skipped), slice_hmax, slice_edges [G, D, 20], slice_count [G, D, 19], slice_hexp / slice_vexp
[G, D, 19] (NaN for an empty bin); per cell tot_edges, tot_count, tot_hexp, tot_vexp, tot_fit [G, 3], tot_rmse [G], tot_fit_spread
[G, 3] and tot_rmse_spread [G] (the largest |change| over 32 fits whose binned input was perturbed by a relative 1e-12, as g20 defines
it); sparse_grids, skipped_slices [(cell, date index)], tot_grids; map_range, map_variance, map_rmse [ny, nx] by :3302-3337.
"""
import argparse
import json
import random
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CELLS = {(0, 1): 0, (0, 0): 9, (1, 1): 10, (1, 0): 12, (2, 1): 30, (2, 0): 45}        # (ix from the west, iy from the south): stations
W, S, NB, ND = -118.0, 33.0, 19, 5


def scene():
    from oracle import raider_oracle as O
    rng = np.random.default_rng(21)
    lon, lat = [], []
    for (ix, iy), k in CELLS.items():
        lo = rng.uniform(W + ix + 0.06, W + ix + 0.94, k); la = rng.uniform(S + iy + 0.06, S + iy + 0.94, k)
        x, y = O.tm_forward(la, lo, lon_0=-117.0)
        la2, lo2 = O.tm_inverse(np.round(x), np.round(y), lon_0=-117.0)                 # integer-metre lattice nodes of zone 11
        # (the committed g21 was made when the oracle rounded k_0 A one ulp differently - k_0 (a / (1 + n) (...)): a regeneration may move
        # lon / lat, and with them everything recorded, by an ulp; stage 1, the device's metres of the NEW lon / lat, has to be redone too)
        lon.append(lo2); lat.append(la2)
    lon, lat = np.concatenate(lon), np.concatenate(lat)
    perm = rng.permutation(lon.size)                                                    # stations do not come sorted by cell
    lon, lat = lon[perm], lat[perm]
    n = lon.size
    v = 2.4 + 0.03 * (lon[None, :] + 116.5) - 0.02 * (lat[None, :] - 34.0) + 0.01 * rng.standard_normal((ND, n)) \
        + 0.02 * np.sin(7.0 * lon[None, :] + np.arange(ND)[:, None]) * np.cos(5.0 * lat[None, :])
    in10 = np.flatnonzero((np.floor(lon - W) == 1) & (np.floor(lat - S) == 1))
    assert in10.size == 10
    v[0::2, in10[3]] = np.nan
    v[4, :] = np.nan
    return lon, lat, v


def reference_module():
    import matplotlib
    matplotlib.use('Agg')
    from oracle.refharness import ref_import
    ref_import.import_reference()
    if 'shapely.strtree' not in sys.modules:
        try:
            import shapely.strtree  # noqa: F401
        except ImportError:
            m = types.ModuleType('shapely.strtree')
            m.STRtree = type('STRtree', (), {})
            sys.modules['shapely.strtree'] = m
    import RAiDER.cli.statsPlot as sp
    return sp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--metres-out')
    ap.add_argument('--metres')
    ap.add_argument('--out', default=str(ROOT / 'tests' / 'golden' / 'g21_grid_variogram.npz'))
    a = ap.parse_args()
    lon, lat, v = scene()
    if a.metres_out:
        from raider_amd import variogram as V
        x, y = V.utm_common_center(lon, lat)
        Path(a.metres_out).parent.mkdir(parents=True, exist_ok=True)
        np.savez(a.metres_out, lon=lon, lat=lat, x=x, y=y)
        print(a.metres_out, 'metres of', lon.size, 'stations')
        return
    if not a.metres:
        ap.error('--metres FILE (written by --metres-out on a GPU) is needed for the reference run')
    m = np.load(a.metres)
    assert np.array_equal(m['lon'], lon) and np.array_equal(m['lat'], lat), 'the metres file belongs to another scene'
    x, y = m['x'], m['y']
    metres = {(lo, la): (xx, yy) for lo, la, xx, yy in zip(lon, lat, x, y)}

    import pandas as pd
    sp = reference_module()

    def utm_lookup(lo, la, common_center=False):
        xy = np.array([metres[(p, q)] for p, q in zip(lo, la)])
        return None, None, xy[:, 0], xy[:, 1]
    sp.WGS84_to_UTM = utm_lookup

    dates = pd.to_datetime(['2020-01-01', '2020-01-13', '2020-01-25', '2020-02-06', '2020-02-18'])
    out = dict(lon=lon, lat=lat, x=x, y=y, values=v)
    # the grid, for three spacings
    rows = [dict(ID=f'S{i:03d}', Lon=lon[i], Lat=lat[i], Date=dates[d], ZTD=v[d, i]) for d in range(ND) for i in range(lon.size) if not np.isnan(v[d, i])]
    df = pd.DataFrame(rows)
    for tag, s in (('05', 0.5), ('1', 1), ('2', 2)):
        rs = object.__new__(sp.RaiderStats)
        rs.df, rs.bbox, rs.spacing = df, None, s
        extent, grid_dim, gridpoints = rs._get_extent()
        out[f'ext{tag}_spacing'] = np.float64(rs.spacing)           # (2 does not divide the 3 degrees of longitude: the reference resets it to 1)
        out[f'ext{tag}_extent'] = np.array(extent, dtype=np.float64); out[f'ext{tag}_grid_dim'] = np.array(grid_dim, dtype=np.int64)
        out[f'ext{tag}_gridpoints'] = np.array(gridpoints, dtype=np.float64)
        if s == 1:
            gp, gdim = np.array(gridpoints, dtype=np.float64), grid_dim
    ng = len(gp)
    inside = (np.abs(lon[:, None] - gp[None, :, 0]) < 0.5) & (np.abs(lat[:, None] - gp[None, :, 1]) < 0.5)
    assert (inside.sum(axis=1) == 1).all()
    node = inside.argmax(axis=1)
    out['gridnode'] = node.astype(np.int64)
    assert sorted(np.bincount(node, minlength=ng).tolist()) == sorted(CELLS.values())
    df['gridnode'] = [int(node[int(i[1:])]) for i in df['ID']]

    workdir = tempfile.mkdtemp(prefix='g21_')
    va = sp.VariogramAnalysis(df, [list(p) for p in gp], 'ZTD', workdir=workdir)
    va.TOT_good_slices = []; va.TOT_res_robust_arr = []; va.TOT_res_robust_rmse = []; va.TOT_tot_timetag = []
    va.sparse_grids = []; va.good_slices = []; va.skipped_slices = []; va.gridcenterlist = []
    log = []
    binned_ref, fit_ref = va._binned_vario, va._fit_vario

    def binned_rec(h, g, xBin=None):
        r = binned_ref(h, g, xBin)
        log.append(('binned', np.array(h), np.array(g), r))
        return r

    def fit_rec(*aa, **kk):
        r = fit_ref(*aa, **kk)
        log.append(('fit', r[0].x.copy(), r[0].fun.copy()))
        return r
    va._binned_vario, va._fit_vario = binned_rec, fit_rec

    state = np.zeros((ng, ND), dtype=np.int64); hmax = np.full((ng, ND), np.nan)
    edges = np.full((ng, ND, NB + 1), np.nan); count = np.zeros((ng, ND, NB), dtype=np.int64)
    hexp = np.full((ng, ND, NB), np.nan); vexp = np.full((ng, ND, NB), np.nan)
    tot_edges = np.full((ng, NB + 1), np.nan); tot_count = np.zeros((ng, NB), dtype=np.int64)
    tot_hexp = np.full((ng, NB), np.nan); tot_vexp = np.full((ng, NB), np.nan)
    tot_fit = np.full((ng, 3), np.nan); tot_rmse = np.full(ng, np.nan); tot_spread = np.full((ng, 3), np.nan); rmse_spread = np.full(ng, np.nan)

    def place(h, r):
        e = np.linspace(0, np.nanmax(h) * 0.67, NB + 1)                                 # (:638)
        c = np.array([np.logical_and(e[b] < h, h <= e[b + 1]).sum() for b in range(NB)], dtype=np.int64)
        assert (c > 0).sum() == len(r[0]) == len(r[1])
        for ee in e[e != 0.0]:
            assert np.abs(h - ee).min() > 1e-12 * ee, 'a pair distance lies on an edge'
        hh = np.full(NB, np.nan); vv = np.full(NB, np.nan)
        hh[c > 0] = r[0]; vv[c > 0] = r[1]
        return e, c, hh, vv

    random.seed(21)
    for g in sorted(set(df['gridnode'])):
        sub = df[df['gridnode'] == g]
        log.clear()
        nskip = len(va.skipped_slices)
        va._append_variogram(g, sub)
        for _, day in va.skipped_slices[nskip:]:
            state[g, list(dates.strftime('%Y-%m-%d')).index(day)] = 2
        good = [list(dates.strftime('%Y%m%d')).index(day) for gg, day in va.good_slices if gg == g]
        calls = [c for c in log if c[0] == 'binned']
        fits = [c for c in log if c[0] == 'fit']
        assert len(calls) == len(fits) == (len(good) + 1 if good else 0)
        for d, c in zip(good, calls):
            nv = int((~np.isnan(v[d, node == g])).sum())
            assert len(c[1]) == nv * (nv - 1) // 2, 'the reference dropped pairs'
            state[g, d] = 1
            hmax[g, d] = np.nanmax(c[1])
            edges[g, d], count[g, d], hexp[g, d], vexp[g, d] = place(c[1], c[3])
        if good:
            c = calls[-1]
            assert len(c[1]) == sum(int(count_pairs) for count_pairs in [len(k[1]) for k in calls[:-1]])
            tot_edges[g], tot_count[g], tot_hexp[g], tot_vexp[g] = place(c[1], c[3])
            tot_fit[g] = fits[-1][1]
            assert np.allclose(tot_fit[g], va.TOT_res_robust_arr[-1], rtol=0, atol=0)
            tot_rmse[g] = float(va.TOT_res_robust_rmse[-1])
            prng = np.random.default_rng(2100 + g)
            h0, v0 = c[3]
            sp_x = np.zeros(3); sp_r = 0.0
            for _ in range(32):
                hp = h0 * (1 + 1e-12 * prng.uniform(-1, 1, h0.size)); vp = v0 * (1 + 1e-12 * prng.uniform(-1, 1, v0.size))
                rp, _, _ = fit_ref(hp, vp, model=va.__exponential__, x0=None, Nparm=3)
                sp_x = np.maximum(sp_x, np.abs(rp.x - tot_fit[g]))
                sp_r = max(sp_r, abs(float(np.sqrt(np.nanmean(rp.fun ** 2))) - tot_rmse[g]))
            tot_spread[g], rmse_spread[g] = sp_x, sp_r
            print(f'cell {g}: good dates {good}, fit {tot_fit[g]}, rmse {tot_rmse[g]:.6g}, spread {sp_x / np.abs(tot_fit[g])} (relative), rmse spread {sp_r:.3g}')
    tot_grids = [i[0] for i in va.TOT_good_slices]
    maps = {}
    for name, src in (('range', [r[0] for r in va.TOT_res_robust_arr]), ('variance', [r[1] for r in va.TOT_res_robust_arr]), ('rmse', va.TOT_res_robust_rmse)):
        maps[name] = np.array([np.nan if i not in tot_grids else float(src[tot_grids.index(i)]) for i in range(ng)]).reshape(gdim).T       # (:3302-3337)
    day_index = {d: k for k, d in enumerate(dates.strftime('%Y-%m-%d'))}
    out.update(slice_state=state, slice_hmax=hmax, slice_edges=edges, slice_count=count, slice_hexp=hexp, slice_vexp=vexp, tot_edges=tot_edges,
               tot_count=tot_count, tot_hexp=tot_hexp, tot_vexp=tot_vexp, tot_fit=tot_fit, tot_rmse=tot_rmse, tot_fit_spread=tot_spread,
               tot_rmse_spread=rmse_spread, sparse_grids=np.array(va.sparse_grids, dtype=np.int64),
               skipped_slices=np.array([[g, day_index[d]] for g, d in va.skipped_slices], dtype=np.int64).reshape(-1, 2),
               tot_grids=np.array(tot_grids, dtype=np.int64), map_range=maps['range'], map_variance=maps['variance'], map_rmse=maps['rmse'],
               density_threshold=np.int64(va.densitythreshold))
    import scipy
    from oracle.refharness import ref_import
    out['_meta'] = np.array(json.dumps(dict(
        ref_import.provenance(), numpy=np.__version__, scipy=scipy.__version__, pandas=pd.__version__,
        route='VariogramAnalysis._append_variogram driven whole, per cell; _binned_vario and _fit_vario wrapped to record',
        utm='RAiDER.cli.statsPlot.WGS84_to_UTM replaced at run time by a look-up of raider_amd.variogram.utm_common_center metres (device transform; PROJ absent)',
        bbox='_get_extent recorded with bbox=None only: the shapely stand-in has no Polygon.intersects',
        generator='tools/gen_golden_grid_variogram.py, companion of oracle/refharness/gen_golden.py')))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(a.out, **out)
    print(a.out, Path(a.out).stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
