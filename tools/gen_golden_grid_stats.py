#!/usr/bin/env python3
"""tests/golden/g22_grid_stats.npz: the reference's own gridded station statistics - `RaiderStats(csv, 'ZTD', grid_heatmap=True, ...all
seven maps...)` (cli/statsPlot.py:946-1289), whose constructor runs `create_DF` (:1423-1794) WHOLE on a CSV this tool writes: the
pandas reader, dropna, `_get_extent`, the station -> cell assignment and the two groupby passes behind every map.

    python tools/gen_golden_grid_stats.py [--out ...]          (no GPU; needs pandas and the reference)

The reference is imported through oracle/refharness/ref_import.import_reference().  Its R-tree (shapely.strtree.STRtree) is absent;
before RAiDER.cli.statsPlot is imported this tool places a stand-in of its own in sys.modules['shapely.strtree'] whose `query`
answers by containment in the cell's rectangle (the harness's Polygon keeps the vertex array in .bounds[0], its Point the coordinates
in .coords[0]).  The stations lie off every cell edge, so containment has one answer.

The scene: the 3 x 2 grid of g21 (lon -118 .. -115, lat 33 .. 35), 1-degree cells holding 0, 1, 2, 3, 5 and 10 stations that have rows,
9 dates, about 30 % holes.  One further station has no row at all - it is absent from the CSV, and present in lon / lat / ids / values
(an all-NaN column), in the interior so that the extent does not hang on it.  The station that is alone in its cell has a single row:
the cell has a mean and a NaN stdev.  The tool asserts that a cell with an even and one with an odd total row count exist.

Recorded: ids, lon, lat [N]; dates [D] (datetime64[D] as int64 days); values [D, N] REBUILT FROM THE REFERENCE'S DATAFRAME (o.df), i.e.
as pandas parsed them - its default float parser moves some values by an ulp against what was written -; for spacings 1 and 0.5
(tags s1, s05): <tag>_plotbbox, <tag>_grid_dim, <tag>_spacing and the seven maps <tag>_grid_heatmap ... <tag>_grid_delay_absolute_stdev.
"""
import argparse
import json
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

CELLS = {(0, 1): 0, (0, 0): 1, (1, 1): 2, (1, 0): 10, (2, 1): 3, (2, 0): 5}          # (ix from the west, iy from the south): stations with rows
W, S, ND = -118.0, 33.0, 9
MAPS = ('grid_heatmap', 'grid_delay_mean', 'grid_delay_median', 'grid_delay_stdev', 'grid_delay_absolute_mean', 'grid_delay_absolute_median',
        'grid_delay_absolute_stdev')


def scene():
    rng = np.random.default_rng(22)
    lon, lat, lone = [], [], None
    for (ix, iy), k in CELLS.items():
        # off every edge of the 1-degree AND the half-degree cells
        lo = W + ix + rng.choice([0.0, 0.5], k) + rng.uniform(0.06, 0.44, k); la = S + iy + rng.choice([0.0, 0.5], k) + rng.uniform(0.06, 0.44, k)
        if k == 1:
            lone = len(np.concatenate(lon)) if lon else 0
        lon.append(lo); lat.append(la)
    lon.append(np.array([-116.27])); lat.append(np.array([33.71]))                     # the station without a row
    lon, lat = np.concatenate(lon), np.concatenate(lat)
    n = lon.size
    rowless = n - 1
    perm = rng.permutation(n)                                                         # stations do not come sorted by cell
    lon, lat = lon[perm], lat[perm]
    lone, rowless = int(np.flatnonzero(perm == lone)[0]), int(np.flatnonzero(perm == rowless)[0])
    v = 2.4 + 0.03 * (lon[None, :] + 116.5) - 0.02 * (lat[None, :] - 34.0) + 0.05 * rng.standard_normal((ND, n))
    v[rng.uniform(size=(ND, n)) < 0.3] = np.nan
    v[:, rowless] = np.nan
    keep = v[4, lone] if not np.isnan(v[4, lone]) else 2.41
    v[:, lone] = np.nan
    v[4, lone] = keep
    for i in range(n):                                                                # every other station keeps at least two rows
        if i not in (lone, rowless) and (~np.isnan(v[:, i])).sum() < 2:
            v[:2, i] = 2.4 + 0.01 * np.arange(2)
    ids = np.array([f'S{i:03d}' for i in range(n)])
    dates = np.datetime64('2020-01-01') + 12 * np.arange(ND)
    return ids, lon, lat, dates, v, lone, rowless


class _ContainmentTree:
    """What RaiderStats asks of an STRtree: query(point) -> the indices of the rectangles that hold it."""

    def __init__(self, polys):
        self.rect = []
        for p in polys:
            xy = np.asarray(p.bounds[0], dtype=np.float64)
            self.rect.append((xy[:, 0].min(), xy[:, 0].max(), xy[:, 1].min(), xy[:, 1].max()))

    def query(self, point):
        x, y = point.coords[0]
        return [k for k, (x0, x1, y0, y1) in enumerate(self.rect) if x0 <= x <= x1 and y0 <= y <= y1]


def reference_module():
    import matplotlib
    matplotlib.use('Agg')
    from oracle.refharness import ref_import
    ref_import.import_reference()
    m = types.ModuleType('shapely.strtree')
    m.STRtree = _ContainmentTree
    sys.modules['shapely.strtree'] = m
    import RAiDER.cli.statsPlot as sp
    return sp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'tests' / 'golden' / 'g22_grid_stats.npz'))
    a = ap.parse_args()
    ids, lon, lat, dates, v, lone, rowless = scene()
    n = lon.size
    import pandas as pd
    sp = reference_module()
    tmp = Path(tempfile.mkdtemp(prefix='g22_'))
    csv = tmp / 'stations.csv'
    with open(csv, 'w') as f:
        f.write('ID,Lat,Lon,Date,ZTD\n')
        for d in range(ND):
            for i in range(n):
                if not np.isnan(v[d, i]):
                    f.write(f'{ids[i]},{float(lat[i])!r},{float(lon[i])!r},{dates[d]},{float(v[d, i])!r}\n')
    out = dict(ids=ids, dates=dates.astype('datetime64[D]').astype(np.int64))
    parsed = None
    for tag, s in (('s1', 1), ('s05', 0.5)):
        o = sp.RaiderStats(str(csv), 'ZTD', workdir=str(tmp / tag), spacing=s, grid_heatmap=True, grid_delay_mean=True, grid_delay_median=True,
                           grid_delay_stdev=True, grid_delay_absolute_mean=True, grid_delay_absolute_median=True, grid_delay_absolute_stdev=True)
        # the series as the reference parsed it
        vv = np.full((ND, n), np.nan); plo = lon.copy(); pla = lat.copy()
        day = o.df['Date'].values.astype('datetime64[D]')
        for sid, lo_, la_, dd, z in zip(o.df['ID'].values, o.df['Lon'].values, o.df['Lat'].values, day, o.df['ZTD'].values):
            i = int(sid[1:]); d = int(np.flatnonzero(dates == dd)[0])
            assert np.isnan(vv[d, i])
            vv[d, i] = z; plo[i] = lo_; pla[i] = la_
        assert np.array_equal(np.isnan(vv), np.isnan(v)), 'the reference dropped or invented rows'
        moved = int((vv != v)[~np.isnan(v)].sum())
        if parsed is None:
            parsed = (vv, plo, pla)
            print(f'pandas parsed {moved} of {int((~np.isnan(v)).sum())} values to another double than was written')
        else:
            assert np.array_equal(parsed[0], vv, equal_nan=True) and np.array_equal(parsed[1], plo) and np.array_equal(parsed[2], pla)
        out[f'{tag}_plotbbox'] = np.array(o.plotbbox, dtype=np.float64); out[f'{tag}_grid_dim'] = np.array(o.grid_dim, dtype=np.int64)
        out[f'{tag}_spacing'] = np.float64(o.spacing)
        for name in MAPS:
            m = np.array(getattr(o, name), dtype=np.float64)
            assert m.shape == (o.grid_dim[1], o.grid_dim[0]), (name, m.shape)
            out[f'{tag}_{name}'] = m
        if tag == 's1':
            heat = out['s1_grid_heatmap']
            assert sorted(np.nan_to_num(heat).astype(int).ravel().tolist()) == sorted(CELLS.values()), heat
            assert np.isnan(out['s1_grid_delay_stdev'][1, 0]) and not np.isnan(out['s1_grid_delay_mean'][1, 0]), 'the lone single-row station'
            node = (np.floor(plo - W) * 2 + (1 - np.floor(pla - S))).astype(int)
            rows = np.array([(~np.isnan(vv[:, node == g])).sum() for g in range(6)])
            assert (rows[rows > 0] % 2 == 0).any() and (rows % 2 == 1).any(), rows
            print('rows per cell', rows.tolist())
    out['values'], out['lon'], out['lat'] = parsed
    out['lone_station'] = np.int64(lone); out['rowless_station'] = np.int64(rowless)
    from oracle.refharness import ref_import
    out['_meta'] = np.array(json.dumps(dict(
        ref_import.provenance(), numpy=np.__version__, pandas=pd.__version__,
        route="RaiderStats(csv, 'ZTD', spacing=..., all seven grid_* = True): the constructor runs create_DF whole",
        strtree='shapely.strtree.STRtree replaced by a generator-owned containment query (stations off every cell edge)',
        values='rebuilt from the reference DataFrame: as pandas parsed the CSV',
        generator='tools/gen_golden_grid_stats.py, companion of oracle/refharness/gen_golden.py')))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(a.out, **out)
    print(a.out, Path(a.out).stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
