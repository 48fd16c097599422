"""Gridded station statistics of a clustered station network: raider_amd.grid_statistics (one device call) on host arrays and on device
tensors, with and without the medians, against the CPU route - pandas' groupby chain as `raiderStats` runs it (per map: the statistic
per station and cell, then the mean per cell; or the statistic per cell) when pandas is importable, else a NumPy restatement per cell.
The record says which one ran.  All on the same machine, the CPU route on whatever threads pandas / NumPy take of it.

Scene: that of tools/bench_grid_variogram.py (20 000 stations, 70 % in 60 clusters, over 40 x 25 one-degree cells; one value in 97
missing), D dates.  The CPU route starts from the long table it needs (built outside the timing, as the reference has it after reading
its CSV); the device routes start from the [D, N] series.  Before timing, the CPU maps are compared with the device's.

Three ALTERNATED repeats (every route once per round) after one warm-up of each; median and span (max - min) per route.  One invocation
measures one D and appends its row to --out: give each its own time limit.  The row also holds the time of the library call alone on
the sorted series on the device, per output group, with and without its median: where the device time goes.

    python tools/bench_grid_stats.py --dates 365 [--stations 20000] [--reps 3] [--out profiles/r27_grid_stats.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tools.bench_grid_variogram import make_scene          # noqa: E402

MAPS = ('grid_delay_mean', 'grid_delay_median', 'grid_delay_stdev', 'grid_delay_absolute_mean', 'grid_delay_absolute_median', 'grid_delay_absolute_stdev')


def pandas_route(df, ng):
    """the seven cell arrays [ng] by groupby, a statistic per (station, cell) and its mean per cell, or the statistic per cell"""
    out = {'grid_heatmap': df.groupby('gridnode')['ID'].nunique().reindex(range(ng)).to_numpy(dtype=np.float64)}
    per_station = df.groupby(['ID', 'gridnode'], as_index=False)['v']
    per_cell = df.groupby('gridnode')['v']
    for stat in ('mean', 'median', 'std'):
        name = 'stdev' if stat == 'std' else stat
        a = getattr(per_station, stat)().groupby('gridnode')['v'].mean()
        out[f'grid_delay_{name}'] = a.reindex(range(ng)).to_numpy(dtype=np.float64)
        out[f'grid_delay_absolute_{name}'] = getattr(per_cell, stat)().reindex(range(ng)).to_numpy(dtype=np.float64)
    return out


def numpy_route(vs, start):
    ng = start.size - 1
    out = {k: np.full(ng, np.nan) for k in ('grid_heatmap',) + MAPS}
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        for c in range(ng):
            s = vs[:, start[c]:start[c + 1]]
            if s.shape[1] == 0 or np.isnan(s).all():
                continue
            cnt = (~np.isnan(s)).sum(axis=0)
            out['grid_heatmap'][c] = (cnt > 0).sum()
            out['grid_delay_mean'][c] = np.nanmean(np.nanmean(s, axis=0)); out['grid_delay_median'][c] = np.nanmean(np.nanmedian(s, axis=0))
            sd = np.where(cnt > 1, np.nanstd(s, axis=0, ddof=1), np.nan)
            out['grid_delay_stdev'][c] = np.nanmean(sd) if (cnt > 1).any() else np.nan
            out['grid_delay_absolute_mean'][c] = np.nanmean(s); out['grid_delay_absolute_median'][c] = np.nanmedian(s)
            out['grid_delay_absolute_stdev'][c] = np.nanstd(s, ddof=1) if cnt.sum() > 1 else np.nan
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dates', type=int, default=365)
    ap.add_argument('--stations', type=int, default=20000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default='profiles/r27_grid_stats.json')
    a = ap.parse_args()
    import torch
    import raider_amd as R
    from raider_amd import _lib as L
    from raider_amd import variogram as V
    ctx = R.Context.default()
    name, cus, _ = ctx.device_info()
    lon, lat, v = make_scene(a.stations, a.dates)
    grid = V.station_grid(lon, lat)
    ng = grid.gridpoints.shape[0]
    sizes = np.diff(grid.start)
    lon_d, lat_d, v_d = torch.from_numpy(lon).cuda(), torch.from_numpy(lat).cuda(), torch.from_numpy(v).cuda()
    try:
        import pandas as pd
        d, i = np.nonzero(~np.isnan(v))
        df = pd.DataFrame({'ID': i.astype(np.int32), 'gridnode': grid.cell[i].astype(np.int32), 'v': v[d, i]})
        del d, i
        cpu_name = f'pandas {pd.__version__} groupby chain on the long table of {len(df)} rows'
        cpu = lambda: pandas_route(df, ng)
    except ImportError:
        vs = np.ascontiguousarray(v[:, grid.order])
        cpu_name = 'NumPy restatement per cell (nanmean / nanmedian / nanstd); pandas is not importable'
        cpu = lambda: numpy_route(vs, grid.start)

    def dev(medians):
        r = R.grid_statistics(lon_d, lat_d, v_d, medians=medians, ctx=ctx)
        torch.cuda.synchronize()
        return r
    routes = {'host_arrays': lambda: R.grid_statistics(lon, lat, v, ctx=ctx), 'host_arrays_no_medians': lambda: R.grid_statistics(lon, lat, v, medians=False, ctx=ctx),
              'device_tensors': lambda: dev(True), 'device_tensors_no_medians': lambda: dev(False), 'cpu': cpu}
    first = {k: f() for k, f in routes.items()}            # the warm-up of each, and the check
    res, ref = first['host_arrays'], first['cpu']
    gmap = lambda x: np.asarray(x).reshape(grid.grid_dim).T
    worst = {}
    for k in ('grid_heatmap',) + MAPS:
        got, want = getattr(res, k), gmap(ref[k])
        assert np.array_equal(np.isnan(got), np.isnan(want)), f'{k}: the routes disagree on the empty cells'
        ok = ~np.isnan(want)
        worst[k] = float((np.abs(got[ok] - want[ok]) / np.maximum(np.abs(want[ok]), 1e-300)).max())
        assert worst[k] <= 1e-9, f'{k}: the routes differ by a relative {worst[k]}'
    times = {k: [] for k in routes}
    for _ in range(a.reps):
        for k, f in routes.items():
            t0 = time.perf_counter(); f(); times[k].append(time.perf_counter() - t0)
    summary = {k: dict(median=statistics.median(t), span=max(t) - min(t), repeats=t) for k, t in times.items()}
    c = summary['cpu']
    for k in routes:
        if k != 'cpu':
            s = summary[k]
            s['ratio_cpu_over_this'] = c['median'] / s['median']
            s['ahead_of_cpu_by_more_than_both_spans'] = bool(c['median'] - s['median'] > c['span'] + s['span'])
    for k in ('host_arrays', 'device_tensors'):
        s, t = summary[k], summary[k + '_no_medians']
        s['medians_cost_s'] = s['median'] - t['median']
        s['medians_cost_above_both_spans'] = bool(s['median'] - t['median'] > s['span'] + t['span'])
    # where the device time goes: the library call alone on the sorted series on the device, one output group at a time
    od = torch.from_numpy(np.ascontiguousarray(grid.order)).cuda()
    vs_d = v_d.index_select(1, od).contiguous(); cs_d = torch.from_numpy(np.ascontiguousarray(grid.start)).cuda()
    n_in = int(grid.order.size)
    buf = {k: torch.empty(n_in if k < 4 else ng, dtype=torch.int64 if k % 4 == 0 else torch.float64, device='cuda') for k in range(12)}

    def group(first, medians):
        p = [L.ptr(buf[k]) if first <= k < first + 4 and (medians or k % 4 != 2) else None for k in range(12)]
        L.check(ctx.lib.rdr_grid_stats(ctx.handle, L.ptr(vs_d), n_in, a.dates, L.ptr(cs_d), ng, *p, L.RDR_DEVICE), ctx.handle)
        torch.cuda.synchronize()
    calls = {'station_group': lambda: group(0, True), 'station_group_no_median': lambda: group(0, False),
             'absolute_group': lambda: group(8, True), 'absolute_group_no_median': lambda: group(8, False)}
    ctimes = {k: [] for k in calls}
    for r in range(a.reps + 1):
        for k, f in calls.items():
            t0 = time.perf_counter(); f(); dt = time.perf_counter() - t0
            if r:
                ctimes[k].append(dt)
    library_calls = {k: dict(median=statistics.median(t), span=max(t) - min(t), repeats=t) for k, t in ctimes.items()}
    gb = a.dates * n_in * 8 / 1e9
    for k, passes in (('station_group', 11), ('station_group_no_median', 2), ('absolute_group', 11), ('absolute_group_no_median', 2)):
        library_calls[k]['passes_over_the_series'] = passes
        library_calls[k]['series_GB_read_per_s_if_every_pass_came_from_memory'] = passes * gb / library_calls[k]['median']
    row = dict(stations=a.stations, dates=a.dates, values=int((~np.isnan(v)).sum()), cells=int(ng), cells_with_stations=int((sizes > 0).sum()),
               largest_cell=int(sizes.max()), cpu_route=cpu_name, largest_relative_difference_to_cpu=worst, seconds=summary,
               library_call_alone_s=library_calls)
    print('# D=%d: ' % a.dates + ', '.join(f"{k} {s['median']:.4f} s (span {s['span']:.4f})" for k, s in summary.items()), file=sys.stderr, flush=True)
    print('#   library call alone: ' + ', '.join(f"{k} {s['median'] * 1e3:.3f} ms" for k, s in library_calls.items()), file=sys.stderr, flush=True)
    out = Path(a.out)
    rec = json.loads(out.read_text()) if out.exists() else dict(tool='bench_grid_stats', rows=[])
    if rec.get('source_hash') != L.source_hash():
        rec = dict(tool='bench_grid_stats', rows=[])
    rec.update(device=name, compute_units=cus, source_hash=L.source_hash())
    rec['rows'] = [r for r in rec['rows'] if (r['stations'], r['dates']) != (a.stations, a.dates)] + [row]
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(rec, indent=1) + '\n')
    print(json.dumps(row))


if __name__ == '__main__':
    main()
