"""Per-grid-cell variograms of a clustered station network: raider_amd.grid_variograms (one device pass per stage) against the route
the package offered before - a Python loop over the cells of raider_amd.station_variograms(..., fit=False), which transforms, deramps
(np.linalg.lstsq per date on the host) and launches per cell.  Both on host arrays, both without fits, on the same machine.

Scene (fixed; not tuned): 20 000 stations over 40 x 25 degrees of 1-degree cells (lon -120 .. -80, lat 25 .. 50): 70 % in 60 Gaussian
clusters of 0.2 .. 1.5 degrees, 30 % uniform; D dates, one value in 97 missing; 19 bins, plane removed, density threshold 10.  The
cell-size histogram is reported.  Before timing, the two routes' counts are asserted equal for every cell of two stations or more.

Three ALTERNATED repeats (new, loop, new, loop, ...) after one warm-up of each; median and span (max - min) per route.  The record says
whether the new route is ahead by more than the two spans together.  The total fits (host scipy, one per cell with a good date) are
timed separately, once.  One invocation measures one D and appends its row to --out: give each its own time limit.

    python tools/bench_grid_variogram.py --dates 64 [--stations 20000] [--reps 3] [--out profiles/r26_grid_variogram.json]
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def make_scene(n, nd, seed=26):
    rng = np.random.default_rng(seed)
    k = int(0.7 * n)
    centres = np.column_stack([rng.uniform(-119.0, -81.0, 60), rng.uniform(26.0, 49.0, 60)])
    width = rng.uniform(0.2, 1.5, 60)
    which = rng.integers(0, 60, k)
    lon = np.concatenate([centres[which, 0] + width[which] * rng.standard_normal(k), rng.uniform(-120.0, -80.0, n - k)])
    lat = np.concatenate([centres[which, 1] + width[which] * rng.standard_normal(k), rng.uniform(25.0, 50.0, n - k)])
    lon = np.clip(lon, -119.999, -80.001); lat = np.clip(lat, 25.001, 49.999)
    perm = rng.permutation(n)
    lon, lat = lon[perm], lat[perm]
    v = 2.4 + 0.01 * (lon[None, :] + 100.0) + 0.05 * rng.standard_normal((nd, n))
    v[rng.random((nd, n)) < 1.0 / 97.0] = np.nan
    return lon, lat, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--dates', type=int, default=64)
    ap.add_argument('--stations', type=int, default=20000)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default='profiles/r26_grid_variogram.json')
    a = ap.parse_args()
    import raider_amd as R
    from raider_amd import _lib as L
    from raider_amd import variogram as V
    ctx = R.Context.default()
    name, cus, _ = ctx.device_info()
    lon, lat, v = make_scene(a.stations, a.dates)
    grid = V.station_grid(lon, lat)
    sizes = np.diff(grid.start)
    cells = [c for c in range(sizes.size) if sizes[c] >= 2]
    index = {c: grid.order[grid.start[c]:grid.start[c + 1]] for c in cells}

    def new_route():
        return V.grid_variograms(lon, lat, v, fit=False, ctx=ctx)

    def loop_route():
        return {c: V.station_variograms(lon[i], lat[i], v[:, i], fit=False, ctx=ctx).variogram for c, i in index.items()}

    gv = new_route(); per = loop_route()                   # the warm-up of both, and the check
    for c in cells:
        assert np.array_equal(gv.count[c], per[c].count), f'cell {c}: the two routes count differently'
    pair_dates = int(sum(int(per[c].count.sum()) for c in cells))
    t_new, t_loop = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter(); new_route(); t_new.append(time.perf_counter() - t0)
        t0 = time.perf_counter(); loop_route(); t_loop.append(time.perf_counter() - t0)
    good = np.flatnonzero((gv.status != 1).any(axis=1))
    t0 = time.perf_counter()
    nfit = 0
    for c in good:
        h, g = gv.total_binned(c)
        if h.size:
            V.fit_variogram(h, g); nfit += 1
    t_fit = time.perf_counter() - t0
    med_new, med_loop = statistics.median(t_new), statistics.median(t_loop)
    span_new, span_loop = max(t_new) - min(t_new), max(t_loop) - min(t_loop)
    bounds = [0, 1, 2, 10, 20, 50, 100, 200, 512, 1 << 30]
    hist = {f'{lo}..{hi - 1}' if hi < (1 << 30) else f'{lo}+': int(((sizes >= lo) & (sizes < hi)).sum()) for lo, hi in zip(bounds[:-1], bounds[1:])}
    row = dict(stations=a.stations, dates=a.dates, bins=19, cells=int(sizes.size), cells_with_stations=int((sizes > 0).sum()),
               cells_with_a_good_date=int(good.size), largest_cell=int(sizes.max()), cell_size_histogram=hist,
               slices_done_on_host_status_2=int((gv.status == 2).sum()), binned_pair_dates=pair_dates,
               grid_variograms_s=dict(median=med_new, span=span_new, repeats=t_new),
               loop_of_station_variograms_s=dict(median=med_loop, span=span_loop, repeats=t_loop),
               ratio_loop_over_new=med_loop / med_new, ahead_by_more_than_both_spans=bool(med_loop - med_new > span_new + span_loop),
               counts_equal=True, total_fits=dict(fits=nfit, seconds=t_fit))
    print(f"# D={a.dates}: grid_variograms {med_new:.3f} s (span {span_new:.3f}), loop {med_loop:.3f} s (span {span_loop:.3f}), "
          f"{nfit} total fits {t_fit:.2f} s", file=sys.stderr, flush=True)
    out = Path(a.out)
    res = json.loads(out.read_text()) if out.exists() else dict(tool='bench_grid_variogram', rows=[])
    if res.get('source_hash') != L.source_hash():
        res = dict(tool='bench_grid_variogram', rows=[])
    res.update(device=name, compute_units=cus, source_hash=L.source_hash())
    res['rows'] = [r for r in res['rows'] if (r['stations'], r['dates']) != (a.stations, a.dates)] + [row]
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + '\n')
    print(json.dumps(row))


if __name__ == '__main__':
    main()
