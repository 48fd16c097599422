"""Delay cubes on a UTM output grid: the per-height host loop the package ran before (transformPoints + Cube.interp per height for
zenith cubes; transformPoints + lla2ecef + getLookVectors + Rays.points + Cube.raytrace per slice for ray-traced ones), rebuilt from
the public per-height calls, against the device routes (rdr_build_cube_grid; rdr_grid_geodetic + one LLH slice batch).  Workloads:
a zenith and a ray-traced cube on a --grid x --grid UTM 11N grid x 20 heights over a 300 x 300 x 80 weather cube; --stations
stations with out_proj = UTM (Zenith and Raytracing: the point branch's intermediate cube on a --pgrid^2 grid and the gather, without
tropo_delay's file prelude); a --dates-date ray-traced series (tropo_delay_series against per-date loops).  Wall times
(median of --reps, the old route once), max |new - old|.  Prints ONE JSON line.

    python tools/bench_projected_grid.py [--grid 1000] [--stations 1000000] [--pgrid 200] [--dates 4] [--reps 3] [--out profiles/<name>.json]
"""
import argparse
import datetime as dt
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

UTM = 32611


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--grid', type=int, default=1000)
    ap.add_argument('--stations', type=int, default=1_000_000)
    ap.add_argument('--pgrid', type=int, default=200)
    ap.add_argument('--dates', type=int, default=4)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import raider_amd as R
    from raider_amd.delay import GridAOI, _build_cube, _build_cube_ray, grid_projection, transformPoints, tropo_delay_series
    from raider_amd.delayFcns import FieldInterpolator
    from raider_amd.losreader import Raytracing
    from raider_amd.synthetic import synthetic_cube
    from raider_amd.utilFcns import lla2ecef

    def timed(fn, reps):
        ts, out = [], None
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), out

    def maxdiff(x, y):
        x, y = np.asarray(x), np.asarray(y)
        same_nan = bool(np.array_equal(np.isnan(x), np.isnan(y)))
        ok = ~np.isnan(x)
        return (float(np.abs(x[ok] - y[ok]).max()) if ok.any() else 0.0), same_nan

    # weather cube over the US south-west, UTM 11N output grid inside it
    c = synthetic_cube(300, 300, 80, seed=0)
    zref = float(c['zs'].max() - 1)
    wm = dict(x=c['xs'], y=c['ys'], z=c['zs'], wet=c['wet'], hydro=c['hydro'], wet_total=c['wet_total'], hydro_total=c['hydro_total'])
    cube = R.Cube(c['ys'], c['xs'], c['zs'], c['wet'], c['hydro'], order='zyx')
    tot = R.Cube(c['ys'], c['xs'], c['zs'], c['wet_total'], c['hydro_total'], order='zyx')
    step = 600000.0 / a.grid
    xg = 200000.0 + step * np.arange(a.grid); yg = 3950000.0 - step * np.arange(a.grid)
    zpts = np.linspace(0.0, 5000.0, 20)
    los = Raytracing(inc=38.0, heading=-167.9)
    ip = [FieldInterpolator(cube, 0), FieldInterpolator(cube, 1)]
    it = [FieldInterpolator(tot, 0), FieldInterpolator(tot, 1)]

    def old_zenith(cb, xg, yg, zpts):
        xx, yy = np.meshgrid(xg, yg)
        out = [np.empty((zpts.size, yg.size, xg.size)) for _ in range(2)]
        for k, ht in enumerate(zpts):
            w, h = cb.interp(transformPoints(yy, xx, np.full(yy.shape, ht), UTM, 4326))
            out[0][k] = w; out[1][k] = h
        return out

    def old_ray(cb, xg, yg, zpts):
        xx, yy = np.meshgrid(xg, yg)
        out = [np.empty((zpts.size, yg.size, xg.size)) for _ in range(2)]
        for k, ht in enumerate(zpts):
            p = transformPoints(yy, xx, np.full(yy.shape, ht), UTM, 4326)
            llh = [p[..., 1], p[..., 0], p[..., 2]]
            xyz = np.stack(lla2ecef(llh[1], llh[0], llh[2]), axis=-1)
            lv = los.getLookVectors(ht, llh, xyz, yy)
            w, h, _, _ = cb.raytrace(R.Rays.points(lat=llh[1], lon=llh[0], los=lv), float(ht), zref)
            out[0][k] = np.asarray(w).reshape(yy.shape); out[1][k] = np.asarray(h).reshape(yy.shape)
        return out

    res = dict(tool='bench_projected_grid', grid=[a.grid, a.grid, int(zpts.size)], cube=[300, 300, 80], crs=f'EPSG:{UTM}', workloads={})
    timed(lambda: _build_cube(xg[:64], yg[:64], zpts, 4326, UTM, it), 1)                        # (warm-up: library, pools)
    timed(lambda: _build_cube_ray(xg[:64], yg[:64], zpts, los, 4326, UTM, ip, MAX_TROPO_HEIGHT=zref), 1)

    # 1. zenith cube
    t_old, o = timed(lambda: old_zenith(tot, xg, yg, zpts), 1)
    t_new, n = timed(lambda: _build_cube(xg, yg, zpts, 4326, UTM, it), a.reps)
    d, m = maxdiff(n[0], o[0])
    res['workloads']['zenith_cube'] = dict(old_ms=t_old, new_ms=t_new, speedup=t_old / t_new, max_abs_diff_m=d, same_nan=m)
    del o, n
    # 2. ray-traced cube
    t_old, o = timed(lambda: old_ray(cube, xg, yg, zpts), 1)
    t_new, n = timed(lambda: _build_cube_ray(xg, yg, zpts, los, 4326, UTM, ip, MAX_TROPO_HEIGHT=zref), a.reps)
    d, m = maxdiff(n[0], o[0])
    res['workloads']['ray_cube'] = dict(old_ms=t_old, new_ms=t_new, speedup=t_old / t_new, max_abs_diff_m=d, same_nan=m)
    del o, n
    # 3. stations with out_proj = UTM: the old route built the intermediate cube with the loops above, wrapped it and gathered
    rng = np.random.default_rng(0)
    ns = a.stations
    la = rng.uniform(31.0, 35.0, ns); lo = rng.uniform(-119.5, -114.5, ns); hg = rng.uniform(0.0, 3000.0, ns)
    yx = transformPoints(la, lo, 0 * la, 4326, UTM)
    px = np.linspace(yx[:, 1].min() - 2000.0, yx[:, 1].max() + 2000.0, a.pgrid); py = np.linspace(yx[:, 0].max() + 2000.0, yx[:, 0].min() - 2000.0, a.pgrid)
    hl = list(zpts)   # (the series' height levels)
    grid = grid_projection(UTM)

    def new_zenith():                        # what _point_branch_on_device runs: one rdr_point_delays_grid call
        return tot.point_delays(px, py, zpts, transformPoints(la, lo, hg, 4326, UTM), grid=grid)[:2]

    def new_ray():                           # one LLH slice batch into a device cube, then the gather
        dc = cube.raytrace_slices_to_cube(los.ray_batch_slices(px, py, zpts, crs=UTM), zpts, zref)[0]
        return dc.interp_project(transformPoints(la, lo, hg, 4326, UTM))
    for name, build, cb, new in (('stations_zenith', old_zenith, tot, new_zenith), ('stations_raytracing', old_ray, cube, new_ray)):
        def old():
            w, h = build(cb, px, py, zpts)
            ic = R.Cube(py, px, zpts, w, h, order='zyx')
            return ic.interp_project(transformPoints(la, lo, hg, 4326, UTM))
        t_old, o = timed(old, 1)
        t_new, n = timed(new, a.reps)
        d, m = maxdiff(n[0], o[0])
        res['workloads'][name] = dict(stations=ns, grid=[a.pgrid, a.pgrid, int(zpts.size)], old_ms=t_old, new_ms=t_new, speedup=t_old / t_new,
                                      max_abs_diff_m=d, same_nan=m)
        del o, n
    # 4. a ray-traced series on the UTM grid
    files = [dict(wm, wet=c['wet'] * (1.0 + 0.02 * e), hydro=c['hydro'] * (1.0 + 0.02 * e)) for e in range(a.dates)]
    dates = [dt.datetime(2020, 1, 1) + dt.timedelta(days=12 * e) for e in range(a.dates)]

    def old_series():
        out = []
        for f in files:
            cb = R.Cube(f['y'], f['x'], f['z'], f['wet'], f['hydro'], order='zyx')
            out.append(old_ray(cb, xg, yg, zpts))
        return out
    t_old, o = timed(old_series, 1)
    ser = {}
    t_new, n = timed(lambda: ser.setdefault('s', tropo_delay_series(dates, files, GridAOI(xg, yg), los, hl, UTM)), 1)
    n = ser['s']
    d, m = maxdiff(np.asarray(n[-1][0]['wet']), o[-1][0])
    res['workloads']['ray_series'] = dict(dates=a.dates, old_ms=t_old, new_ms=t_new, speedup=t_old / t_new, routes=list(n.routes),
                                          max_abs_diff_m=d, same_nan=m)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
