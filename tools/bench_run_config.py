#!/usr/bin/env python3
"""Time a run-configuration file of D dates through raider_amd.cli.calcDelays - one call of tropo_delay_interp_series for all dates -
against the same D configurations run one date at a time (D calls of calcDelays, what a per-date loop does), file I/O on both sides
inside the timed region: reading the YAML, finding and opening D processed weather-model files, uploading them, tracing, writing D
delay cubes.

Workload: 8 dates, a 300 x 300 x 80 synthetic processed model per date (173 MB each, raider_amd.synthetic written with
ProcessedModel.to_netcdf under the names the driver looks for), a bounding box whose output grid is about 316 x 316 nodes (10^5
rays) x 20 heights, ray-traced.  The line of sight is Raytracing(inc=, heading=) put in place of the parsed one: an orbit file
covers one acquisition, and a run of its own for each of eight dates would need eight of them.

Before anything is timed the two sides' outputs are compared (the same bytes).  Then one warm-up of each side and three repeats,
the sides alternating; the cache of opened model files and device cubes (delayFcns.clear_file_cache) is emptied before every run, so
each run reads its files again (from the page cache, both sides alike).  Median and span per side, and where the time of one
all-dates run goes (preparation, the series call, writing).

    python tools/bench_run_config.py [--out profiles/r20_run_config.json] [--dates 8] [--repeats 3]
"""
import argparse
import datetime as dt
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'r20_run_config.json'))
    ap.add_argument('--dates', type=int, default=8)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--grid', default='300,300,80', help='ny,nx,nz of the synthetic model')
    ap.add_argument('--spacing', type=float, default=870.0, help='cube_spacing_in_m of the output grid')
    args = ap.parse_args()
    import yaml
    from raider_amd import Context, Cube, cli, h5lite, _lib as L
    from raider_amd.delayFcns import clear_file_cache
    from raider_amd.losreader import Raytracing
    from raider_amd.synthetic import synthetic_cube
    from raider_amd.weather import ProcessedModel

    class FixedRaytracing(Raytracing):
        def getSensorDirection(self):
            return 'asc'
    parse = cli.read_run_config_file

    def parse_and_inject(path):
        rc = parse(path)
        rc.los_group.los = FixedRaytracing(inc=34.0, heading=-12.0)
        return rc
    cli.read_run_config_file = parse_and_inject

    ny, nx, nz = (int(v) for v in args.grid.split(','))
    days = [dt.date(2020, 1, 1) + dt.timedelta(days=k) for k in range(args.dates)]
    tmp = Path(tempfile.mkdtemp(prefix='bench_run_config_'))
    heights = ' '.join(str(250 * k) for k in range(20))

    def config(dates, out):
        return dict(weather_model='ERA5', look_dir='right', date_group=dict(date_list=[int(d.strftime('%Y%m%d')) for d in dates]),
                    time_group=dict(time='13:00:00', interpolate_time='none'), aoi_group=dict(bounding_box='32 34 -118 -116'),
                    height_group=dict(height_levels=heights), los_group={},
                    runtime_group=dict(output_directory=str(tmp / out), weather_model_directory=str(tmp / 'wm'), cube_spacing_in_m=args.spacing, verbose=False))

    def write_yaml(name, cfg):
        (tmp / name).write_text(yaml.safe_dump(cfg))
        return str(tmp / name)
    all_dates = write_yaml('all.yaml', config(days, 'out_all'))
    singles = [write_yaml(f'one_{k}.yaml', config([d], 'out_one')) for k, d in enumerate(days)]

    # the models, under the names the driver looks for (its own sequence up to set_latlon_bounds)
    rc = cli.checkArgs(cli.read_run_config_file(Path(all_dates)))
    aoi, los, model = rc.aoi_group.aoi, rc.los_group.los, rc.weather_model
    aoi.add_buffer(model.getLLRes())
    aoi.set_output_xygrid(rc.runtime_group.output_projection)
    model.set_latlon_bounds(aoi.calc_buffer_ray(los.getSensorDirection(), lookDir=los.getLookDirection(), incAngle=30), output_spacing=aoi.get_output_spacing())
    S, N, W, E = (float(v) for v in model.get_latlon_bounds())
    t0 = time.perf_counter()
    for k, t in enumerate(rc.date_group.date_list):
        c = synthetic_cube(ny, nx, nz, seed=k, y0=S, y1=N, x0=W, x1=E)
        pm = ProcessedModel(Cube(c['ys'], c['xs'], c['zs'], c['wet'], c['hydro'], order='zyx'),
                            Cube(c['ys'], c['xs'], c['zs'], c['wet_total'], c['hydro_total'], order='zyx'), c['zs'])
        model.setTime(t)
        pm.to_netcdf(model.out_file(model.get_wmLoc()), time=t, model_name=model.Model())
        del pm, c
    model_bytes = sum(p.stat().st_size for p in (tmp / 'wm').iterdir())
    print(f'wrote {args.dates} models, {model_bytes / 1e6:.0f} MB, in {time.perf_counter() - t0:.1f} s; output grid {aoi.ypts.size} x {aoi.xpts.size} x 20', flush=True)
    ctx = Context.default()

    def together():
        clear_file_cache()
        paths = cli.calcDelays([all_dates])
        ctx.synchronize()
        return paths, list(cli.last_run['routes'])

    def one_by_one():
        clear_file_cache()
        paths, routes = [], []
        for y in singles:
            paths += cli.calcDelays([y])
            routes += cli.last_run['routes']
        ctx.synchronize()
        return paths, routes

    # the two sides write the same bytes
    (pa, ra), (pb, rb) = together(), one_by_one()
    assert len(pa) == len(pb) == args.dates and [p.name for p in pa] == [p.name for p in pb]
    for a, b in zip(pa, pb):
        fa, fb = h5lite.File(a), h5lite.File(b)
        for v in ('wet', 'hydro'):
            da = fa[v].read()
            assert np.isfinite(da).all() and da.tobytes() == fb[v].read().tobytes(), (a.name, v)
    out_bytes = sum(p.stat().st_size for p in pa)

    # where one all-dates run spends its time: the three phases of the driver, by wrapping its own calls
    phases = dict(prepare=0.0, series=0.0, write=0.0)

    def timed(fn, key):
        def wrapper(*a, **k):
            t = time.perf_counter()
            try:
                return fn(*a, **k)
            finally:
                ctx.synchronize()
                phases[key] += time.perf_counter() - t
        return wrapper
    saved = cli.prepareWeatherModel, cli.tropo_delay_interp_series, cli._write_date
    cli.prepareWeatherModel, cli.tropo_delay_interp_series, cli._write_date = timed(saved[0], 'prepare'), timed(saved[1], 'series'), timed(saved[2], 'write')
    t = time.perf_counter()
    together()
    phases['total'] = time.perf_counter() - t
    phases['other'] = phases['total'] - phases['prepare'] - phases['series'] - phases['write']
    cli.prepareWeatherModel, cli.tropo_delay_interp_series, cli._write_date = saved

    times = dict(together=[], one_by_one=[])
    for _ in range(args.repeats):
        for name, fn in (('together', together), ('one_by_one', one_by_one)):
            t = time.perf_counter()
            fn()
            times[name].append(time.perf_counter() - t)
    result = dict(device=ctx.device_info()[0], source_hash=L.source_hash(), dates=args.dates, model_grid=[nz, ny, nx], model_bytes=model_bytes,
                  output_grid=[20, int(aoi.ypts.size), int(aoi.xpts.size)], rays_per_date=int(aoi.ypts.size * aoi.xpts.size) * 20, output_bytes=out_bytes,
                  routes=dict(together=ra, one_by_one=rb), outputs_identical=True, phases_of_one_all_dates_run_seconds=phases)
    for name in times:
        result[name] = dict(seconds=times[name], median=statistics.median(times[name]), span=[min(times[name]), max(times[name])],
                            per_date_median=statistics.median(times[name]) / args.dates)
    result['together_faster_in_every_repeat'] = bool(all(a < b for a, b in zip(times['together'], times['one_by_one'])))
    result['speedup_median'] = result['one_by_one']['median'] / result['together']['median']
    print(json.dumps(result), flush=True)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + '\n')
    print('wrote', args.out)
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)


if __name__ == '__main__':
    main()
