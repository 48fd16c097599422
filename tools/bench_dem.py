#!/usr/bin/env python3
"""Time the two raster kernels behind raider_amd.llreader on a scene of the size a user brings: a 4000 x 4000 lat / lon raster pair
(f64, as ISCE writes lat.rdr / lon.rdr) and a 3600 x 3600 int16 DEM (one SRTM-style tile).

  bounds    rdr_raster_bounds over both rasters (device tensors; host arrays, upload included) against np.nanmin / np.nanmax of the
            masked arrays - what bounds_from_latlon_rasters needs;
  sampling  rdr_raster_sample, nearest and linear, at the 16 M pixels (device tensors; host arrays, transfers included) against the
            NumPy restatement of the nearest rule the tests use.

Before anything is timed the device results are compared with NumPy's (bounds: equal; nearest: the same bits).  Then a warm-up and
`--repeats` alternated repeats, the host clock around calls that end in a synchronise; median and spread per route.  No threshold: the
record is the deliverable.

The device routes also carry the kernels' own time (the library's event pairs around its launches, rdr_set_profiling), so that the
wrapper's share - an output allocation, two launches, the read-back of six numbers - can be told from the kernels'.

--ab PARENT_DIR THIS_DIR adds bench.py's headline (G rays/s) from two built checkouts, alternated as tools/ab_bench.sh alternates two
libraries (the C ABI grew, so the parent's library does not load under this tree's binding: each side runs its own tree), to show that
the ray kernels did not move.

    python tools/bench_dem.py [--out profiles/r18_dem_sampling.json] [--repeats 3] [--ab ../parent_checkout .]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

SCENE, DEM = 4000, 3600
NODATA = 0.0


def nearest_numpy(dem, gt, x, y):
    """The restatement of tests/test_gpu_llreader.py: floor of the f64 quotient, NaN outside."""
    col = np.floor((x - gt[0]) / gt[1]); row = np.floor((y - gt[3]) / gt[5])
    ok = (col >= 0) & (col < dem.shape[1]) & (row >= 0) & (row < dem.shape[0])
    out = np.full(x.shape, np.nan)
    out[ok] = dem[row[ok].astype(np.int64), col[ok].astype(np.int64)]
    return out


def summary(seconds):
    return dict(seconds=seconds, median=statistics.median(seconds), spread=max(seconds) - min(seconds))


def headline(tree):
    out = subprocess.run([sys.executable, 'bench.py', '--gpus', '1', '--steps', '20', '--warmup', '5', '--cpu-sample', '0', '--no-e2e', '--no-secondary'],
                         cwd=str(Path(tree).resolve()), env={k: v for k, v in os.environ.items() if k != 'RAIDER_HIP_LIB'}, capture_output=True, text=True,
                         timeout=900)
    if out.returncode != 0:
        raise RuntimeError(f'bench.py in {tree} failed:\n{out.stderr[-2000:]}')
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{')][-1])
    return dict(g_rays_per_s=d['value'] / 1e9, ms_per_step=d.get('ms_per_step'), library_source_hash=d.get('roofline', {}).get('library_source_hash'))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'r18_dem_sampling.json'))
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--ab', nargs=2, metavar=('PARENT_DIR', 'THIS_DIR'))
    args = ap.parse_args()
    import torch
    from raider_amd import Context, _lib as L
    from raider_amd.interpolator import raster_bounds, raster_sample
    ctx = Context.default()
    result = dict(device=ctx.device_info()[0], source_hash=L.source_hash(), scene=[SCENE, SCENE], dem=[DEM, DEM], dem_dtype='int16', repeats=args.repeats)

    # a tilted radar-geometry scene over one 1 x 1 degree DEM tile, a margin of it outside the tile, a no-data border as ISCE leaves one
    rng = np.random.default_rng(18)
    r, c = np.meshgrid(np.linspace(-0.55, 0.55, SCENE), np.linspace(-0.55, 0.55, SCENE), indexing='ij')
    lat = 34.5 + 0.995 * r + 0.087 * c
    lon = -117.5 + 0.995 * c - 0.087 * r
    lat[:, :40] = NODATA; lon[:, :40] = NODATA
    gt = (-118.0, 1.0 / DEM, 0.0, 35.0, 0.0, -1.0 / DEM)
    dem = rng.integers(-100, 4000, (DEM, DEM)).astype(np.int16)
    dlat, dlon, ddem = torch.from_numpy(lat).cuda(), torch.from_numpy(lon).cuda(), torch.from_numpy(dem).cuda()
    n = lat.size

    def sync(v):
        ctx.synchronize(); torch.cuda.synchronize()
        return v

    def np_bounds():
        out = []
        for a in (lat, lon):
            m = np.where(a == NODATA, np.nan, a)
            out.append((np.nanmin(m), np.nanmax(m)))
        return out
    routes_b = dict(numpy=np_bounds, device_tensors=lambda: raster_bounds(dlat, dlon, nodata=NODATA), host_arrays=lambda: raster_bounds(lat, lon, nodata=NODATA))
    routes_s = dict(numpy_nearest=lambda: nearest_numpy(dem, gt, lon, lat),
                    device_nearest=lambda: sync(raster_sample(ddem, gt, dlon, dlat)), host_nearest=lambda: raster_sample(dem, gt, lon, lat),
                    device_linear=lambda: sync(raster_sample(ddem, gt, dlon, dlat, 'linear')), host_linear=lambda: raster_sample(dem, gt, lon, lat, 'linear'))

    # the results agree before anything is timed
    want_b = np_bounds()
    for name in ('device_tensors', 'host_arrays'):
        got = routes_b[name]()
        assert [g[:2] for g in got] == want_b, (name, got, want_b)
    want_s = routes_s['numpy_nearest']()
    for name in ('device_nearest', 'host_nearest'):
        got = routes_s[name]()
        got = got.cpu().numpy() if hasattr(got, 'cpu') else got
        assert np.array_equal(got.view(np.int64), want_s.view(np.int64)), name
    result['valid_heights'] = int(np.isfinite(want_s).sum())
    del want_s, got

    for key, routes in (('bounds', routes_b), ('sampling', routes_s)):
        times = {name: [] for name in routes}
        for fn in routes.values():
            fn()                                                             # warm-up
        for _ in range(args.repeats):
            for name, fn in routes.items():
                sync(None)
                t0 = time.perf_counter()
                fn()
                sync(None)
                times[name].append(time.perf_counter() - t0)
        result[key] = {name: summary(t) for name, t in times.items()}
        for name, fn in routes.items():                                      # the kernels alone: event pairs around the library's launches
            if name.startswith('device'):
                ctx.set_profiling(True)
                for _ in range(args.repeats):
                    fn()
                count, ms = ctx.profile_get(3 if key == 'bounds' else 2)
                ctx.set_profiling(False)
                result[key][name]['kernel_ms'] = ms / args.repeats
                result[key][name]['launch_brackets'] = count // args.repeats
        print(key, json.dumps({name: round(v['median'] * 1e3, 3) for name, v in result[key].items()}), 'ms (median)', flush=True)
    # bytes the device routes must move, from the shapes, over the kernels' own time
    result['bounds']['bytes_read'] = 2 * n * 8
    result['sampling']['bytes_moved_nearest'] = n * (8 + 8 + 8 + 2)             # x, y, out and - at best - each DEM pixel once per point
    b, sn, sl = result['bounds']['device_tensors'], result['sampling']['device_nearest'], result['sampling']['device_linear']
    b['kernel_gb_per_s'] = result['bounds']['bytes_read'] / (b['kernel_ms'] * 1e-3) / 1e9
    sn['kernel_gb_per_s'] = result['sampling']['bytes_moved_nearest'] / (sn['kernel_ms'] * 1e-3) / 1e9
    sn['g_points_per_s'], sl['g_points_per_s'] = n / sn['median'] / 1e9, n / sl['median'] / 1e9

    if args.ab:
        del dlat, dlon, ddem
        ctx.trim(0); torch.cuda.empty_cache()
        runs = {lib: [] for lib in args.ab}
        for _ in range(3):
            for lib in args.ab:
                runs[lib].append(headline(lib))
                print(lib, runs[lib][-1], flush=True)
        result['bench_headline'] = {('parent' if lib == args.ab[0] else 'this'): dict(runs=r, median_g_rays_per_s=statistics.median(x['g_rays_per_s'] for x in r))
                                    for lib, r in runs.items()}
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + '\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
