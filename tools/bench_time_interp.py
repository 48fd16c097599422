#!/usr/bin/env python3
"""Time the 'azimuth_time_grid' combination of three f32 weather-model epochs (pointwise and total cubes) two ways, on the same
inputs in one process: the staged chain of raider_amd.s1_azimuth_timing (get_azimuth_time_grid -> get_inverse_weights_for_dates
-> combine_cubes, what combine_weather_files takes for an orbit beyond the kernel's LDS tables) and the one-pass entry
(combine_cubes_azimuth_time, rdr_cube_blend_azimuth_time).

Sizes: the HRRR level count (57 levels, raider_amd/data/hrrr_l50.npz) on a 600 x 600 grid, and a GUNW-sized 300 x 300 grid.  The
orbit is a Sentinel-1-like cut of +-600 s: 121 state vectors.  Before anything is timed the two routes are compared as the GPU test
compares them (the staged combination on the entry's own time grid: the same bytes; the staged time grid: within one millisecond
tick).  Then a warm-up and three repeats, the routes alternating; the host clock around a call that ends in a synchronise.  Device
bytes per route: what stays allocated when the call has returned (hipMemGetInfo before / after, results included) and what rdr_trim
then gives back (scratch: the staged route's mesh, time-grid and weight staging).

    python tools/bench_time_interp.py [--out profiles/r14_time_interp.json] [--sizes 600,300] [--repeats 3]
"""
import argparse
import datetime as dt
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

DATES = [dt.datetime(2021, 1, 1, 7), dt.datetime(2021, 1, 1, 6), dt.datetime(2021, 1, 1, 8)]


def orbit():
    from raider_amd.orbits import Orbit
    t = np.arange(-600.0, 600.0 + 1e-9, 10.0)
    r, w_ = 7.07e6, 2 * np.pi / 5900.0
    lat0, lon0 = np.radians(30.5), np.radians(-100.0)
    pos = np.stack([r * np.cos(lat0 + w_ * t) * np.cos(lon0), r * np.cos(lat0 + w_ * t) * np.sin(lon0), r * np.sin(lat0 + w_ * t)], -1)
    vel = np.stack([-r * w_ * np.sin(lat0 + w_ * t) * np.cos(lon0), -r * w_ * np.sin(lat0 + w_ * t) * np.sin(lon0), r * w_ * np.cos(lat0 + w_ * t)], -1)
    epoch = dt.datetime(2021, 1, 1, 6, 57, 0)
    return Orbit([epoch + dt.timedelta(seconds=float(x)) for x in t], pos, vel, epoch=epoch)


def scene(n, zs):
    import torch
    from raider_amd import Cube
    half = 0.5 * n * 0.027                                                # ~3 km nodes
    ys, xs = np.linspace(30.5 - half, 30.5 + half, n), np.linspace(-104.0 - half, -104.0 + half, n)
    X, Y = np.meshgrid(xs - xs.mean(), ys - ys.mean())
    c, s = np.cos(np.radians(4.0)), np.sin(np.radians(4.0))
    lat2, lon2 = np.ascontiguousarray(ys.mean() + X * s + Y * c), np.ascontiguousarray(xs.mean() + X * c - Y * s)
    g = torch.Generator(device='cuda').manual_seed(14)
    fields = [torch.rand((zs.size, n, n), generator=g, device='cuda', dtype=torch.float32) * 60 + 0.5 for _ in range(4)]
    pw = [Cube(ys, xs, zs, fields[i], fields[i + 1], order='zyx') for i in range(3)]
    tot = [Cube(ys, xs, zs, fields[i + 1], fields[i], order='zyx') for i in range(3)]
    torch.cuda.synchronize()
    return ys, xs, lat2, lon2, pw, tot


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'r14_time_interp.json'))
    ap.add_argument('--sizes', default='600,300')
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    import torch
    from raider_amd import Context, _lib as L
    from raider_amd import s1_azimuth_timing as S
    zs = np.sort(np.load(REPO / 'raider_amd' / 'data' / 'hrrr_l50.npz')['level_heights'].astype(np.float64))
    orb = orbit()
    ctx = Context.default()
    result = dict(device=ctx.device_info()[0], source_hash=L.source_hash(), nsv=int(orb.time.size), nz=int(zs.size), epochs=3, sizes=[])

    def same(a, b):
        return all(x.tobytes() == y.tobytes() for x, y in zip(a.read(), b.read()))

    for n in (int(v) for v in args.sizes.split(',')):
        ys, xs, lat2, lon2, pw, tot = scene(n, zs)
        shape = (zs.size, n, n)
        nvox = int(np.prod(shape))

        def staged():
            grid = S.get_azimuth_time_grid(np.broadcast_to(lon2, shape), np.broadcast_to(lat2, shape), np.broadcast_to(zs[:, None, None], shape), orb, ctx=ctx)
            out = S.combine_weather_cubes_azimuth_time(pw, tot, DATES, grid, ctx=ctx)
            ctx.synchronize()
            return out, grid

        def fused(grid=False):
            out = S.combine_cubes_azimuth_time(pw, tot, DATES, lat2, lon2, orb, return_time_grid=grid, ctx=ctx)
            ctx.synchronize()
            return out

        def held(fn):
            ctx.trim(0); ctx.synchronize()
            free0 = torch.cuda.mem_get_info()[0]
            out = fn()
            after = free0 - torch.cuda.mem_get_info()[0]
            del out
            return dict(allocated_after_call=int(after), released_by_trim=int(ctx.trim(0)))

        # the outputs agree, as in tests/test_gpu_time_interp.py
        fp, ft, fgrid = fused(grid=True)
        sp, st = S.combine_weather_cubes_azimuth_time(pw, tot, DATES, fgrid, ctx=ctx)
        assert same(fp, sp) and same(ft, st), 'the staged chain on the entry\'s time grid gives other bytes'
        (sp2, st2), sgrid = staged()
        ticks = np.abs((sgrid - np.datetime64(DATES[0], 'ms')).astype(np.int64) - np.rint(fgrid * 1e3).astype(np.int64))
        assert ticks.max() <= 1 and (ticks > 0).mean() < 0.01, (int(ticks.max()), float((ticks > 0).mean()))
        moved = int((ticks > 0).sum())
        del fp, ft, sp, st, sp2, st2, sgrid, fgrid, ticks
        mem = dict(staged=held(staged), fused=held(fused))
        times = dict(staged=[], fused=[])
        staged(); fused()                                                 # warm-up
        for _ in range(args.repeats):
            for name, fn in (('staged', staged), ('fused', fused)):
                t0 = time.perf_counter()
                out = fn()
                times[name].append(time.perf_counter() - t0)
                del out
        entry = dict(grid=[int(v) for v in shape], voxels=nvox, ticks_moved=moved,
                     arithmetic_bytes=dict(sources=6 * nvox * 8, outputs=2 * nvox * 16,
                                           staged_extra=dict(ecef_upload=nvox * 24, los_aztime_range=nvox * 40, seconds_upload=nvox * 8, weights=3 * nvox * 8 * 2),
                                           fused_extra=dict(lat_lon=2 * n * n * 8)),
                     device_bytes=mem)
        for name in ('staged', 'fused'):
            entry[name] = dict(seconds=times[name], median=statistics.median(times[name]), spread=max(times[name]) - min(times[name]))
        entry['fused_faster_in_every_repeat'] = bool(all(f < s for f, s in zip(times['fused'], times['staged'])))
        entry['speedup_median'] = entry['staged']['median'] / entry['fused']['median']
        result['sizes'].append(entry)
        print(json.dumps(entry), flush=True)
        del pw, tot
        ctx.trim(0)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(result, indent=1) + '\n')
    print('wrote', args.out)


if __name__ == '__main__':
    main()
