"""Time series of weather epochs through one ray geometry: the one-epoch loop (Cube.raytrace_slices per date) against the stacked call
(raytrace_slices_epochs) at every shipped epochs-per-launch E, on the configs[2] geometry (scene_grid(4000, 4000), per-column incidence,
heading -167.9) with D epochs of synthetic_cube(300, 300, 80, seed=e).  Device-resident rays and outputs (no PCIe in the timing).
Prints ONE JSON line; --f64 adds a float64 (blended) epoch set, --era5 ERA5's 145 real levels.

    python tools/bench_epochs.py [--epochs 8] [--reps 3] [--rows 4000] [--f64] [--era5] [--out profiles/<name>.json]
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=8)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rows', type=int, default=4000)
    ap.add_argument('--f64', action='store_true')
    ap.add_argument('--era5', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch
    import raider_amd as R
    from raider_amd.engine import epoch_groups
    from raider_amd.synthetic import real_level_heights, scene_grid, synthetic_cube
    dev = torch.device('cuda:0')
    ctx = R.Context.default()
    xp, yp, inc_cols, hd = scene_grid(a.rows, a.rows)
    inc = np.broadcast_to(inc_cols, (yp.size, xp.size)).copy()
    rays = R.Rays.grid(torch.from_numpy(xp).to(dev), torch.from_numpy(yp).to(dev), inc=torch.from_numpy(inc).to(dev),
                       hd=torch.full(inc.shape, hd, dtype=torch.float64, device=dev))
    hts = np.array([0.0])

    def epochs(dtype, zs=None):
        nz = 80 if zs is None else zs.size
        cs = [synthetic_cube(300, 300, nz, seed=e, zs=zs) for e in range(a.epochs)]
        if dtype == 'f64':      # float64 cubes, as an azimuth-time blend of neighbouring dates makes them: the mean of dates e and e+1
            cubes = [R.Cube(c['ys'], c['xs'], c['zs'], 0.5 * (c['wet'].astype(np.float64) + d['wet']), 0.5 * (c['hydro'].astype(np.float64) + d['hydro']),
                            order='zyx') for c, d in zip(cs, cs[1:] + cs[:1])]
        else:
            cubes = [R.Cube(c['ys'], c['xs'], c['zs'], c['wet'], c['hydro'], order='zyx') for c in cs]
        return cubes, float(cs[0]['zs'].max() - 1)

    def timed(fn):
        fn(); torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)

    def run_set(name, cubes, zref):
        D = len(cubes)
        loop_out = {}

        def loop():
            for e, cb in enumerate(cubes):
                loop_out[e] = cb.raytrace_slices(rays, hts, zref, want_partition=False)[:2]
        res = dict(set=name, epochs=D, nz=cubes[0].shape[2], dtype=np.dtype(cubes[0].dtype).name)
        res['loop_ms_per_date'] = timed(loop) / D
        res['stacked'] = {}
        ident = True
        for emax in (2, 4):
            os.environ['RAIDER_HIP_EPOCHS_MAX'] = str(emax)
            st = {}

            def stacked():
                st['out'] = R.raytrace_slices_epochs(cubes, rays, hts, zref, want_partition=False)[:2]
            ms = timed(stacked)
            w, h = st['out']
            same = all(torch.equal(w[e], loop_out[e][0]) and torch.equal(h[e], loop_out[e][1]) for e in range(D))
            ident = ident and same
            ctx.set_profiling(True)
            stacked(); torch.cuda.synchronize()
            pre = ctx.profile_get(0); mar = ctx.profile_get(1)
            ctx.set_profiling(False)
            attr = cubes[0].ray_kernel_attributes(4 if emax == 2 else 5)
            res['stacked'][f'E{emax}'] = dict(ms_per_date=ms / D, speedup=res['loop_ms_per_date'] / (ms / D), groups=epoch_groups(D, emax),
                                             prepass_launches=pre[0], prepass_ms=pre[1], march_launches=mar[0], march_ms=mar[1],
                                             vgpr=attr['vgpr'], scratch=attr['scratch'], bit_identical=same)
        os.environ.pop('RAIDER_HIP_EPOCHS_MAX', None)
        ctx.set_profiling(True)
        cubes[0].raytrace_slices(rays, hts, zref, want_partition=False); torch.cuda.synchronize()
        res['single'] = dict(prepass_ms=ctx.profile_get(0)[1], march_ms=ctx.profile_get(1)[1], march_vgpr=cubes[0].ray_kernel_attributes(1)['vgpr'])
        ctx.set_profiling(False)
        res['bit_identical'] = ident
        return res

    out = dict(tool='bench_epochs', rays=int(xp.size * yp.size), layout='pointer-per-epoch', pack_ms=0.0, sets=[])
    end = ctx.clock_sample(200.0)
    cubes, zref = epochs('f32')
    out['sets'].append(run_set('f32', cubes, zref))
    out['shader_clock_ghz'] = end()
    del cubes
    if a.f64:
        cubes, zref = epochs('f64')
        out['sets'].append(run_set('f64', cubes, zref))
        del cubes
    if a.era5:
        cubes, zref = epochs('f32', zs=real_level_heights('era5'))
        out['sets'].append(run_set('f32_era5_145', cubes, zref))
        del cubes
    out['bit_identical'] = all(s['bit_identical'] for s in out['sets'])
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
