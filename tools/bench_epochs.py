"""Time series of weather epochs through one ray geometry: the one-epoch loop (Cube.raytrace_slices per date) against the stacked call
(raytrace_slices_epochs) at every shipped epochs-per-launch E, on the configs[2] geometry (scene_grid(4000, 4000), per-column incidence,
heading -167.9) with D epochs of synthetic_cube(300, 300, 80, seed=e).  Device-resident rays and outputs (no PCIe in the timing).
Prints ONE JSON line; --f64 adds a float64 (blended) epoch set, --era5 ERA5's 145 real levels.

    python tools/bench_epochs.py [--epochs 8] [--reps 3] [--rows 4000] [--f64] [--era5] [--out profiles/<name>.json]

--per-pixel-ht: the DEM scene of DESIGN 5c instead (bench.py --per-pixel-ht: scene_grid(4000, 4000), per-pixel look vectors, heights
rng(2).uniform(0, 3000)), f32 and f64 epoch sets: a loop of Cube.raytrace per date against ONE raytrace_epochs call, at every epochs-per-launch
setting; per-date milliseconds of every repeat, their median and spread (max - min).  --root DIR imports raider_amd from another
checkout - a build of the parent commit, which has the loop only.  --merge NEW.json PARENT.json [PARENT2.json ...] joins such runs
(no GPU needed) into the file DESIGN 5d quotes: stacked against the parent's loop, and which (dtype, E) stay stacked.

    python tools/bench_epochs.py --per-pixel-ht [--reps 7] [--root DIR] --out <run>.json
    python tools/bench_epochs.py --merge <new>.json <parent>.json ... --out profiles/<name>.json
"""
import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np

def _stats(per_date):
    return dict(ms_per_date=statistics.median(per_date), spread_ms=max(per_date) - min(per_date), repeats_ms_per_date=per_date)


def per_pixel(a):
    """the DEM scene: loop of Cube.raytrace per date against one raytrace_epochs call (when the imported package has it)"""
    import torch
    import raider_amd as R
    from raider_amd import _lib
    from raider_amd.synthetic import scene_grid, synthetic_cube
    dev = torch.device('cuda:0')
    ctx = R.Context.default()
    xp, yp, inc_cols, hd = scene_grid(a.rows, a.rows)
    xp_t = torch.from_numpy(xp).to(dev); yp_t = torch.from_numpy(yp).to(dev)
    inc_t = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(inc_cols, (yp.size, xp.size)))).to(dev)
    los_t = R.Rays.grid(xp_t, yp_t, inc=inc_t, hd=torch.full(inc_t.shape, hd, dtype=torch.float64, device=dev)).look_vectors(ctx)
    del inc_t
    hts = np.random.default_rng(2).uniform(0.0, 3000.0, (yp.size, xp.size))
    rays = R.Rays.grid(xp_t, yp_t, los=los_t, hts=torch.from_numpy(hts).to(dev))
    stacked_fn = getattr(R, 'raytrace_epochs', None)
    D = a.epochs
    inner = 4                  # the D-date work this many times per timed window (a window of ~0.2 s)

    def timed(fn):
        fn(); torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / (inner * D))
        return ts

    out = dict(tool='bench_epochs --per-pixel-ht', rays=int(xp.size * yp.size), epochs=D, reps=a.reps, windows_per_repeat=inner,
               source_hash=_lib.load().rdr_source_hash().decode(), rdr_version=_lib.load().rdr_version(), has_stacked=stacked_fn is not None, sets=[])
    end = ctx.clock_sample(200.0)
    for dtype in ('f32', 'f64'):
        cs = [synthetic_cube(300, 300, 80, seed=e) for e in range(D)]
        if dtype == 'f64':
            cubes = [R.Cube(c['ys'], c['xs'], c['zs'], 0.5 * (c['wet'].astype(np.float64) + d['wet']), 0.5 * (c['hydro'].astype(np.float64) + d['hydro']),
                            order='zyx') for c, d in zip(cs, cs[1:] + cs[:1])]
        else:
            cubes = [R.Cube(c['ys'], c['xs'], c['zs'], c['wet'], c['hydro'], order='zyx') for c in cs]
        zref = float(cs[0]['zs'].max() - 1)
        lw = torch.empty((D, yp.size, xp.size), dtype=torch.float64, device=dev); lh = torch.empty_like(lw)

        def loop():
            for e, cb in enumerate(cubes):
                cb.raytrace(rays, None, zref, out=(lw[e], lh[e]), want_nparts=False)
        res = dict(set=dtype, dtype=np.dtype(cubes[0].dtype).name, loop=_stats(timed(loop)))
        if stacked_fn is not None:
            sw = torch.empty_like(lw); sh = torch.empty_like(lw)

            def stacked():
                stacked_fn(cubes, rays, None, zref, out=(sw, sh), want_nparts=False)
            res['stacked'] = {}
            knob = 'RAIDER_HIP_EPOCHS_MAX' if dtype == 'f32' else 'RAIDER_HIP_EPOCHS_PR_F64_MAX'
            for emax in (1, 2, 4):
                os.environ[knob] = str(emax)
                st = _stats(timed(stacked))
                torch.cuda.synchronize()
                st['bit_identical'] = bool(torch.equal(sw, lw) and torch.equal(sh, lh))
                ctx.set_profiling(True)
                stacked(); torch.cuda.synchronize()
                pre = ctx.profile_get(0); mar = ctx.profile_get(1)
                ctx.set_profiling(False)
                st.update(prepass_launches=pre[0], prepass_ms=pre[1], march_launches=mar[0], march_ms=mar[1])
                if emax > 1:
                    attr = cubes[0].ray_kernel_attributes(6 if emax == 2 else 7)
                    st.update(vgpr=attr['vgpr'], scratch=attr['scratch'])
                res['stacked'][f'E{emax}'] = st
            os.environ.pop(knob, None)
            res['stacked']['default'] = _stats(timed(stacked))
            res['loop_again'] = _stats(timed(loop))          # (the same loop after the stacked runs: drift of the box)
        out['sets'].append(res)
        del cubes
    out['shader_clock_ghz'] = end()
    return out


def merge(files):
    """NEW.json + PARENT.json ... -> the stacked call against the parent build's loop"""
    new = json.loads(Path(files[0]).read_text())
    parents = [json.loads(Path(f).read_text()) for f in files[1:]]
    out = dict(tool='bench_epochs --merge', rays=new['rays'], epochs=new['epochs'], shader_clock_ghz=new.get('shader_clock_ghz'),
               source_hash=new['source_hash'], parent_source_hash=parents[0]['source_hash'], parent_runs=len(parents), sets=[])
    for k, s in enumerate(new['sets']):
        reps = [t for p in parents for t in p['sets'][k]['loop']['repeats_ms_per_date']]
        base = _stats(reps)
        r = dict(set=s['set'], parent_loop=base, loop=s['loop'], loop_again=s['loop_again'], stacked=s['stacked'])
        r['verdict'] = {}
        for name, st in s['stacked'].items():
            gain = base['ms_per_date'] - st['ms_per_date']
            r['verdict'][name] = dict(speedup_vs_parent_loop=base['ms_per_date'] / st['ms_per_date'], gain_ms_per_date=gain,
                                      larger_spread_ms=max(base['spread_ms'], st['spread_ms']),
                                      faster_beyond_spread=bool(gain > max(base['spread_ms'], st['spread_ms'])))
        out['sets'].append(r)
    out['bit_identical'] = all(st.get('bit_identical', True) for s in new['sets'] for st in s['stacked'].values())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--per-pixel-ht', action='store_true')
    ap.add_argument('--root', default=None)
    ap.add_argument('--merge', nargs='+', default=None)
    ap.add_argument('--epochs', type=int, default=8)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--rows', type=int, default=4000)
    ap.add_argument('--f64', action='store_true')
    ap.add_argument('--era5', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.merge or a.per_pixel_ht:
        if a.merge:
            out = merge(a.merge)
        else:
            sys.path.insert(0, str(Path(a.root).resolve() if a.root else Path(__file__).resolve().parent.parent))
            out = per_pixel(a)
        line = json.dumps(out)
        print(line)
        if a.out:
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(line + '\n')
        return
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
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
