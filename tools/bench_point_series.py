"""A date series at query points: the per-date loop against the one stacked call, in the same process on the same box, alternated
`--reps` times; ms per date of every repeat, their median and spread (max - min) on both sides, and whether the bytes agree.

  zenith / projected   tropo_delay's point branch for D dates: 10^6 points, a 150 x 150 x 20 intermediate grid over D synthetic
                       300 x 300 x 80 total-delay cubes.  Host arrays: Cube.point_delays per date against point_delays_epochs.
                       Device tensors: build_delay_cube + interp_project per date against the D builds + one interp_project_epochs.
  gather               the gather stage alone on D 1000 x 1000 x 50 float32 cubes with 5 x 10^6 random points (BASELINE configs[4]'s
                       shape): Cube.interp_project per date (with whatever point index the library's policy builds) against
                       interp_project_epochs, host arrays and device tensors.

    python tools/bench_point_series.py [--epochs 8] [--reps 3] [--points 1000000] [--gather-points 5000000] [--skip-gather]
                                       [--out profiles/r13_point_series.json]
Prints ONE JSON line."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def _stats(per_date):
    return dict(ms_per_date=statistics.median(per_date), spread_ms=max(per_date) - min(per_date), repeats_ms_per_date=per_date)


def _same(a, b):
    import torch
    if hasattr(a, 'is_cuda'):
        return bool(torch.equal(a.view(torch.int64), b.view(torch.int64)))
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def compare(name, D, reps, loop, stacked, sync, extra=None):
    """loop() / stacked() -> (wet[D, n], hydro[D, n]) (lists of D arrays for the loop).  Warm both, size the timed window to >= 0.2 s,
    then alternate them."""
    lw = loop(); sw = stacked(); sync()
    same = all(_same(lw[0][e], sw[0][e]) and _same(lw[1][e], sw[1][e]) for e in range(D))
    t0 = time.perf_counter(); loop(); sync(); once = time.perf_counter() - t0
    inner = max(1, int(np.ceil(0.2 / max(once, 1e-4))))
    tl, ts = [], []
    for _ in range(reps):
        for fn, acc in ((loop, tl), (stacked, ts)):
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            sync()
            acc.append((time.perf_counter() - t0) * 1e3 / (inner * D))
    res = dict(config=name, epochs=D, windows_per_repeat=inner, loop=_stats(tl), stacked=_stats(ts), bit_identical=same)
    gain = res['loop']['ms_per_date'] - res['stacked']['ms_per_date']
    res['speedup'] = res['loop']['ms_per_date'] / res['stacked']['ms_per_date']
    res['faster_beyond_spread'] = bool(gain > max(res['loop']['spread_ms'], res['stacked']['spread_ms']))
    res['slower_beyond_spread'] = bool(-gain > max(res['loop']['spread_ms'], res['stacked']['spread_ms']))
    if extra:
        res.update(extra)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--epochs', type=int, default=8)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--points', type=int, default=1000000)
    ap.add_argument('--gather-points', type=int, default=5000000)
    ap.add_argument('--gather-shape', default='1000x1000x50')
    ap.add_argument('--skip-gather', action='store_true')
    ap.add_argument('--out', default='profiles/r13_point_series.json')
    a = ap.parse_args()
    import torch
    import raider_amd as R
    from raider_amd import _lib
    from raider_amd.synthetic import synthetic_cube
    dev = torch.device('cuda:0')
    ctx = R.Context.default()
    D, n = a.epochs, a.points

    def sync():
        torch.cuda.synchronize(); ctx.synchronize()

    out = dict(tool='bench_point_series', source_hash=_lib.load().rdr_source_hash().decode(), device=ctx.device_info()[0], epochs=D, reps=a.reps, configs=[])
    # ---- the point branch of D dates: zenith, and projected with an incidence array -------------------------------------------------
    cs = [synthetic_cube(300, 300, 80, seed=e) for e in range(D)]
    cubes = [R.Cube(c['ys'], c['xs'], c['zs'], c['wet_total'].astype(np.float32), c['hydro_total'].astype(np.float32), order='zyx') for c in cs]
    del cs
    xp = np.linspace(-119.5, -115.5, 150); yp = np.linspace(34.5, 31.5, 150); zp = np.linspace(0.0, 5000.0, 20)
    rng = np.random.default_rng(0)
    la = rng.uniform(31.5, 34.5, n); lo = rng.uniform(-119.5, -115.5, n); hg = rng.uniform(0.0, 5000.0, n); inc = rng.uniform(25.0, 45.0, n)
    tla, tlo, thg, tinc = (torch.from_numpy(v).to(dev) for v in (la, lo, hg, inc))
    link = lambda proj: dict(bytes_up_per_point_loop=24 + (8 if proj else 0), bytes_up_per_point_and_date_stacked=(24 + (8 if proj else 0)) / D, bytes_down_per_point_and_date=16)
    for name, kw, kwd in (('zenith', {}, {}), ('projected_inc_array', dict(inc=inc), dict(inc=tinc))):
        def loop_host():
            r = [cb.point_delays(xp, yp, zp, la, lo, hg, **kw) for cb in cubes]
            return [x[0] for x in r], [x[1] for x in r]

        def stacked_host():
            return R.point_delays_epochs(cubes, xp, yp, zp, la, lo, hg, **kw)[:2]
        out['configs'].append(compare(f'{name}/host', D, a.reps, loop_host, stacked_host, sync, dict(points=n, grid=[150, 150, 20], **link(bool(kw)))))

        def loop_dev():
            r = [cb.build_delay_cube(xp, yp, zp).interp_project(tla, tlo, thg, **kwd) for cb in cubes]
            return [x[0] for x in r], [x[1] for x in r]

        def stacked_dev():
            return R.interp_project_epochs([cb.build_delay_cube(xp, yp, zp) for cb in cubes], tla, tlo, thg, **kwd)
        out['configs'].append(compare(f'{name}/device', D, a.reps, loop_dev, stacked_dev, sync, dict(points=n, grid=[150, 150, 20])))
    del cubes
    # ---- the gather stage alone on large cubes -----------------------------------------------------------------------------------------
    if not a.skip_gather:
        ny, nx, nz = (int(v) for v in a.gather_shape.split('x'))
        ys = np.linspace(30.0, 36.0, ny); xs = np.linspace(-121.0, -113.0, nx); zs = 41000.0 * np.linspace(0.0, 1.0, nz) ** 2
        g = torch.Generator(device=dev); g.manual_seed(0)
        big = []
        for e in range(D):
            w = torch.rand((ny, nx, nz), dtype=torch.float32, device=dev, generator=g); h = torch.rand((ny, nx, nz), dtype=torch.float32, device=dev, generator=g) + 2.0
            big.append(R.Cube(ys, xs, zs, w, h, order='yxz'))
            del w, h
        m = a.gather_points
        py = rng.uniform(30.0, 36.0, m); px = rng.uniform(-121.0, -113.0, m); pz = rng.uniform(0.0, 41000.0, m)
        ty, tx, tz = (torch.from_numpy(v).to(dev) for v in (py, px, pz))
        for where, (y, x, z) in (('host', (py, px, pz)), ('device', (ty, tx, tz))):
            def loop():
                r = [cb.interp_project(y, x, z) for cb in big]
                return [v[0] for v in r], [v[1] for v in r]

            def stacked():
                return R.interp_project_epochs(big, y, x, z)
            res = compare(f'gather/{where}', D, a.reps, loop, stacked, sync, dict(points=m, cube=[ny, nx, nz], dtype='float32'))
            res['loop_point_index_bytes'] = int(_lib.load().rdr_cube_point_index_bytes(big[0].handle))
            out['configs'].append(res)
    out['bit_identical'] = all(c['bit_identical'] for c in out['configs'])
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + '\n')


if __name__ == '__main__':
    main()
