#!/usr/bin/env python3
"""tests/golden/g19_point_gather.npz: the plain point gather (interp_points_kernel) pinned as raw words, so that a change made to
every gather route at once cannot pass by the routes agreeing with each other.  Run on a GPU at the commit whose bits are to be kept.

The file holds the inputs themselves, not seeds.  Per cube shape (group a: 5 x 2 x 2, b: 4 x 3 x 7, c: 12 x 9 x 20 - descending
uniform y axis, non-uniform z axis, float64 fields that the float32 scenes round; d: 6200 x 2 x 2 float32 with a non-uniform y axis,
whose three axes do not fit the 48 KiB LDS table): <g>_ys, <g>_xs, <g>_zs, <g>_wet, <g>_hydro (fields in (z, y, x) order) and
<g>_pts[1024, 3] = (y, x, z).  Per scene (a32, a64, b32, b64, c32, c64, d32): <scene>_wet_words / <scene>_hyd_words, the float64
outputs of Cube.interp as uint64.  The blend routes of the test take the cube itself as the second epoch.  Shared by every scene:
`div` (a divisor per point, proj_mode 3) and `inc` (an incidence per point, degrees, proj_mode 1) with `cosinc`, the divisor the
device makes of it, cos(inc * DEG_TO_RAD): numpy's cos where the projected outputs agree with it, else the neighbouring double that
reproduces them in every scene (the two libms may differ in the last bit; the test divides by the stored array).

Points: uniform over each axis range widened by 5 % per side (about three quarters inside), rounded to float32 so that the file
compresses; rows 0-5 are fixed: first node, last node, an interior node, x = xs[-2], a NaN coordinate, one ulp beyond zs[-1].

    python tools/gen_golden_point_gather.py [--out tests/golden/g19_point_gather.npz]
"""
import argparse
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

N = 1024
GROUPS = ('a', 'b', 'c', 'd')
SCENES = ('a32', 'a64', 'b32', 'b64', 'c32', 'c64', 'd32')


def make_inputs():
    rng = np.random.default_rng(19)
    G = {}
    for g, (ny, nx, nz) in zip('abc', ((5, 2, 2), (4, 3, 7), (12, 9, 20))):
        ys = np.linspace(30.0, 36.0, ny)[::-1].copy(); xs = np.linspace(-121.0, -113.0, nx)
        zs = np.round(-100 + 30000 * np.linspace(0, 1, nz) ** 2, 3)
        G[g] = dict(ys=ys, xs=xs, zs=zs, wet=rng.normal(100, 30, (nz, ny, nx)), hydro=rng.normal(2000, 300, (nz, ny, nx)))
    ny, nx, nz = 6200, 2, 2          # 6204 doubles of axes > 6144: the kernels read the axes from global memory
    ys = 0.25 * np.cumsum(rng.integers(1, 4, ny)).astype(np.float64)
    G['d'] = dict(ys=ys, xs=np.array([-3.0, 5.0]), zs=np.array([0.0, 700.0]),
                  wet=(rng.integers(0, 16, (nz, ny, nx)) / 4 + 1).astype(np.float32), hydro=(rng.integers(0, 16, (nz, ny, nx)) / 4 + 20).astype(np.float32))
    for g, d in G.items():
        ys, xs, zs = d['ys'], d['xs'], d['zs']
        lo = np.array([ys.min(), xs.min(), zs.min()]); hi = np.array([ys.max(), xs.max(), zs.max()])
        p = rng.uniform(lo - 0.05 * (hi - lo), hi + 0.05 * (hi - lo), (N, 3)).astype(np.float32).astype(np.float64)
        mid = 0.5 * (lo + hi)
        p[0] = [ys[0], xs[0], zs[0]]
        p[1] = [ys[-1], xs[-1], zs[-1]]
        p[2] = [ys[len(ys) // 2], xs[len(xs) // 2], zs[len(zs) // 2]]
        p[3] = [mid[0], xs[-2], mid[2]]
        p[4] = [mid[0], np.nan, mid[2]]
        p[5] = [mid[0], mid[1], np.nextafter(zs[-1], np.inf)]
        d['pts'] = p
    inc = rng.uniform(20.0, 46.0, N)
    div = rng.uniform(0.6, 0.95, N)
    return G, inc, div


def scene_fields(G, scene):
    d = G[scene[0]]
    dt = np.float32 if scene.endswith('32') else np.float64
    return d, d['wet'].astype(dt), d['hydro'].astype(dt)


def words(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64).copy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default='tests/golden/g19_point_gather.npz')
    a = ap.parse_args()
    import raider_amd as R
    G, inc, div = make_inputs()
    out = {f'{g}_{k}': v for g, d in G.items() for k, v in d.items()}
    out['inc'] = inc; out['div'] = div
    proj = {}
    for s in SCENES:
        d, wet, hyd = scene_fields(G, s)
        # the blend routes of the test: w1 = 1, w2 = 0 on the cube itself, in the cube's dtype, is exact for finite values
        for f in (wet, hyd):
            one, zero = f.dtype.type(1), f.dtype.type(0)
            assert np.isfinite(f).all() and ((one * f + zero * f).view(np.uint8) == f.view(np.uint8)).all()
        cube = R.Cube(d['ys'], d['xs'], d['zs'], wet, hyd, order='zyx')
        p = d['pts']
        w, h = (np.array(v) for v in cube.interp(p))
        share = np.isfinite(w).mean()
        assert np.array_equal(np.isfinite(w), np.isfinite(h)) and 0.6 <= share <= 0.9, (s, share)
        assert np.isfinite(w[:4]).all() and np.isnan(w[4:6]).all(), (s, w[:6])
        try:                           # the same share from scipy itself, and the values to round-off
            from scipy.interpolate import RegularGridInterpolator as RGI
            fy = d['ys'][0] > d['ys'][-1]
            ys = d['ys'][::-1] if fy else d['ys']
            for f, got in ((wet, w), (hyd, h)):
                v = f.transpose(1, 2, 0).astype(np.float64)
                ref = RGI((ys, d['xs'], d['zs']), v[::-1] if fy else v, bounds_error=False, fill_value=np.nan)(p)
                assert np.array_equal(np.isfinite(ref), np.isfinite(got)), s
                assert np.nanmax(np.abs(ref - got) / np.abs(ref)) < 1e-13, s
        except ImportError:
            print('scipy is missing: the finite share is the library\'s own')
        out[f'{s}_wet_words'] = words(w); out[f'{s}_hyd_words'] = words(h)
        y, x, z = (np.ascontiguousarray(p[:, k]) for k in range(3))
        pw, ph = (np.array(v) for v in cube.interp_project(y, x, z, divisor=div))
        if not (np.array_equal(words(pw), words(w / div)) and np.array_equal(words(ph), words(h / div))):
            print(f'{s}: proj_mode 3 is NOT the numpy quotient')
        proj[s] = (w, h) + tuple(np.array(v) for v in cube.interp_project(y, x, z, inc=inc))
        print(f'{s}: finite share {share:.3f}')
    # the divisor the device made of inc
    cosinc = np.cos(inc * 0.017453292519943296)
    moved = 0
    for i in range(N):
        cands = [cosinc[i]]
        for step in (1, 2):
            up = dn = cosinc[i]
            for _ in range(step):
                up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
            cands += [up, dn]
        fits = [c for c in cands if all(words(w[i] / c) == words(pw[i]) and words(h[i] / c) == words(ph[i]) for (w, h, pw, ph) in proj.values())]
        assert fits, (i, inc[i])
        moved += fits[0] != cosinc[i]
        cosinc[i] = fits[0]
    print(f'cosinc: {moved} of {N} values differ from numpy\'s cos by an ulp or two')
    out['cosinc'] = cosinc
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(a.out, **out)
    print(a.out, Path(a.out).stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
