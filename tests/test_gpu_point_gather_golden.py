"""GPU: every route of the point gather against FIXED words (tests/golden/g19_point_gather.npz, tools/gen_golden_point_gather.py).
The bit-for-bit tests of test_gpu_points.py, test_gpu_parity.py and test_gpu_point_epochs.py compare the routes with each other, so a
change made to all of them at once would pass; here the plain route's float64 outputs, recorded as uint64 before the routes were
folded into one body, pin each of them - NaNs included, no tolerance."""
import functools
from pathlib import Path

import numpy as np
import pytest

SCENES = ('a32', 'a64', 'b32', 'b64', 'c32', 'c64', 'd32')      # 5x2x2, 4x3x7, 12x9x20 in both dtypes; d: 6200x2x2, axes beyond the LDS table


@functools.lru_cache(maxsize=None)
def _golden():
    g = dict(np.load(Path(__file__).parent / 'golden' / 'g19_point_gather.npz'))
    for v in g.values():
        v.setflags(write=False)
    return g


def _scene(scene):
    """(axes, fields in the scene's dtype, points, expected wet / hydro words)"""
    g = _golden()
    k = scene[0]
    dt = np.float32 if scene.endswith('32') else np.float64
    return (g[f'{k}_ys'], g[f'{k}_xs'], g[f'{k}_zs']), (g[f'{k}_wet'].astype(dt), g[f'{k}_hydro'].astype(dt)), g[f'{k}_pts'], \
        (g[f'{scene}_wet_words'], g[f'{scene}_hyd_words'])


def _cube(scene):
    import raider_amd as R
    (ys, xs, zs), (wet, hyd), _, _ = _scene(scene)
    return R.Cube(ys, xs, zs, wet, hyd, order='zyx')


def _words(a):
    a = a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check(res, want, what):
    for got, exp, name in zip(res, want, ('wet', 'hydro')):
        got = _words(got)
        bad = np.flatnonzero(got != exp)
        assert bad.size == 0, f'{what}: {bad.size} {name} words differ, first at point {bad[0]}: {got[bad[0]]:#x} != {exp[bad[0]]:#x}'


@pytest.mark.parametrize('scene', SCENES)
def test_fixture_is_the_scene_the_generator_describes(scene):
    """(needs no GPU) about three quarters of the points inside (the condition of the fixture, not a measurement), the fixed rows 0-5,
    finite fields"""
    (ys, xs, zs), (wet, hyd), pts, (ww, hw) = _scene(scene)
    w = ww.view(np.float64)
    assert pts.shape == (1024, 3) and ww.shape == hw.shape == (1024,)
    assert 0.6 <= np.isfinite(w).mean() <= 0.9 and np.array_equal(np.isfinite(w), np.isfinite(hw.view(np.float64)))
    assert np.array_equal(pts[0], [ys[0], xs[0], zs[0]]) and np.array_equal(pts[1], [ys[-1], xs[-1], zs[-1]]) and pts[3, 1] == xs[-2]
    assert np.isnan(pts[4]).sum() == 1 and pts[5, 2] == np.nextafter(zs[-1], np.inf)
    assert np.isfinite(w[:4]).all() and np.isnan(w[4:6]).all()
    assert np.isfinite(wet).all() and np.isfinite(hyd).all()        # so the blend routes below are exact: no scene leaves them out
    assert (len(ys) + len(xs) + len(zs)) * 8 > 48 * 1024 if scene == 'd32' else len(ys) <= 12


@pytest.mark.gpu
@pytest.mark.parametrize('scene', SCENES)
def test_plain_and_quad_routes_give_the_stored_words(scene):
    import torch
    _, _, pts, want = _scene(scene)
    cube = _cube(scene)
    assert cube.point_index(build=False) == 0
    _check(cube.interp(pts), want, 'plain, host points')
    _check(cube.interp(torch.from_numpy(pts.copy()).cuda()), want, 'plain, device points')
    assert cube.point_index() > 0                                   # from here on the gather reads the corner-quad copy
    _check(cube.interp(pts), want, 'quad')
    cube.point_index(build=False)


@pytest.mark.gpu
@pytest.mark.parametrize('scene', SCENES)
def test_epochs_route_gives_the_stored_words_for_every_epoch(scene):
    """D = 1 .. 4 dates (launch groups 1, 2, 2 + 1, 4), every date the same cube; host arrays take the stacked kernels"""
    import raider_amd as R
    _, _, pts, want = _scene(scene)
    cubes = [_cube(scene) for _ in range(4)]
    y, x, z = (np.ascontiguousarray(pts[:, k]) for k in range(3))
    for D in (1, 2, 3, 4):
        w, h = R.interp_project_epochs(cubes[:D], y, x, z)
        assert w.shape == h.shape == (D, 1024)
        for e in range(D):
            _check((w[e], h[e]), want, f'epochs, D = {D}, epoch {e}')


@pytest.mark.gpu
@pytest.mark.parametrize('scene', SCENES)
def test_blend_and_pair_routes_give_the_stored_words(scene):
    """weights (1, 0) with the cube as both epochs: 1 * a + 0 * a is exact for finite values (every field of the fixture is finite), so
    the blend at the corners and the paired blended cube reproduce the plain route's words"""
    _, _, pts, want = _scene(scene)
    cube = _cube(scene)
    _check(cube.interp_blend(1.0, cube, 0.0, pts), want, 'blend at the corners')
    _check(cube.interp_blend(1.0, cube, 0.0, pts, via_cube=True), want, 'paired blended cube')


@pytest.mark.gpu
@pytest.mark.parametrize('scene', SCENES)
def test_projected_routes_are_the_stored_words_over_the_divisor(scene):
    """proj_mode 3 (a divisor per point) and 1 (an incidence per point; `cosinc` is the divisor the device makes of it): stored / divisor
    in numpy - IEEE division, the same on both sides"""
    import raider_amd as R
    g = _golden()
    _, _, pts, want = _scene(scene)
    cube = _cube(scene)
    y, x, z = (np.ascontiguousarray(pts[:, k]) for k in range(3))
    ww, hw = (v.view(np.float64) for v in want)
    with np.errstate(invalid='ignore'):
        by_div = (_words(ww / g['div']), _words(hw / g['div']))
        by_inc = (_words(ww / g['cosinc']), _words(hw / g['cosinc']))
    _check(cube.interp_project(y, x, z, divisor=g['div']), by_div, 'proj_mode 3')
    _check(cube.interp_project(y, x, z, inc=g['inc']), by_inc, 'proj_mode 1')
    w, h = R.interp_project_epochs([cube, cube, cube], y, x, z, divisor=g['div'])
    for e in range(3):
        _check((w[e], h[e]), by_div, f'epochs, proj_mode 3, epoch {e}')
    w, h = R.interp_project_epochs([cube, cube], y, x, z, inc=np.stack([g['inc'], g['inc']]))
    for e in range(2):
        _check((w[e], h[e]), by_inc, f'epochs, proj_mode 1 with per-date incidences, epoch {e}')
