"""GPU: a time series of weather epochs through one ray geometry (rdr_raytrace_slices_epochs, tropo_delay_series) - bit for bit what
one call per date gives."""
import datetime as dt
import logging

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import raider_oracle as O

TIGHT = 1e-9          # metres: tests/test_gpu_parity.py's tolerance against the oracle


def _wm(c, scale=1.0, proj=None, dtype=None, hole=False):
    w, h = c['wet'] * scale, c['hydro'] * scale
    if dtype is not None:
        w, h = w.astype(dtype), h.astype(dtype)
    else:
        w, h = w.astype(c['wet'].dtype), h.astype(c['hydro'].dtype)
    if hole:
        w = w.copy(); h = h.copy()
        w[:, 10:14, 12:18] = np.nan; h[:, 10:14, 12:18] = np.nan
    d = dict(x=c['xs'], y=c['ys'], z=c['zs'], wet=w, hydro=h, wet_total=c['wet_total'], hydro_total=c['hydro_total'])
    if proj is not None:
        d['proj'] = proj
    return d


def _epochs(n, ny=40, nx=44, nz=24, **kw):
    """n epochs on one grid with distinct fields: seeds, a per-epoch scale, a NaN block in epoch 2 only"""
    cs = [O.synthetic_cube(ny, nx, nz, seed=10 + e, **kw) for e in range(n)]
    return cs, [1.0 + 0.03 * e for e in range(n)]


def _same_ds(a, b):
    for k in ('wet', 'hydro'):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k
    aa = {k: v for k, v in a.attrs.items() if k != 'history'}; ba = {k: v for k, v in b.attrs.items() if k != 'history'}
    assert repr(aa) == repr(ba)


def _series_vs_loop(files, aoi_factory, los, hl, caplog, route='stacked'):
    from raider_amd.delay import tropo_delay, tropo_delay_series
    dates = [dt.datetime(2020, 1, 1) + dt.timedelta(days=12 * i) for i in range(len(files))]
    caplog.clear()
    with caplog.at_level(logging.CRITICAL):
        ser = tropo_delay_series(dates, files, aoi_factory(), los, hl)
    crit_s = [r.getMessage() for r in caplog.records if r.levelno >= logging.CRITICAL]
    caplog.clear()
    with caplog.at_level(logging.CRITICAL):
        loop = [tropo_delay(t, f, aoi_factory(), los, hl) for t, f in zip(dates, files)]
    crit_l = [r.getMessage() for r in caplog.records if r.levelno >= logging.CRITICAL]
    assert len(ser) == len(loop) and crit_s == crit_l
    for a, b in zip(ser, loop):
        if b[1] is None:
            assert a[1] is None
            _same_ds(a[0], b[0])
        else:
            assert np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)
    assert ser.routes == [route] * len(files), ser.routes
    return ser


def test_series_equals_per_date_lonlat_f32_f64(caplog):
    from raider_amd.delay import GridAOI
    from raider_amd.losreader import Raytracing
    cs, sc = _epochs(5)
    xp = np.linspace(-119.5, -115.5, 37); yp = np.linspace(34.5, 31.5, 29)
    inc = 30.0 + 16.0 * np.arange(37) / 37.0
    los = Raytracing(inc=np.broadcast_to(inc, (29, 37)).copy(), heading=-167.9)
    hl = [0.0, 500.0, 2000.0, 4000.0]
    for dtype in (None, np.float64):
        files = [_wm(c, s, dtype=dtype, hole=(e == 2)) for e, (c, s) in enumerate(zip(cs, sc))]
        ser = _series_vs_loop(files, lambda: GridAOI(xp, yp), los, hl, caplog)
        w0 = np.asarray(ser[0][0]['wet']); w2 = np.asarray(ser[2][0]['wet'])
        assert np.isfinite(w0).all() and np.isnan(w2).any() and not np.array_equal(w0, np.asarray(ser[1][0]['wet']))


def test_series_equals_per_date_lcc_and_polar_stereographic(caplog):
    from raider_amd.delay import GridAOI
    from raider_amd.losreader import Raytracing
    los = Raytracing(inc=38.0, heading=-167.9)
    hl = [0.0, 800.0, 3000.0]
    # HRRR-like LCC grid over the US south-west
    H = dict(lat_1=38.5, lat_2=38.5, lat_0=38.5, lon_0=262.5, a=6371229.0, es=0.0)
    hrrr = '+proj=lcc +lat_1=38.5 +lat_2=38.5 +lat_0=38.5 +lon_0=262.5 +x_0=0 +y_0=0 +a=6371229 +b=6371229 +units=m +no_defs'
    cs, sc = _epochs(3, 50, 60, 20, y0=-9.0e5, y1=1.0e5, x0=-2.2e6, x1=-1.3e6)
    files = [_wm(c, s, proj=hrrr) for c, s in zip(cs, sc)]
    xp = np.linspace(-117.5, -114.0, 21); yp = np.linspace(36.0, 33.5, 17)
    ser = _series_vs_loop(files, lambda: GridAOI(xp, yp), los, hl, caplog)
    assert np.isfinite(np.asarray(ser[0][0]['hydro'])).mean() > 0.9
    # HRRR-AK-like polar-stereographic grid
    par = dict(lat_0=90.0, lat_ts=60.0, lon_0=225.0, a=6371229.0, es=0.0)
    ak = '+proj=stere +lat_0=90 +lon_0=225 +lat_ts=60 +a=6371229 +b=6371229'
    cx, cy = O.stere_forward(61.0, -150.0, **par)
    cs = [O.synthetic_cube(50, 50, 20, seed=20 + e, ztop=26000.0) for e in range(3)]
    for c in cs:
        c['xs'] = cx + 6000.0 * (np.arange(50) - 25); c['ys'] = cy + 6000.0 * (np.arange(50) - 25)
    files = [_wm(c, 1.0 + 0.05 * e, proj=ak) for e, c in enumerate(cs)]
    xp = np.linspace(-150.8, -149.2, 15); yp = np.linspace(61.4, 60.6, 13)
    ser = _series_vs_loop(files, lambda: GridAOI(xp, yp), los, [0.0, 1000.0, 2500.0], caplog)
    assert np.isfinite(np.asarray(ser[0][0]['hydro'])).mean() > 0.9


def test_series_with_generic_rays(caplog):
    """a polar scene: pass 1 classifies rays generic; the stacked call marches them with the generic kernel per epoch"""
    import raider_amd as R
    from raider_amd.delay import GridAOI
    from raider_amd.losreader import Raytracing
    cs = [O.synthetic_cube(12, 40, 6, seed=30 + e, ztop=15000.0, y0=86.0, y1=89.9, x0=-60.0, x1=60.0) for e in range(3)]
    files = [_wm(c, 1.0 + 0.1 * e) for e, c in enumerate(cs)]
    xp = np.linspace(-20.0, 20.0, 9); yp = np.linspace(88.9, 88.0, 7)
    _series_vs_loop(files, lambda: GridAOI(xp, yp), Raytracing(inc=30.0, heading=-167.9), [9300.0, 9800.0, 10500.0], caplog)
    cubes = [R.Cube(c['ys'], c['xs'], c['zs'], c['wet'], c['hydro'], order='zyx') for c in cs]
    rays = R.Rays.grid(xp, yp, inc=30.0, hd=-167.9)
    zref = cs[0]['zs'].max() - 1
    w, h, K, npt, fl = R.raytrace_slices_epochs(cubes, rays, [9300.0, 9800.0], zref)
    assert cubes[0].ctx.generic_ray_count() > 0
    for e, cb in enumerate(cubes):
        w1, h1, K1, np1, f1 = cb.raytrace_slices(rays, [9300.0, 9800.0], zref)
        assert np.array_equal(w[e], w1, equal_nan=True) and np.array_equal(h[e], h1, equal_nan=True)


def _grid_cubes(D, dtype=np.float32, ny=40, nx=44, nz=24):
    import raider_amd as R
    cs, sc = _epochs(D, ny, nx, nz)
    return cs, [R.Cube(c['ys'], c['xs'], c['zs'], (c['wet'] * s).astype(dtype), (c['hydro'] * s).astype(dtype), order='zyx')
                for c, s in zip(cs, sc)]


def test_engine_epochs_equal_single_calls_for_every_grouping():
    import raider_amd as R
    cs, cubes = _grid_cubes(6)
    hole = (cs[3]['wet'] * 1.09).astype(np.float32); hole[:, 22:28, 12:20] = np.nan           # (over the scene)
    cubes[3] = R.Cube(cs[3]['ys'], cs[3]['xs'], cs[3]['zs'], hole, cs[3]['hydro'], order='zyx')
    from raider_amd.synthetic import scene_grid
    _, _, inc_cols, hd = scene_grid(45, 53)
    xp = np.linspace(-119.0, -116.0, 53); yp = np.linspace(34.0, 32.0, 45)
    rays = R.Rays.grid(xp, yp, inc=np.broadcast_to(inc_cols, (45, 53)).copy(), hd=hd)
    hts = np.array([0.0, 300.0, 1500.0])
    zref = cs[0]['zs'].max() - 1
    single = [cb.raytrace_slices(rays, hts, zref, want_nan=True) for cb in cubes]
    for D in range(1, 7):
        w, h, K, npt, fl, nan = R.raytrace_slices_epochs(cubes[:D], rays, hts, zref, want_nan=True)
        assert w.shape == (D, 3, 45, 53) and fl.shape == (D, 3)
        for e in range(D):
            sw, sh, sK, snp, sfl, snan = single[e]
            assert np.array_equal(w[e], sw, equal_nan=True) and np.array_equal(h[e], sh, equal_nan=True), (D, e)
            assert np.array_equal(K, sK) and np.array_equal(npt, snp) and np.array_equal(fl[e], sfl) and np.array_equal(nan[e], snan)
    assert single[3][5].all() and not single[0][5].any()
    # device arrays: the same bits
    import torch
    dev = torch.device('cuda:0')
    rays_d = R.Rays.grid(torch.from_numpy(xp).to(dev), torch.from_numpy(yp).to(dev), inc=torch.from_numpy(np.broadcast_to(inc_cols, (45, 53)).copy()).to(dev),
                         hd=torch.full((45, 53), hd, dtype=torch.float64, device=dev))
    wd, hd_, _, _, _ = R.raytrace_slices_epochs(cubes[:4], rays_d, hts, zref)
    w, h, _, _, _ = R.raytrace_slices_epochs(cubes[:4], rays, hts, zref)
    assert np.array_equal(wd.cpu().numpy(), w, equal_nan=True) and np.array_equal(hd_.cpu().numpy(), h, equal_nan=True)


def test_pass_one_runs_once_and_epochs_do_not_mix():
    import raider_amd as R
    cs, cubes = _grid_cubes(6)
    xp = np.linspace(-119.0, -116.0, 40); yp = np.linspace(34.0, 32.0, 33)
    rays = R.Rays.grid(xp, yp, inc=35.0, hd=-167.9)
    hts = np.array([0.0, 1000.0])
    zref = cs[0]['zs'].max() - 1
    ctx = cubes[0].ctx
    try:
        ctx.set_profiling(True)
        R.raytrace_slices_epochs(cubes[:1], rays, hts, zref)
        one = ctx.profile_get(0)[0]
        ctx.set_profiling(True)                                            # (restarts the counts)
        R.raytrace_slices_epochs(cubes, rays, hts, zref)
        six = ctx.profile_get(0)[0]
        marches = ctx.profile_get(1)[0]
    finally:
        ctx.set_profiling(False)
    assert one >= 1 and six == one and marches >= 2
    w, h, *_ = R.raytrace_slices_epochs(cubes, rays, hts, zref)
    perm = [4, 0, 5, 2, 1, 3]
    wp, hp, *_ = R.raytrace_slices_epochs([cubes[i] for i in perm], rays, hts, zref)
    assert np.array_equal(wp, w[perm]) and np.array_equal(hp, h[perm])


def test_mismatched_epochs_are_refused_by_name():
    import raider_amd as R
    from raider_amd._lib import check
    cs, cubes = _grid_cubes(3)
    rays = R.Rays.grid(np.linspace(-119.0, -116.0, 20), np.linspace(34.0, 32.0, 18), inc=35.0, hd=-167.9)
    zref = cs[0]['zs'].max() - 1
    c = cs[2]
    bad = {
        'z axis': R.Cube(c['ys'], c['xs'], c['zs'] + 1.0, c['wet'], c['hydro'], order='zyx'),
        'dtype': R.Cube(c['ys'], c['xs'], c['zs'], c['wet'].astype(np.float64), c['hydro'].astype(np.float64), order='zyx'),
        'projection': R.Cube(c['ys'], c['xs'], c['zs'], c['wet'], c['hydro'], order='zyx').set_projection_lcc(38.5, 38.5, 38.5, 262.5),
    }
    for what, cb in bad.items():
        with pytest.raises(ValueError, match='epoch 2'):
            R.raytrace_slices_epochs([cubes[0], cubes[1], cb], rays, [0.0], zref)
    with pytest.raises(ValueError, match='per-ray heights'):
        R.raytrace_slices_epochs(cubes, R.Rays.grid(np.linspace(-119.0, -116.0, 20), np.linspace(34.0, 32.0, 18), inc=35.0, hd=-167.9,
                                                    hts=np.zeros((18, 20))), [0.0], zref)


def test_stations_take_the_stacked_route(caplog):
    from raider_amd.delay import PointsAOI
    from raider_amd.losreader import Raytracing
    cs, sc = _epochs(4)
    files = [_wm(c, s, hole=(e == 1)) for e, (c, s) in enumerate(zip(cs, sc))]
    rng = np.random.default_rng(3)
    la = rng.uniform(32.0, 34.0, 300); lo = rng.uniform(-119.0, -116.0, 300); hg = rng.uniform(0.0, 900.0, 300)
    xp = np.linspace(-119.5, -115.5, 31); yp = np.linspace(34.5, 31.5, 27)
    los, hl = Raytracing(inc=39.0, heading=-167.9), [0.0, 500.0, 1500.0, 3000.0]
    ser = _series_vs_loop(files, lambda: PointsAOI(la, lo, hg, xp, yp), los, hl, caplog)
    # tropo_delay_point_series runs the same stacked call (_stacked_point_rays): the same bytes per date - the NaNs of the holed date
    # where they are - and the same routes
    from raider_amd.delay import tropo_delay_point_series
    dates = [dt.datetime(2020, 1, 1) + dt.timedelta(days=12 * i) for i in range(len(files))]
    pser = tropo_delay_point_series(dates, files, PointsAOI(la, lo, hg, xp, yp), los, hl)
    assert len(pser) == len(ser) == 4 and pser.routes == ser.routes
    for a, b in zip(ser, pser):
        for u, v in zip(a, b):
            u, v = np.asarray(u), np.asarray(v)
            assert u.shape == v.shape == (300,) and u.dtype == v.dtype == np.float64 and u.tobytes() == v.tobytes()


def test_fallbacks_route_per_date(caplog):
    from raider_amd.delay import GridAOI, PointsAOI
    from raider_amd.losreader import Conventional, Raytracing, Zenith
    cs, sc = _epochs(3)
    files = [_wm(c, s) for c, s in zip(cs, sc)]
    xp = np.linspace(-119.5, -115.5, 21); yp = np.linspace(34.5, 31.5, 17)
    hl = [0.0, 500.0, 1500.0]
    _series_vs_loop(files, lambda: GridAOI(xp, yp), Zenith(), hl, caplog, route='per-date')
    rng = np.random.default_rng(4)
    la = rng.uniform(32.0, 34.0, 100); lo = rng.uniform(-119.0, -116.0, 100); hg = rng.uniform(0.0, 900.0, 100)
    inc = rng.uniform(30.0, 45.0, 100)
    _series_vs_loop(files, lambda: PointsAOI(la, lo, hg, xp, yp), Conventional(inc=inc, heading=0 * inc), hl, caplog, route='per-date')
    los = Raytracing(inc=38.0, heading=-167.9)
    _series_vs_loop(files[:1], lambda: GridAOI(xp, yp), los, hl, caplog, route='per-date')
    # one epoch on another grid: the others still share their pass 1
    from raider_amd.delay import tropo_delay_series
    odd = dict(files[1], z=files[1]['z'] + 1.0)
    ser = tropo_delay_series([dt.datetime(2020, 1, d) for d in (1, 2, 3)], [files[0], odd, files[2]], GridAOI(xp, yp), los, hl)
    assert ser.routes == ['stacked', 'per-date', 'stacked']
    odd32 = dict(files[1], wet=files[1]['wet'].astype(np.float64), hydro=files[1]['hydro'].astype(np.float64))
    ser = tropo_delay_series([dt.datetime(2020, 1, d) for d in (1, 2)], [files[0], odd32], GridAOI(xp, yp), los, hl)
    assert ser.routes == ['per-date', 'per-date']
    _series_vs_loop([files[0], odd32], lambda: GridAOI(xp, yp), los, hl, caplog, route='per-date')


def test_one_stacked_epoch_against_the_c_oracle():
    import raider_amd as R
    from oracle import oracle_c as OC
    cs, cubes = _grid_cubes(3)
    xp = np.linspace(-119.0, -116.0, 26); yp = np.linspace(34.0, 32.0, 21)
    yy, xx = np.meshgrid(yp, xp, indexing='ij')
    los = O.look_vectors_from_inc_hd(np.full(yy.shape, 36.0), np.full(yy.shape, -167.9), yy, xx, np.full(yy.shape, 500.0))
    zref = cs[0]['zs'].max() - 1
    w, h, K, npt, fl = R.raytrace_slices_epochs(cubes, R.Rays.grid(xp, yp, los=np.ascontiguousarray(los)), [500.0], zref)
    c = dict(cs[1], wet=(cs[1]['wet'] * 1.03).astype(np.float32), hydro=(cs[1]['hydro'] * 1.03).astype(np.float32))
    ow, oh, onp = OC.build_cube_ray_slice(c, xp, yp, 500.0, los, zref)
    assert np.array_equal(npt[0, :K[0]], onp)
    np.testing.assert_allclose(w[1, 0], ow, rtol=0, atol=TIGHT)
    np.testing.assert_allclose(h[1, 0], oh, rtol=0, atol=TIGHT)


def test_small_slice_budget_chunks_the_series(monkeypatch, caplog):
    from raider_amd.delay import GridAOI
    from raider_amd.losreader import Raytracing
    cs, sc = _epochs(3)
    files = [_wm(c, s) for c, s in zip(cs, sc)]
    xp = np.linspace(-119.5, -115.5, 21); yp = np.linspace(34.5, 31.5, 17)
    monkeypatch.setenv('RAIDER_HIP_SLICE_BUDGET_BYTES', str(21 * 17 * 200))      # two slices per call
    with caplog.at_level(logging.INFO):
        _series_vs_loop(files, lambda: GridAOI(xp, yp), Raytracing(inc=38.0, heading=-167.9), [0.0, 300.0, 900.0, 1800.0, 3000.0], caplog)


# The one-cube marcher and the stacked one run the same two level loops (raider_kernels.h: march_slice_levels, march_ray_height_levels)
# in EVERY horizontal-grid variant, not only on exactly uniform axes.  The axes choose the instantiation (raider_hip.hip:
# axis_uniformity -> march_grid):
#   regular   np.linspace axes: uniform to round-off (worst node < 1e-11 cells off) -> GRID = 1, REGULAR, sliced and per-ray heights
#   tables    the same axes rounded through float32: ~1e-6 cells off, so not exact but nearly uniform on both axes -> GRID = 2, TABLES,
#             for the slices; per-ray heights are not built for TABLES and fall back to GRID = 0, run-time flags (uni = 1)
#   flags     one node of the y axis moved by a quarter of a spacing: y is not exact any more, x still is -> neither REGULAR (both exact)
#             nor TABLES (neither exact), whichever side of the 0.25-cell bound of "nearly uniform" round-off puts y: GRID = 0, run-time
#             flags (exact_x = 1, exact_y = 0), sliced and per-ray heights
_FOLD_NY, _FOLD_NX, _FOLD_NZ, _FOLD_D = 12, 14, 9, 7          # 7 epochs: the groups 4 + 2 + 1

_STAGE_OFF_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
import raider_amd as R
d = np.load(sys.argv[2])
cube = R.Cube(d['ys'], d['xs'], d['zs'], d['wet'], d['hydro'], order='zyx')
rays = R.Rays.grid(d['xp'], d['yp'], inc=d['inc'], hd=-167.9)
w, h, K, npt, fl = cube.raytrace_slices(rays, d['hts'], float(d['zref']))
np.savez(sys.argv[3], w=w, h=h, K=K, npt=npt, fl=fl)
"""


def _fold_axes(c, kind):
    ys, xs = c['ys'].copy(), c['xs'].copy()
    if kind == 'tables':
        ys, xs = ys.astype(np.float32).astype(np.float64), xs.astype(np.float32).astype(np.float64)
    elif kind == 'flags':
        ys[5] += 0.25 * (ys[1] - ys[0])
    return ys, xs


@pytest.mark.parametrize('kind', ['regular', 'tables', 'flags'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_stacked_equals_single_in_every_grid_variant(dtype, kind, tmp_path):
    import os
    import subprocess
    import sys
    import raider_amd as R
    cs, sc = _epochs(_FOLD_D, _FOLD_NY, _FOLD_NX, _FOLD_NZ)
    ys, xs = _fold_axes(cs[0], kind)
    fields = [((c['wet'] * s).astype(dtype), (c['hydro'] * s).astype(dtype)) for c, s in zip(cs, sc)]
    cubes = [R.Cube(ys, xs, c['zs'], w, h, order='zyx') for c, (w, h) in zip(cs, fields)]
    zref = float(cs[0]['zs'].max() - 1)
    # 21 x 37 pixels over the cube's interior: partial 16 x 16 tiles in both directions
    ny, nx = 21, 37
    xp = np.linspace(-119.5, -115.5, nx); yp = np.linspace(34.5, 31.5, ny)
    inc = np.broadcast_to(30.0 + 16.0 * np.arange(nx) / nx, (ny, nx)).copy()
    # (a) height slices
    hts = np.array([0.0, 300.0])
    rays = R.Rays.grid(xp, yp, inc=inc, hd=-167.9)
    w, h, K, npt, fl = R.raytrace_slices_epochs(cubes, rays, hts, zref)
    assert w.shape == (_FOLD_D, 2, ny, nx) and np.isfinite(w).all() and np.isfinite(h).all()
    single = [cb.raytrace_slices(rays, hts, zref) for cb in cubes]
    for e, (sw, sh, sK, snp, sfl) in enumerate(single):
        assert np.array_equal(w[e], sw, equal_nan=True) and np.array_equal(h[e], sh, equal_nan=True), e
        assert np.array_equal(K, sK) and np.array_equal(npt, snp) and np.array_equal(fl[e], sfl), e
    assert not np.array_equal(w[0], w[1])
    # (b) per-ray heights: a smooth ramp between 0 and 1500 m (ht = None: the level table of the lowest ray, Rays.table_height)
    ramp = 1500.0 * (0.5 * np.arange(ny)[:, None] / (ny - 1) + 0.5 * np.arange(nx)[None, :] / (nx - 1))
    rays_h = R.Rays.grid(xp, yp, inc=inc, hd=-167.9, hts=ramp)
    wp, hp, npp, flp = R.raytrace_epochs(cubes, rays_h, None, zref)
    assert wp.shape == (_FOLD_D, ny, nx) and np.isfinite(wp).all() and np.isfinite(hp).all()
    for e, cb in enumerate(cubes):
        sw, sh, snp, sfl = cb.raytrace(rays_h, None, zref)
        assert np.array_equal(wp[e], sw, equal_nan=True) and np.array_equal(hp[e], sh, equal_nan=True), e
        assert np.array_equal(npp, snp) and flp == sfl, e
    # (c) f64 cubes on exact axes stage a level's footprint in LDS (march_kernel's STAGED path, which stayed apart from the shared loops):
    # the same call with the staging switched off runs the shared slice loop - the same bytes.  The switch is read once per process.
    if dtype is np.float64 and kind == 'regular':
        repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        src, dst = str(tmp_path / 'scene.npz'), str(tmp_path / 'out.npz')
        np.savez(src, ys=ys, xs=xs, zs=cs[0]['zs'], wet=fields[0][0], hydro=fields[0][1], xp=xp, yp=yp, inc=inc, hts=hts, zref=zref)
        env = dict(os.environ, RAIDER_HIP_F64_STAGE='0')
        done = subprocess.run([sys.executable, '-c', _STAGE_OFF_CHILD, repo, src, dst], env=env, timeout=120, capture_output=True, text=True)
        assert done.returncode == 0, done.stderr[-2000:]
        got = np.load(dst)
        sw, sh, sK, snp, sfl = single[0]
        assert got['w'].tobytes() == sw.tobytes() and got['h'].tobytes() == sh.tobytes()
        assert np.array_equal(got['K'], sK) and np.array_equal(got['npt'], snp) and np.array_equal(got['fl'], sfl)
