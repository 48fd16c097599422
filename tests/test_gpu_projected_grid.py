"""GPU: delay cubes on output grids in a projected CRS (UTM, LCC, polar stereographic) through the device routes - rdr_build_cube_grid,
rdr_point_delays_grid, rdr_grid_geodetic + the LLH slice batches - against the reference's per-height loop (delay.py:205-215,256-323)
rebuilt from the public per-height calls (transformPoints + Cube.interp / cube.raytrace(Rays.points(...))), bit for bit."""
import ctypes as C
import datetime as dt
import logging
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import raider_oracle as O

WHEN = dt.datetime(2020, 1, 1)
HRRR = '+proj=lcc +lat_1=38.5 +lat_2=38.5 +lat_0=38.5 +lon_0=262.5 +x_0=0 +y_0=0 +a=6371229 +b=6371229 +units=m +no_defs'
H = dict(lat_1=38.5, lat_2=38.5, lat_0=38.5, lon_0=262.5 - 360.0, a=6371229.0, es=0.0)
AK = '+proj=stere +lat_0=90 +lon_0=225 +lat_ts=60 +a=6371229 +b=6371229'
AKP = dict(lat_0=90.0, lat_ts=60.0, lon_0=225.0, a=6371229.0, es=0.0)
XG = 300000.0 + 20000.0 * np.arange(12)          # UTM 11N over the US south-west (the c1 cube: -121..-113, 30..36)
YG = 3800000.0 - 20000.0 * np.arange(9)


def _utm_grid_outside():
    """XG / YG widened so that some nodes fall outside the lon/lat cube"""
    return np.concatenate([[100000.0], XG, [900000.0]]), np.concatenate([[4100000.0], YG])


def _old_zenith(cube, xg, yg, zpts, pts_crs, model_crs):
    """delay.py:205-215 as the per-height loop ran it: transformPoints per height, then the interpolators"""
    from raider_amd.delay import transformPoints
    xx, yy = np.meshgrid(xg, yg)
    out = [np.zeros((zpts.size, yg.size, xg.size)) for _ in range(2)]
    for k, ht in enumerate(zpts):
        w, h = cube.interp(transformPoints(yy, xx, np.full(yy.shape, ht), pts_crs, model_crs))
        out[0][k] = w; out[1][k] = h
    return out


def _lonlat_cube(dtype, seed=0):
    import raider_amd as R
    c = O.synthetic_cube(50, 50, 40, seed=seed)
    w, h = c['wet_total'], c['hydro_total']
    return R.Cube(c['ys'], c['xs'], c['zs'], w.astype(dtype), h.astype(dtype), order='zyx'), c


def test_zenith_cube_is_the_per_height_loop_bit_for_bit():
    import raider_amd as R
    from raider_amd.delay import _build_cube
    from raider_amd.delayFcns import FieldInterpolator
    xg, yg = _utm_grid_outside()
    for dtype in (np.float64, np.float32):
        tot, c = _lonlat_cube(dtype)
        zpts = np.array([-500.0, 0.0, 800.0, 3000.0, float(c['zs'].max()) + 10.0])     # below and above the z axis: NaN
        # UTM grid -> lon/lat model
        zw, zh = _build_cube(xg, yg, zpts, 4326, 32611, [FieldInterpolator(tot, 0), FieldInterpolator(tot, 1)])
        ow, oh = _old_zenith(tot, xg, yg, zpts, 32611, 4326)
        assert np.array_equal(zw, ow, equal_nan=True) and np.array_equal(zh, oh, equal_nan=True)
        assert np.isnan(zw).any() and np.isfinite(zw).any()
        # UTM grid -> LCC model
        m = O.synthetic_cube(60, 70, 20, seed=6, y0=-9.0e5, y1=1.0e5, x0=-2.2e6, x1=-1.3e6)
        lc = R.Cube(m['ys'], m['xs'], m['zs'], m['wet_total'].astype(dtype), m['hydro_total'].astype(dtype), order='zyx')
        zpl = np.array([-300.0, 100.0, 1500.0])
        zw, zh = _build_cube(xg, yg, zpl, dict(H, proj='lcc'), 32611, [FieldInterpolator(lc, 0), FieldInterpolator(lc, 1)])
        ow, oh = _old_zenith(lc, xg, yg, zpl, 32611, dict(H, proj='lcc'))
        assert np.array_equal(zw, ow, equal_nan=True) and np.array_equal(zh, oh, equal_nan=True) and np.isfinite(zw[1:]).mean() > 0.5
        # LCC grid -> lon/lat model
        cx, cy = O.lcc_forward(33.0, -117.0, **H)
        lx = cx + 40000.0 * (np.arange(15) - 7); ly = cy - 40000.0 * (np.arange(11) - 5)
        zw, zh = _build_cube(lx, ly, zpts, 4326, HRRR, [FieldInterpolator(tot, 0), FieldInterpolator(tot, 1)])
        ow, oh = _old_zenith(tot, lx, ly, zpts, HRRR, 4326)
        assert np.array_equal(zw, ow, equal_nan=True) and np.array_equal(zh, oh, equal_nan=True) and np.isfinite(zw[1]).all()
        # polar-stereographic grid -> a lon/lat model around Alaska
        a = O.synthetic_cube(40, 50, 30, seed=3, y0=55.0, y1=68.0, x0=-165.0, x1=-135.0)
        ac = R.Cube(a['ys'], a['xs'], a['zs'], a['wet_total'].astype(dtype), a['hydro_total'].astype(dtype), order='zyx')
        sx, sy = O.stere_forward(61.0, -150.0, **AKP)
        px = sx + 50000.0 * (np.arange(13) - 6); py = sy + 50000.0 * (np.arange(10) - 5)
        zw, zh = _build_cube(px, py, zpts, 4326, AK, [FieldInterpolator(ac, 0), FieldInterpolator(ac, 1)])
        ow, oh = _old_zenith(ac, px, py, zpts, AK, 4326)
        assert np.array_equal(zw, ow, equal_nan=True) and np.array_equal(zh, oh, equal_nan=True) and np.isfinite(zw[1]).all()


def test_grid_geodetic_is_transformPoints():
    import raider_amd as R
    import torch
    from raider_amd.delay import transformPoints
    xx, yy = np.meshgrid(XG, YG)
    want = transformPoints(yy, xx, 0.0, 32611, 4326)
    lat, lon = R.grid_geodetic(32611, XG, YG, device=None)
    assert np.array_equal(lat, want[..., 0]) and np.array_equal(lon, want[..., 1])
    tl, to = R.grid_geodetic(32611, torch.from_numpy(XG).cuda(), torch.from_numpy(YG).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(tl.cpu().numpy(), lat) and np.array_equal(to.cpu().numpy(), lon)
    cx, cy = O.lcc_forward(33.0, -117.0, **H)
    lx = cx + 40000.0 * np.arange(5); ly = cy - 40000.0 * np.arange(4)
    xx, yy = np.meshgrid(lx, ly)
    want = transformPoints(yy, xx, 0.0, HRRR, 4326)
    lat, lon = R.grid_geodetic(HRRR, lx, ly, device=None)
    assert np.array_equal(lat, want[..., 0]) and np.array_equal(lon, want[..., 1])


def _orbit_los():
    from raider_amd.losreader import Raytracing
    d = Path(__file__).resolve().parent / 'golden' / 'orbit_files'
    los = Raytracing(str(d / 'S1_sv_file.txt'), time=dt.datetime(2018, 11, 12, 23, 0, 2) + dt.timedelta(seconds=35))
    orb = los._orbit
    mid, _ = O.orbit_hermite(orb.time, orb.position, orb.velocity, [35.0])
    lon_s, lat_s, _ = O.ecef2lla(mid[:, 0], mid[:, 1], mid[:, 2])
    return los, float(lat_s[0]), float(lon_s[0])


def _old_ray(cube, xg, yg, zpts, crs, zref, los=None, inc=None, hd=None, orbit=None):
    """delay.py:256-323 slice by slice on the transformPoints nodes: (wet, hydro, [nparts], [flags])"""
    import raider_amd as R
    from raider_amd.delay import transformPoints
    from raider_amd.utilFcns import lla2ecef
    xx, yy = np.meshgrid(xg, yg)
    ll = transformPoints(yy, xx, np.zeros(yy.shape), crs, 4326)
    lat, lon = ll[..., 0].ravel().copy(), ll[..., 1].ravel().copy()
    out = [np.zeros((zpts.size, yg.size, xg.size)) for _ in range(2)]
    nps, fls = [], []
    for k, ht in enumerate(zpts):
        if orbit is not None:
            lv = orbit.look_vectors(np.stack(lla2ecef(lat.reshape(yy.shape), lon.reshape(yy.shape), np.full(yy.shape, ht)), axis=-1))
            rays = R.Rays.points(lat=lat, lon=lon, los=lv)
        else:
            rays = R.Rays.points(lat=lat, lon=lon, los=los, inc=inc, hd=hd)
        w, h, npk, fl = cube.raytrace(rays, float(ht), zref)
        out[0][k] = np.asarray(w).reshape(yg.size, xg.size); out[1][k] = np.asarray(h).reshape(yg.size, xg.size)
        nps.append(npk); fls.append(fl)
    return out[0], out[1], nps, fls, (lat, lon)


def test_ray_cube_is_the_per_slice_loop_bit_for_bit():
    import raider_amd as R
    from raider_amd import _lib as L
    from raider_amd.delay import _build_cube_ray
    from raider_amd.delayFcns import FieldInterpolator
    from raider_amd.losreader import Raytracing
    c = O.synthetic_cube(50, 50, 40, seed=0)
    zref = float(c['zs'].max() - 1)
    zpts = np.array([0.0, 800.0, 2500.0])
    for dtype in (np.float32, np.float64):
        cube = R.Cube(c['ys'], c['xs'], c['zs'], c['wet'].astype(dtype), c['hydro'].astype(dtype), order='zyx')
        ip = [FieldInterpolator(cube, 0), FieldInterpolator(cube, 1)]
        inc = 30.0 + 10.0 * np.random.default_rng(2).random((YG.size, XG.size)); hd = np.full(inc.shape, -167.9)
        from raider_amd.delay import transformPoints
        xx, yy = np.meshgrid(XG, YG)
        ll = transformPoints(yy, xx, 0.0, 32611, 4326)
        lv = np.ascontiguousarray(O.look_vectors_from_inc_hd(inc, hd, ll[..., 0], ll[..., 1], np.zeros(inc.shape)))
        cases = [(Raytracing(inc=36.0, heading=-167.9), dict(inc=np.full(XG.size * YG.size, 36.0), hd=np.full(XG.size * YG.size, -167.9))),
                 (Raytracing(inc=inc, heading=hd), dict(inc=inc.ravel().copy(), hd=hd.ravel().copy())),
                 (Raytracing(look_vectors=lv), dict(los=lv.reshape(-1, 3).copy()))]
        for los, kw in cases:
            w, h = _build_cube_ray(XG, YG, zpts, los, 4326, 32611, ip, MAX_TROPO_HEIGHT=zref)
            ow, oh, onp, ofl, _ = _old_ray(cube, XG, YG, zpts, 32611, zref, **kw)
            assert np.array_equal(w, ow) and np.array_equal(h, oh) and np.isfinite(w).all()
            # the partition of each slice: the same nParts and flags as the slice-by-slice calls
            rays = los.ray_batch_slices(XG, YG, zpts, crs=32611)
            assert rays.struct.origin_mode == L.ORIGIN_LLH
            _, _, K, nparts, flags = cube.raytrace_slices(rays, zpts, zref)
            for k in range(zpts.size):
                assert np.array_equal(nparts[k, :K[k]], onp[k]) and flags[k] == ofl[k]
    # orbit-based lines of sight: targets built on the device from the grid's 2-D lat / lon
    los, lat_s, lon_s = _orbit_los()
    zone = int((lon_s - 3.5 + 180.0) // 6) + 1
    crs = 32600 + zone
    from raider_amd.delay import transformPoints
    cy, cx = transformPoints(lat_s, lon_s - 3.5, 0.0, 4326, crs)[:2]
    xg = cx + np.linspace(-60000.0, 60000.0, 25); yg = cy + np.linspace(10000.0, -10000.0, 15)
    oc = O.synthetic_cube(40, 44, 30, seed=4, y0=lat_s - 2, y1=lat_s + 2, x0=lon_s - 7, x1=lon_s - 0.5)
    cube = R.Cube(oc['ys'], oc['xs'], oc['zs'], oc['wet'], oc['hydro'], order='zyx')
    zr = float(oc['zs'].max() - 1)
    hts = np.array([0.0, 1500.0, 4000.0])
    w, h = _build_cube_ray(xg, yg, hts, los, 4326, crs, [FieldInterpolator(cube, 0), FieldInterpolator(cube, 1)], MAX_TROPO_HEIGHT=zr)
    ow, oh, _, _, _ = _old_ray(cube, xg, yg, hts, crs, zr, orbit=los._orbit)
    assert np.array_equal(w, ow) and np.array_equal(h, oh) and np.isfinite(w).all()


def test_ray_cube_against_the_oracle():
    """64 x 64 UTM block against the oracle's delay.py:256-323 on the transformPoints nodes: <= 1e-9 m, same NaN mask"""
    import raider_amd as R
    from raider_amd.delay import _build_cube_ray, transformPoints
    from raider_amd.delayFcns import FieldInterpolator
    from raider_amd.losreader import Raytracing
    c = O.synthetic_cube(50, 50, 40, seed=1)
    zref = float(c['zs'].max() - 1)
    cube = R.Cube(c['ys'], c['xs'], c['zs'], c['wet'], c['hydro'], order='zyx')
    xg = 200000.0 + 4500.0 * np.arange(64); yg = 3880000.0 - 4000.0 * np.arange(64)
    zpts = np.array([0.0, 1200.0])
    w, h = _build_cube_ray(xg, yg, zpts, Raytracing(inc=38.0, heading=-167.9), 4326, 32611, [FieldInterpolator(cube, 0), FieldInterpolator(cube, 1)],
                           MAX_TROPO_HEIGHT=zref)
    xx, yy = np.meshgrid(xg, yg)
    ll = transformPoints(yy, xx, 0.0, 32611, 4326)
    lat, lon = ll[..., 0], ll[..., 1]
    ip = list(O.getInterpolators(c['xs'], c['ys'], c['zs'], c['wet'], c['hydro']))
    model_zs = ip[0].grid[2]
    ow, oh = np.zeros((2, 64, 64)), np.zeros((2, 64, 64))
    for k, ht in enumerate(zpts):                                     # oracle.build_cube_ray's slice body on the transformed nodes
        hh = np.full(lat.shape, ht)
        xyz = np.stack(O.lla2ecef(lat, lon, hh), axis=-1)
        LOS = O.look_vectors_from_inc_hd(np.full(lat.shape, 38.0), np.full(lat.shape, -167.9), lat, lon, hh)
        rl, lo_, hi_ = O.build_ray(model_zs, ht, xyz, LOS, zref)
        O.integrate_slice(model_zs, rl, lo_, hi_, O.nparts_from_lengths(rl), ip, [ow[k], oh[k]])
    assert np.array_equal(np.isnan(w), np.isnan(ow)) and np.isfinite(w).mean() > 0.9
    ok = ~np.isnan(w)
    assert np.abs(w[ok] - ow[ok]).max() <= 1e-9 and np.abs(h[ok] - oh[ok]).max() <= 1e-9


def _ulp_close(a, b, ulps=2):
    a, b = np.asarray(a), np.asarray(b)
    nan = np.isnan(a)
    assert np.array_equal(nan, np.isnan(b))
    return bool(np.all(np.abs(a[~nan] - b[~nan]) <= ulps * np.spacing(np.abs(b[~nan]))))


def test_point_branch_on_a_utm_grid_is_one_device_route(monkeypatch):
    """PointsAOI with out_proj = EPSG:32611: Zenith, Conventional and Raytracing take the device route (no host cube) and give what the
    old host sequence - per-height transformPoints + gathers, the cube into a Dataset and back, two gathers, los() - gives."""
    import raider_amd as R
    from raider_amd import delay as D
    from raider_amd.delay import PointsAOI, tropo_delay, transformPoints
    from raider_amd.losreader import Conventional, Raytracing, Zenith, inc_hd_to_enu
    c = O.synthetic_cube(50, 50, 40, seed=0)
    wm = dict(x=c['xs'], y=c['ys'], z=c['zs'], wet=c['wet'], hydro=c['hydro'], wet_total=c['wet_total'], hydro_total=c['hydro_total'])
    rng = np.random.default_rng(8)
    n = 600
    la = rng.uniform(32.0, 34.0, n); lo = rng.uniform(-118.5, -116.5, n); hg = rng.uniform(0, 3000, n)
    yx = transformPoints(la, lo, 0 * la, 4326, 32611)
    xu = np.arange(yx[:, 1].min() - 5000, yx[:, 1].max() + 5000, 4000.0); yu = np.arange(yx[:, 0].max() + 5000, yx[:, 0].min() - 5000, -4000.0)
    hl = list(c['zs'][:15])
    zref = float(c['zs'].max() - 1)
    pn = transformPoints(la, lo, hg, 4326, 32611)
    tot = R.Cube(c['ys'], c['xs'], c['zs'], c['wet_total'], c['hydro_total'], order='zyx')
    cub = R.Cube(c['ys'], c['xs'], c['zs'], c['wet'], c['hydro'], order='zyx')
    zp = np.asarray(hl, dtype=np.float64)
    # the old host sequence, explicitly: intermediate cube slice by slice, as a Cube with axes (yu, xu, hl), then the gather
    zw, zh = _old_zenith(tot, xu, yu, zp, 32611, 4326)
    zc = R.Cube(yu, xu, zp, zw, zh, order='zyx')
    sw, sh = zc.interp(pn)
    rw, rh, _, _, _ = _old_ray(cub, xu, yu, zp, 32611, zref, inc=np.full(xu.size * yu.size, 39.0), hd=np.full(xu.size * yu.size, -167.9))
    rc = R.Cube(yu, xu, zp, rw, rh, order='zyx')
    tw, th = rc.interp(pn)

    def no_host_cube(*a, **k):
        raise AssertionError('the host sequence ran')
    monkeypatch.setattr(D, '_get_delays_on_cube', no_host_cube)
    wz, hz = tropo_delay(WHEN, wm, PointsAOI(la, lo, hg, xu, yu), Zenith(), hl, 32611, None)
    assert np.array_equal(wz, sw, equal_nan=True) and np.array_equal(hz, sh, equal_nan=True) and np.isfinite(wz).mean() > 0.9
    inc = rng.uniform(25, 45, n); hd = np.full(n, -167.9)
    wp, hp = tropo_delay(WHEN, wm, PointsAOI(la, lo, hg, xu, yu), Conventional(inc=inc, heading=hd), hl, 32611, None)
    up = inc_hd_to_enu(inc, hd)[..., -1]
    assert _ulp_close(wp, sw / up) and _ulp_close(hp, sh / up)
    wr, hr = tropo_delay(WHEN, wm, PointsAOI(la, lo, hg, xu, yu), Raytracing(inc=39.0, heading=-167.9), hl, 32611, None)
    assert np.array_equal(wr, tw, equal_nan=True) and np.array_equal(hr, th, equal_nan=True) and np.isfinite(wr).mean() > 0.9


def _counts(ctx, fn):
    import torch
    ctx.set_profiling(True)
    fn()
    torch.cuda.synchronize()
    got = [ctx.profile_get(k)[0] for k in range(4)]
    ctx.set_profiling(False)
    return got


def test_one_batch_per_cube():
    """A 20-height UTM cube launches what its lon/lat twin of the same size launches: one prepass / march batch for the ray-traced
    cube, one build (kind 2) for the zenith cube - and no per-height transform / gather (kind 3)."""
    import raider_amd as R
    from raider_amd._lib import Context
    from raider_amd.delay import _build_cube, _build_cube_ray
    from raider_amd.delayFcns import FieldInterpolator
    from raider_amd.losreader import Raytracing
    ctx = Context.default()
    c = O.synthetic_cube(50, 50, 40, seed=0)
    zref = float(c['zs'].max() - 1)
    cube = R.Cube(c['ys'], c['xs'], c['zs'], c['wet'], c['hydro'], order='zyx')
    tot = R.Cube(c['ys'], c['xs'], c['zs'], c['wet_total'], c['hydro_total'], order='zyx')
    zpts = np.linspace(0.0, 6000.0, 20)
    xu = 300000.0 + 5000.0 * np.arange(48); yu = 3800000.0 - 5000.0 * np.arange(40)
    xl = np.linspace(-119.5, -115.5, 48); yl = np.linspace(34.5, 31.5, 40)
    los = Raytracing(inc=38.0, heading=-167.9)
    ip = [FieldInterpolator(cube, 0), FieldInterpolator(cube, 1)]
    it = [FieldInterpolator(tot, 0), FieldInterpolator(tot, 1)]
    utm = _counts(ctx, lambda: _build_cube_ray(xu, yu, zpts, los, 4326, 32611, ip, MAX_TROPO_HEIGHT=zref))
    ll = _counts(ctx, lambda: _build_cube_ray(xl, yl, zpts, los, 4326, 4326, ip, MAX_TROPO_HEIGHT=zref))
    assert utm[:2] == ll[:2] and ll[0] >= 1, (utm, ll)
    utm = _counts(ctx, lambda: _build_cube(xu, yu, zpts, 4326, 32611, it))
    ll = _counts(ctx, lambda: _build_cube(xl, yl, zpts, 4326, 4326, it))
    assert utm[2] == ll[2] == 1 and utm[3] == 0, (utm, ll)


def test_series_on_a_utm_grid_is_stacked(caplog):
    from raider_amd.delay import GridAOI, PointsAOI, tropo_delay, tropo_delay_series, transformPoints
    from raider_amd.losreader import Raytracing
    cs = [O.synthetic_cube(40, 44, 24, seed=10 + e) for e in range(3)]
    files = [dict(x=c['xs'], y=c['ys'], z=c['zs'], wet=c['wet'] * (1 + 0.03 * e), hydro=c['hydro'] * (1 + 0.03 * e), wet_total=c['wet_total'],
                  hydro_total=c['hydro_total']) for e, c in enumerate(cs)]
    dates = [WHEN + dt.timedelta(days=12 * i) for i in range(3)]
    inc = 30.0 + 16.0 * np.arange(XG.size) / XG.size
    los = Raytracing(inc=np.broadcast_to(inc, (YG.size, XG.size)).copy(), heading=-167.9)
    hl = [0.0, 500.0, 2000.0, 4000.0]
    ser = tropo_delay_series(dates, files, GridAOI(XG, YG), los, hl, 32611)
    assert ser.routes == ['stacked'] * 3
    for t, f, got in zip(dates, files, ser):
        want = tropo_delay(t, f, GridAOI(XG, YG), los, hl, 32611)
        assert got[1] is None and want[1] is None
        for k in ('wet', 'hydro'):
            assert np.array_equal(np.asarray(got[0][k]), np.asarray(want[0][k]), equal_nan=True)
        assert repr({k: v for k, v in got[0].attrs.items() if k != 'history'}) == repr({k: v for k, v in want[0].attrs.items() if k != 'history'})
    assert np.isfinite(np.asarray(ser[0][0]['wet'])).all()
    # stations with out_proj = UTM
    rng = np.random.default_rng(3)
    la = rng.uniform(32.2, 33.8, 300); lo = rng.uniform(-118.4, -116.6, 300); hg = rng.uniform(0, 2000, 300)
    yx = transformPoints(la, lo, 0 * la, 4326, 32611)
    xu = np.arange(yx[:, 1].min() - 5000, yx[:, 1].max() + 5000, 5000.0); yu = np.arange(yx[:, 0].max() + 5000, yx[:, 0].min() - 5000, -5000.0)
    los1 = Raytracing(inc=38.0, heading=-167.9)
    ser = tropo_delay_series(dates, files, PointsAOI(la, lo, hg, xu, yu), los1, hl, 32611)
    assert ser.routes == ['stacked'] * 3
    for t, f, got in zip(dates, files, ser):
        w, h = tropo_delay(t, f, PointsAOI(la, lo, hg, xu, yu), los1, hl, 32611)
        assert np.array_equal(got[0], w, equal_nan=True) and np.array_equal(got[1], h, equal_nan=True)


def test_new_entries_refuse_bad_arguments():
    from raider_amd import _lib as L
    from raider_amd._lib import Context, ptr
    import raider_amd as R
    ctx = Context.default()
    lib, h = ctx.lib, ctx.handle
    c = O.synthetic_cube(20, 22, 16, seed=0)
    tot = R.Cube(c['ys'], c['xs'], c['zs'], c['wet_total'], c['hydro_total'], order='zyx')
    tm = np.array([6378137.0, 0.0066943799901413165, 0.0, -117.0, 0.9996, 500000.0, 0.0])
    bad_tm = tm.copy(); bad_tm[4] = 0.0
    x, y, z = XG.copy(), YG.copy(), np.array([0.0, 500.0])
    out = np.empty(x.size * y.size * z.size); o2 = np.empty_like(out)
    lat, lon = np.empty(x.size * y.size), np.empty(x.size * y.size)
    pts = np.zeros(3); w1 = np.empty(1); h1 = np.empty(1)
    cube_out = C.c_void_p()
    G = L.RDR_GRID_TM
    calls = [
        lambda k, p, nx: lib.rdr_grid_geodetic(h, k, ptr(p), p.size, ptr(x), nx, ptr(y), y.size, ptr(lat), ptr(lon), L.RDR_HOST),
        lambda k, p, nx: lib.rdr_build_cube_grid(h, tot.handle, k, ptr(p), p.size, ptr(x), nx, ptr(y), y.size, ptr(z), z.size, ptr(out), ptr(o2), L.RDR_HOST),
        lambda k, p, nx: lib.rdr_build_cube_grid_to_cube(h, tot.handle, k, ptr(p), p.size, ptr(x), nx, ptr(y), y.size, ptr(z), z.size, L.RDR_HOST,
                                                         C.byref(cube_out)),
        lambda k, p, nx: lib.rdr_point_delays_grid(h, tot.handle, k, ptr(p), p.size, ptr(x), nx, ptr(y), y.size, ptr(z), z.size, ptr(pts), None, None, 1,
                                                   0, None, 0.0, ptr(w1), ptr(h1), None),
    ]
    for fn in calls:
        assert fn(G, tm, x.size) == L.RDR_OK
        assert fn(0, tm, x.size) == L.RDR_ERR_INVALID                 # lon/lat is no projected grid
        assert fn(7, tm, x.size) == L.RDR_ERR_INVALID                 # unknown kind
        assert fn(G, bad_tm, x.size) == L.RDR_ERR_INVALID             # k_0 = 0
        assert fn(G, tm[:5].copy(), x.size) == L.RDR_ERR_INVALID      # too few parameters
        assert fn(G, tm, -1) == L.RDR_ERR_INVALID                     # negative count
        assert fn(L.RDR_PROJ_LCC, tm, x.size) == L.RDR_ERR_INVALID    # 7 parameters for a cone
    if cube_out.value:
        lib.rdr_cube_destroy(cube_out)
    assert lib.rdr_grid_geodetic(h, G, ptr(tm), tm.size, None, x.size, ptr(y), y.size, ptr(lat), ptr(lon), L.RDR_HOST) == L.RDR_ERR_INVALID
    assert lib.rdr_build_cube_grid(h, None, G, ptr(tm), tm.size, ptr(x), x.size, ptr(y), y.size, ptr(z), z.size, ptr(out), ptr(o2), L.RDR_HOST) == L.RDR_ERR_INVALID
    assert lib.rdr_synchronize(h) == 0
    # an LLH batch without its grid's axes still cannot become a cube
    rays = R.Rays.points(lat=np.full(6, 33.0), lon=np.linspace(-118, -117, 6), inc=np.full(6, 38.0), hd=np.full(6, -167.9))
    with pytest.raises(Exception, match='GRID batch'):
        tot.raytrace_slices_to_cube(rays, np.array([0.0, 500.0]), float(c['zs'].max() - 1))
