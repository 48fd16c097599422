"""GPU: weather models interpolated in time on the device (raider_amd/time_interp.py, rdr_cube_blend_azimuth_time).

center_time: combine_weather_files against the reference's own `timeInterp` product (golden g12) and against Cube.blend.
azimuth_time_grid: the one-pass kernel against the staged chain of s1_azimuth_timing (get_azimuth_time_grid ->
get_inverse_weights_for_dates -> combine_cubes) - bitwise on the entry's own time grid, and the time grid itself within one
millisecond tick of the staged one.  Then the date series through tropo_delay_interp_series against tropo_delay date by date."""
import datetime as dt
import logging
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / 'golden'
NZ, NY, NX = 7, 33, 41                     # 9 471 voxels: 36 full workgroups of 256 and one partial
DATES = [dt.datetime(2021, 1, 1, 7), dt.datetime(2021, 1, 1, 6), dt.datetime(2021, 1, 1, 8)]


def _test_orbit(n_per_10s=1):
    """the synthetic orbit of test_gpu_aztime.py::test_weighted_combination_and_time_grid (13 vectors; denser on request)"""
    from raider_amd.orbits import Orbit
    t = np.arange(-60.0, 60.0 + 1e-9, 10.0 / n_per_10s)
    r, w_ = 7.07e6, 2 * np.pi / 5900.0
    lat0, lon0 = np.radians(30.5), np.radians(-100.0)
    pos = np.stack([r * np.cos(lat0 + w_ * t) * np.cos(lon0), r * np.cos(lat0 + w_ * t) * np.sin(lon0), r * np.sin(lat0 + w_ * t)], -1)
    vel = np.stack([-r * w_ * np.sin(lat0 + w_ * t) * np.cos(lon0), -r * w_ * np.sin(lat0 + w_ * t) * np.sin(lon0), r * w_ * np.cos(lat0 + w_ * t)], -1)
    epoch = dt.datetime(2021, 1, 1, 6, 57, 0)
    return Orbit([epoch + dt.timedelta(seconds=float(x)) for x in t], pos, vel, epoch=epoch)


def _rotated(ys, xs, degrees=4.0):
    """(ny, nx) latitudes / longitudes of the grid turned about its centre: not separable into a row and a column vector"""
    X, Y = np.meshgrid(xs - xs.mean(), ys - ys.mean())
    c, s = np.cos(np.radians(degrees)), np.sin(np.radians(degrees))
    return np.ascontiguousarray(ys.mean() + X * s + Y * c), np.ascontiguousarray(xs.mean() + X * c - Y * s)


@pytest.fixture(scope='module')
def scene():
    from raider_amd import Cube
    rng = np.random.default_rng(16)
    ys, xs, zs = np.linspace(30, 31, NY), np.linspace(-118, -117, NX), np.linspace(0, 9000, NZ)
    f = rng.uniform(0.5, 60.0, (3, 2, NZ, NY, NX)).astype(np.float32)
    pw = [Cube(ys, xs, zs, f[i, 0], f[i, 1], order='zyx') for i in range(3)]                                         # three f32 epochs
    tot32 = [Cube(ys, xs, zs, f[(i + 1) % 3, 1], f[i, 0], order='zyx') for i in range(3)]
    tot64 = [Cube(ys, xs, zs, f[(i + 1) % 3, 1].astype(np.float64) / 7, f[i, 0].astype(np.float64) / 3, order='zyx') for i in range(3)]
    lat2, lon2 = _rotated(ys, xs)
    return dict(ys=ys, xs=xs, zs=zs, pw=pw, tot32=tot32, tot64=tot64, lat2=lat2, lon2=lon2, orb=_test_orbit())


def _same(a, b):
    (aw, ah), (bw, bh) = a.read(), b.read()
    return aw.dtype == np.float64 and aw.tobytes() == bw.tobytes() and ah.tobytes() == bh.tobytes()


@pytest.fixture(scope='module')
def fused(scene):
    """the reference run of the fused entry: both sets, three dates, host lat / lon, with its time grid"""
    from raider_amd.s1_azimuth_timing import combine_cubes_azimuth_time
    return combine_cubes_azimuth_time(scene['pw'], scene['tot32'], DATES, scene['lat2'], scene['lon2'], scene['orb'], return_time_grid=True)


def test_fused_equals_staged_chain_bitwise(scene, fused):
    """(a) on the entry's own time grid the staged chain gives the same bytes: nd = 3 and 2; pointwise only, total only, both; f64
    totals beside f32 pointwise cubes; host and device lat2d / lon2d; a window that zeroes one date on part of the grid."""
    import torch
    from raider_amd.s1_azimuth_timing import combine_cubes_azimuth_time, combine_weather_cubes_azimuth_time
    pw, tot32, tot64, lat2, lon2, orb = (scene[k] for k in ('pw', 'tot32', 'tot64', 'lat2', 'lon2', 'orb'))
    fp, ft, grid = fused
    assert grid.shape == (NZ, NY, NX) and grid.dtype == np.float64 and np.isfinite(grid).all()
    assert fp.shape == (NY, NX, NZ) and fp.dtype == np.float64 and fp.projection is None
    assert all(np.array_equal(a, b) for a, b in zip(fp.grid, pw[0].grid))
    sp, st = combine_weather_cubes_azimuth_time(pw, tot32, DATES, grid)
    assert _same(fp, sp) and _same(ft, st)
    assert np.isfinite(fp.read()[0]).all() and not np.array_equal(fp.read()[0], pw[0].read()[0].astype(np.float64))
    # one set at a time: the same cubes, and None for the absent set
    op, none, g2 = combine_cubes_azimuth_time(pw, None, DATES, lat2, lon2, orb, return_time_grid=True)
    assert none is None and _same(op, sp) and np.array_equal(g2, grid)
    none, ot, g2 = combine_cubes_azimuth_time(None, tot32, DATES, lat2, lon2, orb)
    assert none is None and g2 is None and _same(ot, st)
    # f32 pointwise cubes beside f64 totals (what a processed model holds)
    mp, mt, _ = combine_cubes_azimuth_time(pw, tot64, DATES, lat2, lon2, orb)
    _, st64 = combine_weather_cubes_azimuth_time(pw, tot64, DATES, grid)
    assert _same(mp, sp) and _same(mt, st64)
    # nd = 2
    p2, t2, g2 = combine_cubes_azimuth_time(pw[:2], tot32[:2], DATES[:2], lat2, lon2, orb, return_time_grid=True)
    assert np.array_equal(g2, grid)
    sp2, st2 = combine_weather_cubes_azimuth_time(pw[:2], tot32[:2], DATES[:2], g2)
    assert _same(p2, sp2) and _same(t2, st2)
    # device tensors for lat2d / lon2d: the time grid comes back as a device tensor
    dev = torch.device('cuda:0')
    dp, dtot, dg = combine_cubes_azimuth_time(pw, tot32, DATES, torch.from_numpy(lat2).to(dev), torch.from_numpy(lon2).to(dev), orb, return_time_grid=True)
    assert dg.is_cuda and np.array_equal(dg.cpu().numpy(), grid) and _same(dp, sp) and _same(dtot, st)
    # a window between the smallest and the largest distance to the 06:00 model: that date counts on part of the grid only
    d6 = np.abs(grid - (DATES[1] - DATES[0]).total_seconds())
    window_h = float(np.median(d6)) / 3600.0
    inside = d6 <= window_h * 3600.0
    assert 0.2 < inside.mean() < 0.8
    wp, wt, wg = combine_cubes_azimuth_time(pw, tot32, DATES, lat2, lon2, orb, temporal_window_hours=window_h, return_time_grid=True)
    swp, swt = combine_weather_cubes_azimuth_time(pw, tot32, DATES, wg, temporal_window_hours=window_h)
    assert np.array_equal(wg, grid) and _same(wp, swp) and _same(wt, swt) and not _same(wp, sp)
    diff = (wp.read()[0] != fp.read()[0]).transpose(2, 0, 1)            # (y, x, z) -> (z, y, x)
    # (with the inferred window of one model step, 3600 s, 06:00 counts everywhere and 08:00 nowhere: the two runs differ exactly where the
    # narrower window drops 06:00)
    assert (np.abs(grid - 3600.0) > 3600.0).all() and (d6 <= 3600.0).all()
    assert diff[~inside].mean() > 0.99 and not diff[inside].any()


def test_fused_time_grid_against_staged_time_grid(scene, fused):
    """(b) the kernel's time grid against get_azimuth_time_grid on the same mesh: both truncate to milliseconds, so every voxel is
    within one tick, and a tick moves only where device and NumPy trigonometry put a voxel on different sides of a millisecond
    boundary: fewer than 1 % of the voxels (the bound test_gpu_aztime.py applies between the device and the oracle on this orbit)."""
    from raider_amd.s1_azimuth_timing import get_azimuth_time_grid
    zs, lat2, lon2, orb = (scene[k] for k in ('zs', 'lat2', 'lon2', 'orb'))
    grid = fused[2]
    shape = (NZ, NY, NX)
    sec = get_azimuth_time_grid(np.broadcast_to(lon2, shape), np.broadcast_to(lat2, shape), np.broadcast_to(zs[:, None, None], shape), orb, as_datetime64=False)
    ticks_fused = np.rint((grid + (DATES[0] - orb.epoch).total_seconds()) * 1e3).astype(np.int64)                       # ms since the orbit epoch
    ticks_staged = np.rint(sec * 1e3).astype(np.int64)
    apart = np.abs(ticks_fused - ticks_staged)
    print(f'time grid: {int((apart > 0).sum())} of {apart.size} voxels one tick apart, max {int(apart.max())} tick(s)')
    assert np.abs(grid + (DATES[0] - orb.epoch).total_seconds() - sec).max() <= 1.001e-3
    assert (apart > 0).mean() < 0.01
    assert 150.0 < -grid.mean() < 210.0 and np.ptp(grid) > 1.0           # 06:57 + ~0 s against the 07:00 model; seconds across the scene


def test_sentinel1_orbit_fixture(scene):
    """(c) the Sentinel-1 orbit file of the reference's own fixtures, cut to +-600 s, at the scene tests/orbit_anchor.py looks at"""
    from raider_amd import Cube, _lib as L
    from raider_amd.orbits import Orbit
    from raider_amd.s1_azimuth_timing import combine_cubes_azimuth_time, combine_weather_cubes_azimuth_time, get_azimuth_time_grid
    from raider_amd.utilFcns import ecef2lla
    from tests import orbit_anchor as A
    when = dt.datetime(2018, 11, 12, 23, 0, 2) + dt.timedelta(seconds=35)
    orb = Orbit.from_file(str(GOLD / 'orbit_files' / 'S1_orbit_example.EOF'), when, pad=600)
    assert 4 <= orb.time.size <= L.ORBIT_LDS_MAX_SV
    mid = 0.5 * (A.S1_POS[3] + A.S1_POS[4])                               # the sensor near t = 35 s
    lon_s, lat_s, _ = (float(np.ravel(v)[0]) for v in ecef2lla(mid[0:1], mid[1:2], mid[2:3]))
    ny, nx, nz = 9, 11, 4
    ys, xs, zs = lat_s + np.linspace(-0.5, 0.5, ny), lon_s - np.linspace(4.6, 2.4, nx), np.array([-200.0, 0.0, 1500.0, 9000.0])
    rng = np.random.default_rng(3)
    f = rng.uniform(1.0, 50.0, (3, 2, nz, ny, nx)).astype(np.float32)
    pw = [Cube(ys, xs, zs, f[i, 0], f[i, 1], order='zyx') for i in range(3)]
    lat2, lon2 = _rotated(ys, xs, 3.0)
    dates = [dt.datetime(2018, 11, 12, 23), dt.datetime(2018, 11, 12, 22), dt.datetime(2018, 11, 13, 0)]
    fp, ft, grid = combine_cubes_azimuth_time(pw, pw[::-1], dates, lat2, lon2, orb, return_time_grid=True)
    assert np.isfinite(grid).all() and 2.0 < grid.min() and grid.max() < 72.0                # seconds after 23:00:00, inside the eight vectors
    sp, st = combine_weather_cubes_azimuth_time(pw, pw[::-1], dates, grid)
    assert _same(fp, sp) and _same(ft, st)
    shape = (nz, ny, nx)
    sec = get_azimuth_time_grid(np.broadcast_to(lon2, shape), np.broadcast_to(lat2, shape), np.broadcast_to(zs[:, None, None], shape), orb, as_datetime64=False)
    assert np.abs(grid + (dates[0] - orb.epoch).total_seconds() - sec).max() <= 1.001e-3


def test_status_flags_and_routing(scene, fused, monkeypatch):
    """(d) an orbit that does not reach the scene, (e) a window that excludes every date, (f) more state vectors than the kernel's
    LDS tables hold: status flags and host routing only."""
    from raider_amd import _lib as L
    from raider_amd import s1_azimuth_timing as S
    from raider_amd.time_interp import combine_weather_files
    from raider_amd.weather import ProcessedModel
    pw, tot64, lat2, lon2, orb, zs = (scene[k] for k in ('pw', 'tot64', 'lat2', 'lon2', 'orb', 'zs'))
    with pytest.raises(ValueError, match='The Time Grid return nans meaning no orbit was downloaded.'):
        S.combine_cubes_azimuth_time(pw, None, DATES, lat2, lon2 + 90.0, orb)                  # zero Doppler lies far outside the 120 s arc
    with pytest.raises(ValueError, match='within temporal window'):
        S.combine_cubes_azimuth_time(pw, None, DATES, lat2, lon2, orb, temporal_window_hours=0.01)      # 36 s; the nearest model is 180 s away
    with pytest.raises(ValueError, match='Dates provided must be unique'):
        S.combine_cubes_azimuth_time(pw[:2], None, [DATES[0], DATES[0]], lat2, lon2, orb)
    # combine_weather_files: in-memory models on a lon/lat grid (their 2-D coordinates are the mesh of the axes)
    models = [ProcessedModel(pw[i], tot64[i], zs) for i in range(3)]
    calls = []
    for name in ('combine_cubes_azimuth_time', 'get_azimuth_time_grid'):
        monkeypatch.setattr(S, name, (lambda fn, name: lambda *a, **k: calls.append(name) or fn(*a, **k))(getattr(S, name), name))
    when = dt.datetime(2021, 1, 1, 6, 57, 3)
    with pytest.raises(NotImplementedError, match='Azimuth Time is currently only implemented for HRRR'):
        combine_weather_files(models, when, 'GMAO', interp_method='azimuth_time_grid', orbit=orb, times=DATES)
    assert calls == []
    one = combine_weather_files(models, when, 'HRRR', interp_method='azimuth_time_grid', orbit=orb, times=DATES)
    assert calls == ['combine_cubes_azimuth_time']
    dense = _test_orbit(n_per_10s=30)                                                      # 361 state vectors
    assert dense.time.size > L.ORBIT_LDS_MAX_SV
    calls.clear()
    two = combine_weather_files(models, when, 'HRRR', interp_method='azimuth_time_grid', orbit=dense, times=DATES)
    assert calls == ['get_azimuth_time_grid']
    for m in (one, two):
        assert isinstance(m, ProcessedModel) and m.proj == 4326 and m.model_times == DATES and m.interpolation_method == 'azimuth_time_grid'
        assert m.pointwise.dtype == np.float64 and m.total.dtype == np.float64 and m.pointwise.shape == (NY, NX, NZ)
        assert np.isfinite(m['wet']).all() and np.isfinite(m['hydro_total']).all() and m['wet'].shape == (NZ, NY, NX)
    # the same orbit sampled 30 x denser
    # the acquisition times differ by the Hermite error, i.e. by at most one millisecond tick: 1e-3 / 180 s of the weight of the 07:00 model,
    # d(w0) <= w0 (1 - w0) 5.6e-6 <= 1.4e-6, times the spread of the fields (< 60)
    np.testing.assert_allclose(two['wet'], one['wet'], rtol=0, atol=1.4e-6 * 60)


def test_center_time_reproduces_the_reference_product(golden, tmp_path):
    """combine_weather_files on the two GMAO epochs of golden g12 for the product's acquisition time: the reference's own
    `timeInterp` arrays bit for bit - through the returned model and, with write=True, back from the written file."""
    from raider_amd import Cube, h5lite
    from raider_amd.time_interp import combine_weather_files
    from raider_amd.weather import ProcessedModel
    g = golden('g12_gmao_time_interp')
    when = dt.datetime.fromisoformat(str(g['query_time']))
    paths = []
    for tag in ('t12', 't15'):
        t = dt.datetime.strptime(str(g[f'{tag}_datetime']), '%Y_%m_%dT%H_%M_%S')
        m = ProcessedModel(Cube(g['y'], g['x'], g['z'], g[f'{tag}_wet'], g[f'{tag}_hydro'], order='zyx'),
                           Cube(g['y'], g['x'], g['z'], g[f'{tag}_wet_total'], g[f'{tag}_hydro_total'], order='zyx'), g['z'])
        paths.append(tmp_path / f'GMAO_{t:%Y_%m_%d_T%H_%M_%S}_32N_36N_121W_114W.nc')
        m.to_netcdf(paths[-1], time=t, model_name='GMAO')
    out = combine_weather_files(paths, when, 'GMAO', interp_method='center_time', write=True)
    assert out.interpolation_method == 'center_time' and out.model_times == [dt.datetime(2020, 1, 30, 12), dt.datetime(2020, 1, 30, 15)]
    assert out.path == tmp_path / f'GMAO_{when:%Y_%m_%dT%H_%M_%S}_timeInterp_32N_36N_121W_114W.nc' and out.path.exists()
    f = h5lite.File(out.path)
    for v in ('wet', 'hydro', 'wet_total', 'hydro_total'):
        want = g[f'interp_{v}']
        assert out[v].dtype == want.dtype and np.array_equal(out[v], want), v
        assert f[v].read().dtype == want.dtype and np.array_equal(f[v].read(), want), v
    assert int(np.ravel(f.attrs['Date1'])[0]) == 0 and int(np.ravel(f.attrs['Date2'])[0]) == 0
    assert np.array_equal(f['z'].read(), g['z']) and np.array_equal(f['y'].read().astype(np.float64), g['y'])
    # without write nothing is written
    out.path.unlink()
    again = combine_weather_files(paths, when, 'GMAO')
    assert again.path is None and not out.path.exists() and np.array_equal(again['wet'], g['interp_wet'])


def _synthetic_models(times, ny=6, nx=7, nz=5, **kw):
    from raider_amd import Cube
    from raider_amd.synthetic import synthetic_cube
    from raider_amd.weather import ProcessedModel
    out = {}
    for k, t in enumerate(times):
        c = synthetic_cube(ny, nx, nz, seed=40 + k, **kw)
        out[t] = ProcessedModel(Cube(c['ys'], c['xs'], c['zs'], c['wet'], c['hydro'], order='zyx'),
                                Cube(c['ys'], c['xs'], c['zs'], c['wet_total'], c['hydro_total'], order='zyx'), c['zs'])
    return out


def test_center_time_is_cube_blend():
    """both combined cubes of two synthetic 6 x 7 x 5 models are Cube.blend's bytes"""
    from raider_amd.time_interp import combine_weather_files, get_weights_time_interp
    t1, t2, when = dt.datetime(2020, 1, 1, 12), dt.datetime(2020, 1, 1, 18), dt.datetime(2020, 1, 1, 13, 7, 9)
    models = _synthetic_models([t1, t2])
    out = combine_weather_files([models[t1], models[t2]], when, 'ERA5', times=[t1, t2])
    w1, w2 = get_weights_time_interp([t1, t2], when)
    for got, a, b, dtype in ((out.pointwise, models[t1].pointwise, models[t2].pointwise, np.float32), (out.total, models[t1].total, models[t2].total, np.float64)):
        want = a.blend(w1, b, w2)
        assert got.dtype == dtype and got.shape == (6, 7, 5)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got.read(), want.read()))
    with pytest.raises(ValueError, match='pass times='):
        combine_weather_files([models[t1], models[t2]], when, 'ERA5')


def test_series_equals_tropo_delay_date_by_date(caplog):
    """three dates with center_time: a ray-traced 6 x 7 cube at three heights (stacked), a zenith LOS at points; bit for bit
    tropo_delay(t, combine_weather_files(...)) per date; the provenance attributes; one file for a date at a model time."""
    from raider_amd.delay import GridAOI, PointsAOI, tropo_delay
    from raider_amd.losreader import Raytracing, Zenith
    from raider_amd.time_interp import combine_weather_files, tropo_delay_interp, tropo_delay_interp_series
    day = dt.datetime(2020, 1, 1)
    models = _synthetic_models([day + dt.timedelta(hours=h) for h in range(0, 73, 3)], ny=12, nx=14, nz=10)
    dates = [dt.datetime(2020, 1, 1, 13, 52, 44), dt.datetime(2020, 1, 2, 13, 10, 0), dt.datetime(2020, 1, 3, 12, 0, 30)]
    hts = [0.0, 500.0, 1500.0]

    def per_date(t, aoi, los):
        lo = t.replace(hour=12, minute=0, second=0)
        if t == dates[2]:
            return tropo_delay(t, models[lo], aoi, los, hts)
        wm = combine_weather_files([models[lo], models[lo + dt.timedelta(hours=3)]], t, 'ERA5', times=[lo, lo + dt.timedelta(hours=3)])
        return tropo_delay(t, wm, aoi, los, hts)
    grid = GridAOI(np.linspace(-119.0, -116.0, 7), np.linspace(34.5, 32.0, 6))
    ray = Raytracing(inc=35.0, heading=-167.9)
    with caplog.at_level(logging.WARNING):
        res = tropo_delay_interp_series(dates, models, grid, ray, height_levels=hts, interpolate_time='center_time', time_step_hours=3, model_name='ERA5')
    assert 'Time interpolation is not needed as exact time is available' in caplog.text
    assert res.routes == ['stacked'] * 3
    for (ds, none), t in zip(res, dates):
        want, _ = per_date(t, grid, ray)
        assert none is None
        for v in ('wet', 'hydro'):
            got = np.asarray(ds[v][:])
            assert got.shape == (3, 6, 7) and np.isfinite(got).all() and got.tobytes() == np.asarray(want[v][:]).tobytes(), (t, v)
        lo = t.replace(hour=12, minute=0, second=0)
        used = [lo] if t == dates[2] else [lo, lo + dt.timedelta(hours=3)]
        assert ds.attrs['model_name'] == 'ERA5' and ds.attrs['interpolation_method'] == 'center_time'
        assert list(ds.attrs['model_times_used']) == [u.strftime('%Y%m%dT%H:%M:%S') for u in used]
    one, _ = tropo_delay_interp(dates[0], models, grid, ray, height_levels=hts, time_step_hours=3, model_name='ERA5')
    assert np.asarray(one['wet'][:]).tobytes() == np.asarray(res[0][0]['wet'][:]).tobytes() and one.attrs['interpolation_method'] == 'center_time'
    # zenith at points
    rng = np.random.default_rng(8)
    pts = PointsAOI(rng.uniform(32.2, 34.3, 50), rng.uniform(-118.8, -116.2, 50), rng.uniform(0.0, 1400.0, 50), xpts=grid.xpts, ypts=grid.ypts)
    got = tropo_delay_interp_series(dates, models, pts, Zenith(), height_levels=hts, interpolate_time='center_time', time_step_hours=3, model_name='ERA5')
    for (w, h), t in zip(got, dates):
        ww, wh = per_date(t, pts, Zenith())
        assert np.isfinite(w).all() and w.tobytes() == np.asarray(ww).tobytes() and h.tobytes() == np.asarray(wh).tobytes(), t
