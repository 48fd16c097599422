"""GPU: the two raster kernels (rdr_raster_sample, rdr_raster_bounds) and the AOI classes of raider_amd.llreader through the public
entries.  The sampling rules are restated in NumPy here (nearest: floor of the f64 quotient; linear: the bilinear form in
np.longdouble on the f64 cell weights); the bounds are NumPy's own exact reductions; the end-to-end cases are the reference
tests' own numbers (test/test_llreader.py, test/test_intersect.py)."""
import datetime as dt
import xml.etree.ElementTree as ET
from pathlib import Path

import numpy as np
import pytest

from raider_amd import rawraster
from raider_amd.interpolator import interpolate_elevation, interpolateDEM, raster_bounds, raster_sample
from raider_amd.utilFcns import rio_stats

pytestmark = pytest.mark.gpu

FILES = Path(__file__).parent / 'golden' / 'ref_files'
S4 = FILES / 'scenario_4'
H, W = 37, 53
GTS = {'north_up': (-101.7, 0.0131, 0.0, 21.6, 0.0, -0.0173), 'south_up': (-101.7, 0.0131, 0.0, 15.2, 0.0, 0.0173)}
NODATA = -32768.0
SIZES = (1, 63, 64, 65, 100003)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope='module')
def dems():
    rng = np.random.default_rng(17)
    base = rng.integers(-200, 4000, (H, W)).astype(np.int16)
    base[5, 7:19] = int(NODATA); base[H - 1, W - 1] = int(NODATA); base[0, 0] = int(NODATA)          # a no-data run and two corners
    f64 = base + rng.uniform(-0.5, 0.5, (H, W)); f64[base == int(NODATA)] = NODATA
    return {'int16': base, 'float32': f64.astype(np.float32), 'float64': f64}


def _points(gt, rng):
    """About 6000 (x, y): interior, exactly on every cell edge (the four raster edges among them), one ulp either side of edges,
    outside on every side, NaN coordinates."""
    x0, dx, _, y0, _, dy = gt
    xe, ye = x0 + np.arange(W + 1) * dx, y0 + np.arange(H + 1) * dy               # cell edges as the f64 products give them
    lo_x, hi_x, lo_y, hi_y = min(xe[0], xe[-1]), max(xe[0], xe[-1]), min(ye[0], ye[-1]), max(ye[0], ye[-1])
    xs, ys = [rng.uniform(lo_x, hi_x, 4300)], [rng.uniform(lo_y, hi_y, 4300)]
    for e in (xe, np.nextafter(xe, -np.inf), np.nextafter(xe, np.inf)):           # on / beside vertical edges, rows at random and on edges
        xs += [e, e]; ys += [rng.uniform(lo_y, hi_y, e.size), rng.choice(ye, e.size)]
    for e in (ye, np.nextafter(ye, -np.inf), np.nextafter(ye, np.inf)):
        ys += [e, e]; xs += [rng.uniform(lo_x, hi_x, e.size), rng.choice(xe, e.size)]
    cx, cy = np.meshgrid([xe[0], xe[-1]], [ye[0], ye[-1]])                        # the four corners
    xs.append(cx.ravel()); ys.append(cy.ravel())
    m = 300                                                                       # outside, every side and the diagonals
    xs += [rng.uniform(lo_x - 1, lo_x, m), rng.uniform(hi_x, hi_x + 1, m), rng.uniform(lo_x - 1, hi_x + 1, m), rng.uniform(lo_x - 1, hi_x + 1, m)]
    ys += [rng.uniform(lo_y - 1, hi_y + 1, m), rng.uniform(lo_y - 1, hi_y + 1, m), rng.uniform(lo_y - 1, lo_y, m), rng.uniform(hi_y, hi_y + 1, m)]
    xs.append(np.array([np.nan, x0 + dx, np.nan, np.inf, -np.inf, 1e300])); ys.append(np.array([y0 + dy, np.nan, np.nan, y0 + dy, y0 + dy, -1e300]))
    x, y = np.concatenate(xs), np.concatenate(ys)
    order = rng.permutation(x.size)
    return x[order], y[order]


@pytest.fixture(scope='module')
def points():
    rng = np.random.default_rng(5)
    out = {}
    for name, gt in GTS.items():
        x, y = _points(gt, rng)
        assert 6000 <= x.size < 7000
        pick = rng.integers(0, x.size, SIZES[-1])
        out[name] = (x, y, x[pick], y[pick])
    return out


def nearest_ref(dem, gt, x, y, nodata=None):
    """The rule of interpolate_elevation with rasterio's rowcol default: floor of the f64 quotient, NaN outside / for NaN coordinates."""
    with np.errstate(invalid='ignore'):
        col = np.floor((x - gt[0]) / gt[1]); row = np.floor((y - gt[3]) / gt[5])
        ok = (col >= 0) & (col < dem.shape[1]) & (row >= 0) & (row < dem.shape[0])
    out = np.full(x.shape, np.nan)
    out[ok] = dem[row[ok].astype(np.int64), col[ok].astype(np.int64)]
    if nodata is not None:
        out[out == nodata] = np.nan
    return out


def _ascending(dem, gt):
    """(gy, gx, values): pixel-centre axes in ascending order (two roundings per node: the product, the sum) and the raster flipped to match."""
    def axis(o, s, n):
        j = np.arange(n) if s > 0 else n - 1 - np.arange(n)
        return o + (j + 0.5) * s
    v = dem if gt[1] > 0 else dem[:, ::-1]
    v = v if gt[5] > 0 else v[::-1]
    return axis(gt[3], gt[5], dem.shape[0]), axis(gt[0], gt[1], dem.shape[1]), v


def linear_ref(dem, gt, x, y):
    """(value in long double, NaN mask, max |corner|): the cell by scipy's rule on the ascending centres, the two weights as the f64
    quotients scipy forms, then the bilinear form - products of weights, products with the corners, the sum - without f64 rounding."""
    gy, gx, v = _ascending(dem, gt)
    with np.errstate(invalid='ignore'):
        inside = (x >= gx[0]) & (x <= gx[-1]) & (y >= gy[0]) & (y <= gy[-1])
    xi, yi = np.where(inside, x, gx[0]), np.where(inside, y, gy[0])
    kx = np.clip(np.searchsorted(gx, xi, side='right') - 1, 0, gx.size - 2)
    ky = np.clip(np.searchsorted(gy, yi, side='right') - 1, 0, gy.size - 2)
    tx = ((xi - gx[kx]) / (gx[kx + 1] - gx[kx])).astype(np.longdouble)
    ty = ((yi - gy[ky]) / (gy[ky + 1] - gy[ky])).astype(np.longdouble)
    c = [v[ky, kx].astype(np.longdouble), v[ky, kx + 1].astype(np.longdouble), v[ky + 1, kx].astype(np.longdouble), v[ky + 1, kx + 1].astype(np.longdouble)]
    val = c[0] * ((1 - ty) * (1 - tx)) + c[1] * ((1 - ty) * tx) + c[2] * (ty * (1 - tx)) + c[3] * (ty * tx)
    return val, ~inside, np.max(np.abs(np.stack(c)), axis=0).astype(np.float64)


@pytest.mark.parametrize('orient', sorted(GTS))
@pytest.mark.parametrize('dtype', ['int16', 'float32', 'float64'])
def test_nearest_sampling_is_the_numpy_rule_bit_for_bit(dems, points, dtype, orient):
    import torch
    dem, gt = dems[dtype], GTS[orient]
    x, y, bx, by = points[orient]
    want = nearest_ref(dem, gt, x, y)
    assert np.isnan(want).sum() > 1000 and (~np.isnan(want)).sum() > 3500
    got = raster_sample(dem, gt, x, y)
    assert got.dtype == np.float64 and np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_bits(raster_sample(dem, gt, x, y, nodata=NODATA)), _bits(nearest_ref(dem, gt, x, y, NODATA)))
    assert np.isnan(nearest_ref(dem, gt, x, y, NODATA)).sum() > np.isnan(want).sum()
    # 2-D points keep their shape; an empty batch never reaches the library
    assert np.array_equal(_bits(interpolate_elevation((dem, gt), x[:6000].reshape(60, 100), y[:6000].reshape(60, 100))), _bits(want[:6000].reshape(60, 100)))
    assert raster_sample(dem, gt, np.empty((0, 3)), np.empty((0, 3))).shape == (0, 3)
    # device tensors in, a device tensor out; wave and grid-stride tails
    big = nearest_ref(dem, gt, bx, by)
    dx, dy, ddem = torch.from_numpy(bx).cuda(), torch.from_numpy(by).cuda(), torch.from_numpy(dem).cuda()
    for n in SIZES:
        out = raster_sample(ddem, gt, dx[:n], dy[:n])
        assert out.is_cuda and out.dtype == torch.float64 and np.array_equal(_bits(out.cpu().numpy()), _bits(big[:n])), n
        assert np.array_equal(_bits(raster_sample(dem, gt, bx[:n], by[:n])), _bits(big[:n])), n
    out = raster_sample(dem, gt, dx, dy, nodata=NODATA)                         # a host raster with device points is uploaded
    assert out.is_cuda and np.array_equal(_bits(out.cpu().numpy()), _bits(nearest_ref(dem, gt, bx, by, NODATA)))


@pytest.mark.parametrize('orient', sorted(GTS))
@pytest.mark.parametrize('dtype', ['int16', 'float32', 'float64'])
def test_linear_sampling_within_the_rounding_bound(dems, points, dtype, orient):
    """|device - long double| <= 2^-50 max|corner|: given the cell and the two f64 weights, the form rounds 8 times (1 - ty, 1 - tx,
    a weight product, a product with the corner and the running sum per term - fewer where the compiler fuses a product into the
    sum), each by at most half an ulp of a quantity no larger than the largest corner: 8 x 2^-53."""
    import torch
    dem, gt = dems[dtype], GTS[orient]
    x, y, bx, by = points[orient]
    gy, gx, v = _ascending(dem, gt)
    # the hull's own corners (inside), one ulp beyond each side (outside), and every node of a diagonal walk (exact values)
    ex_in, ey_in = np.array([gx[0], gx[-1], gx[0], gx[-1], gx[7]]), np.array([gy[0], gy[-1], gy[-1], gy[0], gy[-1]])
    ex_out = np.array([np.nextafter(gx[0], -np.inf), np.nextafter(gx[-1], np.inf), gx[3], gx[3]])
    ey_out = np.array([gy[2], gy[2], np.nextafter(gy[0], -np.inf), np.nextafter(gy[-1], np.inf)])
    rows = np.arange(W) % H
    x, y = np.concatenate([x, ex_in, ex_out, gx]), np.concatenate([y, ey_in, ey_out, gy[rows]])
    want, nan_mask, cmax = linear_ref(dem, gt, x, y)
    k = x.size - W - 9
    assert not nan_mask[k:k + 5].any() and nan_mask[k + 5:k + 9].all() and not nan_mask[k + 9:].any()      # the last centre is inside
    got = raster_sample(dem, gt, x, y, 'linear')
    assert np.array_equal(np.isnan(got), nan_mask) and 1000 < nan_mask.sum() < x.size - 3000
    err = np.abs(got[~nan_mask].astype(np.longdouble) - want[~nan_mask]).astype(np.float64)
    bound = 2.0 ** -50 * cmax[~nan_mask]
    print(f'linear {dtype} {orient}: max err / bound = {np.max(err / bound):.3f}, max err {err.max():.3e}')
    assert np.all(err <= bound)
    assert np.array_equal(got[k + 9:], v[rows, np.arange(W)].astype(np.float64))                          # on a node: that pixel, exactly
    # device tensors, the wave and grid-stride tails: the same bits as the host-array call
    bwant = raster_sample(dem, gt, bx, by, 'linear')
    dx, dy = torch.from_numpy(bx).cuda(), torch.from_numpy(by).cuda()
    for n in SIZES:
        out = raster_sample(dem, gt, dx[:n], dy[:n], 'linear')
        assert out.is_cuda and np.array_equal(_bits(out.cpu().numpy()), _bits(bwant[:n])), n
    # no-data corners poison their cells
    nd = raster_sample(dem, gt, x, y, 'linear', nodata=NODATA)
    assert np.isnan(nd).sum() > nan_mask.sum() and np.array_equal(_bits(nd[~np.isnan(nd)]), _bits(got[~np.isnan(nd)]))
    with pytest.raises(ValueError, match='two pixels per axis'):
        raster_sample(dem[:1], gt, x[:4], y[:4], 'linear')


def test_interpolate_dem_is_the_reference_route_on_a_descending_list(dems, tmp_path):
    """The reference's 1-D branch interpolates onto the outer product of np.sort(lats)[::-1] and lons, and StationFile.readZ takes the
    diagonal: on a list already sorted by descending latitude that IS each station's own height, and interpolateDEM returns it.
    Both sides sit within 2^-50 max|corner| of the exact form on the same weights (scipy forms the same quotients), so they differ by
    at most 2^-49 max|corner|.  On any other order the diagonal pairs latitudes with the wrong longitudes; interpolateDEM does not."""
    from scipy.interpolate import RegularGridInterpolator
    dem, gt = dems['float64'], GTS['north_up']
    gy, gx, v = _ascending(dem, gt)
    rng = np.random.default_rng(3)
    lats = np.sort(rng.uniform(gy[0], gy[-1], 41))[::-1].copy(); lons = rng.uniform(gx[0], gx[-1], 41)
    rgi = RegularGridInterpolator((gy, gx), v, method='linear', bounds_error=False)
    yy, xx = np.meshgrid(np.sort(lats)[::-1], lons, indexing='ij')
    ref = np.diag(rgi(np.stack([yy, xx], axis=-1)))
    got = interpolateDEM((dem, gt), (lats, lons))
    assert got.shape == (41,) and np.all(np.abs(got - ref) <= 2.0 ** -49 * np.abs(dem).max())
    shuffled = rng.permutation(41)
    assert np.array_equal(interpolateDEM((dem, gt), (lats[shuffled], lons[shuffled])), got[shuffled])
    # StationFile without heights: sampled from demFile, written back to the CSV (llreader.py:231-241)
    import pandas as pd
    from raider_amd.llreader import StationFile
    rawraster.write_envi(dems['int16'], tmp_path / 'dem.envi', geotransform=gt)
    csv = tmp_path / 'stations.csv'
    pd.DataFrame({'ID': [f'S{i}' for i in range(41)], 'Lat': lats[shuffled], 'Lon': lons[shuffled]}).to_csv(csv, index=False)
    aoi = StationFile(csv, demFile=str(tmp_path / 'dem.envi'))
    csv_lats, csv_lons = aoi.readLL()                    # (pandas' default parser may read a coordinate back one ulp off: the file's are the stations')
    assert np.allclose(csv_lats, lats[shuffled], rtol=1e-15, atol=0) and np.allclose(csv_lons, lons[shuffled], rtol=1e-15, atol=0)
    z = aoi.readZ()
    assert np.array_equal(z, raster_sample(dems['int16'], gt, csv_lons, csv_lats, 'linear'))
    back = StationFile(csv).readZ()                      # the heights now come from the file: the CSV text round trip, to an ulp
    assert 'Hgt_m' in pd.read_csv(csv).columns and np.allclose(back, z, rtol=1e-15, atol=0)
    pd.DataFrame({'Lat': [80.0, 81.0], 'Lon': [10.0, 11.0]}).to_csv(csv, index=False)
    with pytest.raises(Exception, match='DEM interpolation failed'):
        StationFile(csv, demFile=str(tmp_path / 'dem.envi')).readZ()
    # a DEM in a projected CRS is refused by name
    rawraster.write_envi(dems['int16'], tmp_path / 'utm.envi', geotransform=(499980.0, 30.0, 0.0, 3700020.0, 0.0, -30.0), proj=32611)
    with pytest.raises(ValueError, match='32611'):
        interpolate_elevation(tmp_path / 'utm.envi', lons, lats)


def _masked(a, nodata):
    a = np.asarray(a, dtype=np.float64)
    return np.where(a == nodata, np.nan, a)


def test_bounds_of_the_reference_rasters_are_gdals():
    lat, lat_prof = rawraster.rio_open(S4 / 'lat.rdr')
    lon, lon_prof = rawraster.rio_open(S4 / 'lon.rdr')
    assert lat_prof['nodata'] == lon_prof['nodata'] == 0.0
    got = raster_bounds(lat, lon, nodata=0.0)
    for (lo, hi, count), data, name in zip(got, (lat, lon), ('lat.rdr', 'lon.rdr')):
        md = {m.get('key'): m.text for m in ET.parse(S4 / (name + '.vrt')).getroot().iter('MDI')}
        assert f'{lo:.14g}' == md['STATISTICS_MINIMUM'] and f'{hi:.14g}' == md['STATISTICS_MAXIMUM']          # to the digits GDAL printed
        valid = data[data != 0.0]
        assert lo == valid.min() and hi == valid.max() and count == valid.size == 45 * 226 - 388
        stats, crs, gt = rio_stats(S4 / name)                                  # utilFcns.py:213-241 on one band
        assert (stats.min, stats.max, stats.count) == (lo, hi, count) and crs == 4326 and gt is None


@pytest.mark.parametrize('n', [1, 63, 64, 65, 20340, 1000003])
def test_bounds_equal_numpy_exactly(n):
    import torch
    rng = np.random.default_rng(n)
    a, b = rng.uniform(-180.0, 180.0, n), rng.uniform(-90.0, 90.0, n)
    if n > 1:
        a[rng.integers(0, n, max(1, n // 50))] = np.nan
        b[: n // 3] = -9999.0; a[n // 2: n // 2 + 40] = -9999.0            # no-data runs
        b[rng.integers(0, n, max(1, n // 70))] = np.nan
    a[-1], b[-1] = 200.0, -100.0                                           # the extreme sits in the last element
    want = tuple((np.nanmin(m), np.nanmax(m), int(np.isfinite(m).sum())) for m in (_masked(a, -9999.0), _masked(b, -9999.0)))
    assert want[0][1] == 200.0 and want[1][0] == -100.0
    got = raster_bounds(a, b, nodata=-9999.0)
    assert got == want
    assert raster_bounds(torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), nodata=-9999.0) == want
    assert raster_bounds(a)[0] == (np.nanmin(a), np.nanmax(a), int(np.isfinite(a).sum())) and np.isnan(raster_bounds(a)[1][0]) and raster_bounds(a)[1][2] == 0
    if n >= 20340:
        # the other element types, and device views that start off a 16-byte boundary (the scalar head of the vector loop)
        ci, di = rng.integers(-30000, 30000, n).astype(np.int16), rng.integers(-30000, 30000, n).astype(np.int16)
        ci[n // 2: n // 2 + 40] = -9999; di[: n // 3] = -9999; ci[-1], di[-1] = 32000, -32000
        for c, d in ((a.astype(np.float32), b.astype(np.float32)), (ci, di)):
            tc, td = torch.from_numpy(c).cuda(), torch.from_numpy(d).cuda()
            for off in (0, 1, 3):
                w = tuple((np.nanmin(m), np.nanmax(m), int(np.isfinite(m).sum())) for m in (_masked(c[off:], -9999.0), _masked(d[off:], -9999.0)))
                assert raster_bounds(tc[off:], td[off:], nodata=-9999.0) == w, (c.dtype, off)
                assert raster_bounds(c[off:], d[off:], nodata=-9999.0) == w, (c.dtype, off)
    if n == 1000003:                                                       # no atomics: the same bytes on every run
        ta, tb = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        from raider_amd import _lib as L
        ctx = L.Context.default(); ctx.adopt_torch_stream(ta)
        outs = [torch.empty(6, dtype=torch.float64, device='cuda') for _ in range(2)]
        for o in outs:
            L.check(ctx.lib.rdr_raster_bounds(ctx.handle, L.ptr(ta), L.ptr(tb), L.RDR_F64, n, 1, -9999.0, L.ptr(o), L.RDR_DEVICE), ctx.handle)
        assert outs[0].cpu().numpy().tobytes() == outs[1].cpu().numpy().tobytes()


def test_raster_aoi_without_a_valid_pixel(tmp_path):
    from raider_amd.llreader import RasterRDR
    for name in ('lat.rdr', 'lon.rdr'):
        rawraster.write_envi(np.zeros((9, 14)), tmp_path / name, nodata=0.0)
    with pytest.raises(ValueError, match='no valid pixel'):
        RasterRDR(str(tmp_path / 'lat.rdr'), str(tmp_path / 'lon.rdr'))


@pytest.fixture(scope='module')
def scene_model():
    from raider_amd.synthetic import synthetic_cube
    c = synthetic_cube(19, 13, 14, seed=4, y0=14.0, y1=23.0, x0=-103.0, x1=-97.0)
    return dict(x=c['xs'], y=c['ys'], z=c['zs'], wet=c['wet'], hydro=c['hydro'], wet_total=c['wet_total'], hydro_total=c['hydro_total'])


def test_raster_aoi_through_tropo_delay(scene_model):
    """RasterRDR on the reference's scenario_4 rasters, taken through calcDelays' order (add_buffer, set_output_xygrid), gives the bytes
    PointsAOI gives on the three arrays; the bounds are test_latlon_reader's."""
    from raider_amd.delay import PointsAOI, tropo_delay
    from raider_amd.llreader import RasterRDR, bounds_from_latlon_rasters
    from raider_amd.losreader import Zenith
    lat_true, lon_true, hgt_true = (rawraster.rio_open(S4 / n)[0] for n in ('lat.rdr', 'lon.rdr', 'warpedDEM.dem'))
    aoi = RasterRDR(str(S4 / 'lat.rdr'), str(S4 / 'lon.rdr'), hgt_file=str(S4 / 'warpedDEM.dem'))
    assert aoi.type() == 'radar_rasters' and aoi.projection() == 4326 and aoi.geotransform() is None
    lats, lons = aoi.readLL()
    assert lats.shape == lons.shape == (45, 226) and np.array_equal(lats, lat_true) and np.array_equal(lons, lon_true) and np.array_equal(aoi.readZ(), hgt_true)
    bounds_true = [15.7637, 21.4936, -101.6384, -98.2418]
    assert all(np.allclose(b, t, rtol=1e-4) for b, t in zip(aoi.bounds(), bounds_true))
    assert list(bounds_from_latlon_rasters(str(S4 / 'lat.rdr') + ';1', str(S4 / 'lon.rdr'))[0]) == aoi.bounds()           # the file;band syntax
    aoi.add_buffer(0.5)
    aoi.set_output_xygrid(4326)
    when = dt.datetime(2020, 1, 3, 23, 0)
    wet, hyd = tropo_delay(when, scene_model, aoi, Zenith())
    wet2, hyd2 = tropo_delay(when, scene_model, PointsAOI(lat_true, lon_true, hgt_true, aoi.xpts, aoi.ypts), Zenith())
    assert wet.shape == (45, 226) and np.isfinite(wet).sum() == 45 * 226 - 388
    assert np.asarray(wet).tobytes() == np.asarray(wet2).tobytes() and np.asarray(hyd).tobytes() == np.asarray(hyd2).tobytes()


def test_raster_aoi_heights_from_a_dem_feed_the_ray_tracer(scene_model, tmp_path):
    import torch
    import raider_amd as R
    from raider_amd.llreader import GeocodedFile, RasterRDR
    rng = np.random.default_rng(8)
    gt = (-102.0, 0.0125, 0.0, 22.0, 0.0, -0.0125)
    dem = rng.integers(-50, 3000, (560, 340)).astype(np.int16)
    rawraster.write_envi(dem, tmp_path / 'dem.envi', geotransform=gt)
    aoi = RasterRDR(str(S4 / 'lat.rdr'), str(S4 / 'lon.rdr'), dem_file=str(tmp_path / 'dem.envi'))
    lats, lons = aoi.readLL()
    z = aoi.readZ()
    assert z.shape == (45, 226) and np.array_equal(_bits(z), _bits(interpolate_elevation(tmp_path / 'dem.envi', lons, lats)))
    assert np.array_equal(_bits(z), _bits(nearest_ref(dem, gt, lons, lats))) and np.isnan(z).sum() == 388           # the no-data pixels lie at (0, 0)
    with pytest.raises(FileNotFoundError, match='download'):
        RasterRDR(str(S4 / 'lat.rdr'), str(S4 / 'lon.rdr')).readZ()
    # the DEM as its own AOI: heights at its own readLL()
    own = GeocodedFile(tmp_path / 'dem.envi', is_dem=True)
    oy, ox = own.readLL()
    assert np.array_equal(_bits(own.readZ()), _bits(nearest_ref(dem, gt, ox, oy))) and own.readZ().shape == dem.shape
    # a gridded scene on the device: heights sampled there go into Rays.grid as they are
    xpts = torch.linspace(-101.5, -98.5, 31, dtype=torch.float64, device='cuda'); ypts = torch.linspace(21.4, 15.9, 23, dtype=torch.float64, device='cuda')
    yy, xx = torch.meshgrid(ypts, xpts, indexing='ij')
    hts = interpolate_elevation((torch.from_numpy(dem).cuda(), gt), xx.contiguous(), yy.contiguous())
    assert hts.is_cuda and hts.shape == (23, 31) and np.array_equal(hts.cpu().numpy(), nearest_ref(dem, gt, xx.cpu().numpy(), yy.cpu().numpy()))
    m = scene_model
    cube = R.Cube(m['y'], m['x'], m['z'], m['wet'], m['hydro'], order='zyx')
    zref = float(m['z'].max() - 1)
    wet, hyd, _, _ = cube.raytrace(R.Rays.grid(xpts, ypts, inc=34.0, hd=-167.0, hts=hts), None, zref, want_nparts=False)
    assert wet.is_cuda and wet.shape == (23, 31)
    wet_h, hyd_h, _, _ = cube.raytrace(R.Rays.grid(xpts.cpu().numpy(), ypts.cpu().numpy(), inc=34.0, hd=-167.0, hts=hts.cpu().numpy()), None, zref)
    assert np.isfinite(wet_h).all() and np.array_equal(wet.cpu().numpy(), wet_h) and np.array_equal(hyd.cpu().numpy(), hyd_h)


def test_station_aoi_in_the_order_of_calcdelays(golden):
    """test/test_intersect.py::test_gnss_intersect through the AOI class: StationFile -> add_buffer(ERA-5's 0.25 deg) at the default
    2000 m cube spacing -> set_output_xygrid(4326) -> tropo_delay; 2.34514 m at TORP, and golden g13's grid and delays."""
    from raider_amd.delay import tropo_delay
    from raider_amd.llreader import StationFile
    from raider_amd.losreader import Zenith
    import pandas as pd
    g = golden('g13_gnss_intersect')
    csv = FILES / 'scenario_6_stations.csv'
    aoi = StationFile(csv, cube_spacing_in_m=2000.0)
    aoi.add_buffer(0.25)
    aoi.set_output_xygrid(4326)
    assert np.array_equal(aoi.xpts, g['x_aoi']) and np.array_equal(aoi.ypts, g['y_aoi'])
    wet, hyd = tropo_delay(dt.datetime(2020, 1, 30, 13, 52, 45), str(FILES / 'ERA-5_2020_01_30_T13_52_45_32N_35N_120W_115W.nc'), aoi, Zenith(),
                           height_levels=None, out_proj=4326, zref=None)
    torp = list(pd.read_csv(csv)['ID']).index('TORP')
    np.testing.assert_almost_equal(wet[torp] + hyd[torp], 2.34514, decimal=4)
    np.testing.assert_allclose(wet, g['wet_aoi'], rtol=0, atol=1e-14); np.testing.assert_allclose(hyd, g['hydro_aoi'], rtol=0, atol=1e-14)


def test_bounding_box_aoi_builds_a_cube(scene_model):
    """BoundingBox -> add_buffer -> set_output_xygrid -> tropo_delay: the cube GridAOI gives on the same axes."""
    from raider_amd.delay import GridAOI, tropo_delay
    from raider_amd.llreader import BoundingBox
    from raider_amd.losreader import Zenith
    aoi = BoundingBox([17.0, 19.0, -101.0, -99.0])
    aoi.add_buffer(0.5)
    aoi.set_output_xygrid(4326)
    when = dt.datetime(2020, 1, 3, 23, 0)
    ds, _ = tropo_delay(when, scene_model, aoi, Zenith(), height_levels=[0.0, 1500.0])
    ds2, _ = tropo_delay(when, scene_model, GridAOI(aoi.xpts, aoi.ypts), Zenith(), height_levels=[0.0, 1500.0])
    assert np.asarray(ds['wet'][:]).shape == (2, aoi.ypts.size, aoi.xpts.size) and np.isfinite(np.asarray(ds['wet'][:])).all()
    assert np.array_equal(np.asarray(ds['wet'][:]), np.asarray(ds2['wet'][:])) and np.array_equal(np.asarray(ds['hydro'][:]), np.asarray(ds2['hydro'][:]))
    # a UTM output grid: the box goes through this package's transformPoints (transform_bbox's 11 x 11 mesh)
    aoi.set_output_xygrid('EPSG:32614')
    assert aoi.xpts[1] - aoi.xpts[0] == 0.5e5 and aoi.ypts[0] - aoi.ypts[1] == 0.5e5 and 1.7e6 < aoi.ypts[-1] < aoi.ypts[0] < 2.3e6
