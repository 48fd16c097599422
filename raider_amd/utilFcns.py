"""Geodesy helpers of the delay path (tools/RAiDER/utilFcns.py:55-137).

lla2ecef / ecef2lla run on the GPU (the reference goes through pyproj/PROJ, utilFcns.py:77-88);
the ENU rotations and degree trig are the same few NumPy expressions the reference uses and are kept
on the host because the reference's callers use them on tiny arrays outside the hot loops (inside the
ray kernels the same conversions are fused on-device, csrc/geodesy.h)."""

import numpy as np

from ._lib import Context, check, f64, ptr, RDR_HOST


def projectDelays(delay, inc):
    """utilFcns.py:55-59."""
    if np.any(np.asarray(inc) == 90):
        raise ZeroDivisionError
    return delay / cosd(inc)


def sind(x):
    """utilFcns.py:67-69."""
    return np.sin(np.radians(x))


def cosd(x):
    """utilFcns.py:72-74."""
    return np.cos(np.radians(x))


def lla2ecef(lat, lon, height):
    """utilFcns.py:77-81 - returns the (x, y, z) tuple pyproj's always_xy transform returns."""
    lat, lon, height = np.broadcast_arrays(np.asarray(lat, dtype=np.float64), np.asarray(lon, dtype=np.float64),
                                           np.asarray(height, dtype=np.float64))
    shp = lat.shape
    ctx = Context.default()
    la, lo, hh = f64(lat).ravel(), f64(lon).ravel(), f64(height).ravel()
    xyz = np.empty((la.size, 3))
    check(ctx.lib.rdr_lla2ecef(ctx.handle, ptr(la), ptr(lo), ptr(hh), la.size, ptr(xyz), RDR_HOST), ctx.handle)
    return xyz[:, 0].reshape(shp), xyz[:, 1].reshape(shp), xyz[:, 2].reshape(shp)


def ecef2lla(x, y, z):
    """utilFcns.py:84-88 - returns (lon, lat, height) (always_xy order)."""
    x, y, z = np.broadcast_arrays(np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64), np.asarray(z, dtype=np.float64))
    shp = x.shape
    xyz = np.ascontiguousarray(np.stack([x.ravel(), y.ravel(), z.ravel()], axis=-1))
    ctx = Context.default()
    n = xyz.shape[0]
    lon, lat, h = np.empty(n), np.empty(n), np.empty(n)
    check(ctx.lib.rdr_ecef2lla(ctx.handle, ptr(xyz), n, ptr(lon), ptr(lat), ptr(h), RDR_HOST), ctx.handle)
    return lon.reshape(shp), lat.reshape(shp), h.reshape(shp)


def enu2ecef(east, north, up, lat0, lon0, h0):
    """utilFcns.py:91-121: rotate a local ENU vector at (lat0, lon0) into ECEF; h0 is unused there too."""
    slat, clat, slon, clon = sind(lat0), cosd(lat0), sind(lon0), cosd(lon0)
    t = clat * up - slat * north
    w = slat * up + clat * north
    u = clon * t - slon * east
    v = slon * t + clon * east
    return np.stack((u, v, w), axis=-1)


def ecef2enu(xyz, lat, lon, height):
    """utilFcns.py:124-137."""
    x, y, z = xyz[..., 0], xyz[..., 1], xyz[..., 2]
    slat, clat, slon, clon = sind(lat), cosd(lat), sind(lon), cosd(lon)
    t = clon * x + slon * y
    e = -slon * x + clon * y
    n = -slat * t + clat * z
    u = clat * t + slat * z
    return np.stack((e, n, u), axis=-1)


def utm_params(epsg):
    """Transverse-Mercator parameters of a WGS 84 / UTM zone EPSG code (326zz north, 327zz south), or None."""
    epsg = int(epsg)
    if 32601 <= epsg <= 32660 or 32701 <= epsg <= 32760:
        zone = epsg % 100
        return dict(a=6378137.0, es=0.0066943799901413165, lat_0=0.0, lon_0=6.0 * zone - 183.0, k_0=0.9996, x_0=500000.0,
                    y_0=10000000.0 if epsg >= 32701 else 0.0)
    return None


def cone_abi(params):
    """(kind, parameter array) of a conic CRS as the C ABI takes it (RDR_PROJ_LCC / RDR_PROJ_STERE; rdr_transform_cone)."""
    if params.get('proj', 'lcc') == 'stere':
        lat_ts = params.get('lat_ts')
        return 2, np.array([params['a'], params['es'], params['lat_0'], np.nan if lat_ts is None else lat_ts, params.get('k_0', 1.0), params['lon_0'],
                            params.get('x_0', 0.0), params.get('y_0', 0.0)], dtype=np.float64)
    return 1, np.array([params['a'], params['es'], params['lat_1'], params['lat_2'], params['lat_0'], params['lon_0'], params.get('x_0', 0.0),
                        params.get('y_0', 0.0)], dtype=np.float64)


def tm_abi(params):
    """The parameter array of a transverse-Mercator CRS as the C ABI takes it (rdr_transform_tm, RDR_GRID_TM)."""
    return np.array([params[k] for k in ('a', 'es', 'lat_0', 'lon_0', 'k_0', 'x_0', 'y_0')], dtype=np.float64)


def conic(a_in, b_in, params, inverse=False):
    """Forward: (lat, lon) deg -> (y, x) m; inverse: (y, x) m -> (lat, lon) deg for a conic model CRS, on the GPU (rdr_transform_cone).
    params: dict(proj='lcc', a, es, lat_1, lat_2, lat_0, lon_0, x_0, y_0) (HRRR, models/hrrr.py:248-259) or
    dict(proj='stere', a, es, lat_0, lat_ts, k_0, lon_0, x_0, y_0) (HRRR-AK, models/hrrr.py:22-25; polar aspect only)."""
    from . import _lib as L
    from ._lib import Context, check, f64, ptr
    a_in, b_in = np.broadcast_arrays(np.asarray(a_in, dtype=np.float64), np.asarray(b_in, dtype=np.float64))
    shp = a_in.shape
    ua, ub = f64(a_in).ravel(), f64(b_in).ravel()
    oa, ob = np.empty(ua.size), np.empty(ua.size)
    kind, p = cone_abi(params)
    ctx = Context.default()
    check(ctx.lib.rdr_transform_cone(ctx.handle, kind, ptr(p), p.size, int(bool(inverse)), ptr(ua), ptr(ub), ua.size, ptr(oa), ptr(ob), L.RDR_HOST),
          ctx.handle)
    return oa.reshape(shp), ob.reshape(shp)


def transverse_mercator(a_in, b_in, params, inverse=False):
    """Forward: (lat, lon) deg -> (y, x) m; inverse: (y, x) m -> (lat, lon) deg, on the GPU (rdr_transform_tm: Krueger series to n^6,
    the formulation of PROJ's etmerc / utm).  params: dict(a, es, lat_0, lon_0, k_0, x_0, y_0)."""
    import ctypes as C
    from . import _lib as L
    from ._lib import Context, check, f64, ptr
    a_in, b_in = np.broadcast_arrays(np.asarray(a_in, dtype=np.float64), np.asarray(b_in, dtype=np.float64))
    shp = a_in.shape
    ua, ub = f64(a_in).ravel(), f64(b_in).ravel()
    oa, ob = np.empty(ua.size), np.empty(ua.size)
    p = tm_abi(params)
    ctx = Context.default()
    check(ctx.lib.rdr_transform_tm(ctx.handle, ptr(p), p.size, int(bool(inverse)), ptr(ua), ptr(ub), ua.size, ptr(oa), ptr(ob), L.RDR_HOST), ctx.handle)
    return oa.reshape(shp), ob.reshape(shp)


def rio_open(path, userNDV=None, band=None):
    """utilFcns.py:164-202 (rasterio when installed, else GeoTIFFs and flat-binary rasters with a .vrt / ENVI .hdr side-car)."""
    from .rawraster import rio_open as _rio_open
    return _rio_open(path, userNDV=userNDV, band=band)


def _raster_dtype(array):
    """utilFcns.py:257-304: what a delay raster is written as - float -> float32, complex -> complex64, anything else -> uint8."""
    return np.complex64 if 'complex' in str(array.dtype) else (np.float32 if 'float' in str(array.dtype) else np.uint8)


def writeArrayToRaster(array, path, noDataValue=0.0, fmt='ENVI', proj=None, gt=None):
    """utilFcns.py:257-304: a 2-D array as a GDAL-readable raster (float -> float32, complex -> complex64, anything else -> uint8).
    rasterio writes it when installed; without it the ENVI format is written natively (flat binary + .hdr), other formats raise
    (writeDelays writes GTiff without rasterio through raider_amd.tifflite; this function's contract is left as it was)."""
    from pathlib import Path
    array = np.asarray(array)
    if array.ndim != 2:
        raise RuntimeError(f'writeArrayToRaster: cannot write an array of shape {np.shape(array)} to a raster image')
    dtype = _raster_dtype(array)
    path = Path(path)
    if fmt == 'nc':
        fmt = 'GTiff'; path = path.with_suffix('.tif')
    try:
        import rasterio
    except ImportError:
        rasterio = None
    if rasterio is not None:
        trans = None
        if gt is not None:
            try:
                trans = rasterio.Affine.from_gdal(*gt)
            except TypeError:
                trans = gt
        with rasterio.open(path, mode='w', count=1, width=array.shape[1], height=array.shape[0], dtype=dtype, crs=proj, nodata=noDataValue, driver=fmt,
                           transform=trans) as dst:
            dst.write(array.astype(dtype), 1)
        return
    if str(fmt).upper() != 'ENVI':
        raise ImportError(f'writing {fmt} rasters needs rasterio, which is not installed (ENVI is written without it)')
    from .rawraster import write_envi
    write_envi(array.astype(dtype), path, nodata=noDataValue, geotransform=gt, proj=proj)


def _gpu_visible():
    try:
        import torch
        return bool(torch.cuda.is_available())
    except ImportError:
        return False


def _write_delay_raster(array, path, ndv, fmt, proj, gt):
    """One delay raster of writeDelays: writeArrayToRaster, except that GTiff - the reference's default raster_format - is written by
    raider_amd.tifflite (deflate strips; the element type by writeArrayToRaster's rule, complex refused by name) when rasterio is not installed.
    With a GPU visible the strips are differenced (predictor 2) and deflated there in one call; without one, zlib on the host as
    before.  The decoded pixels and every tag but Predictor and the strip byte counts are the same on both routes."""
    import importlib.util
    if str(fmt).upper() == 'GTIFF' and importlib.util.find_spec('rasterio') is None:
        from .tifflite import write as write_tiff
        array = np.asarray(array)
        if array.ndim != 2:
            raise RuntimeError(f'writeArrayToRaster: cannot write an array of shape {np.shape(array)} to a raster image')
        dtype = _raster_dtype(array)
        on_device = dict(encoder='device', predictor=2) if dtype != np.complex64 and array.size and _gpu_visible() else {}
        write_tiff(path, array.astype(dtype), transform=gt, crs=proj, nodata=ndv, compress='deflate', **on_device)     # (complex64: refused by name there)
        return
    writeArrayToRaster(array, path, noDataValue=ndv, fmt=fmt, proj=proj, gt=gt)


def writeDelays(aoi, wetDelay, hydroDelay, wet_path, hydro_path=None, outformat=None, ndv=0.0):
    """utilFcns.py:431-464: station AOIs -> the station CSV with wetDelay / hydroDelay / totalDelay columns; raster AOIs -> two rasters."""
    from pathlib import Path
    import pandas as pd
    wetDelay[np.isnan(wetDelay)] = ndv                  # (in place, as the reference does)
    hydroDelay[np.isnan(hydroDelay)] = ndv
    t = aoi.type() if callable(getattr(aoi, 'type', None)) else getattr(aoi, 'type', None)
    if t == 'station_file':
        df = pd.read_csv(aoi._filename).drop_duplicates(subset=['Lat', 'Lon'])
        df['wetDelay'] = wetDelay
        df['hydroDelay'] = hydroDelay
        df['totalDelay'] = wetDelay + hydroDelay
        df.to_csv(str(wet_path), index=False)
        return
    if hydro_path is None:
        raise ValueError('Hydro delay file path must be specified if the AOI is not a station file')
    proj = aoi.projection() if hasattr(aoi, 'projection') else None
    gt = aoi.geotransform() if hasattr(aoi, 'geotransform') else None
    _write_delay_raster(wetDelay, Path(wet_path), ndv, outformat or 'ENVI', proj, gt)
    _write_delay_raster(hydroDelay, Path(hydro_path), ndv, outformat or 'ENVI', proj, gt)


# ---- what llreader.py takes from utilFcns: bounding boxes and raster metadata (utilFcns.py:140-161, 213-254, 586-630) -----------
def get_file_and_band(filestr):
    """utilFcns.py:244-254: `file;band` -> (Path, band), band 1 without a suffix."""
    from pathlib import Path
    parts = filestr.split(';')
    if len(parts) == 1:
        return Path(filestr.strip()), 1
    elif len(parts) == 2:
        return Path(parts[0].strip()), int(parts[1].strip())
    else:
        raise ValueError(f'Cannot interpret {filestr} as valid filename')


def clip_bbox(bbox, spacing):
    """utilFcns.py:623-630: clip box to multiple of spacing (outwards)."""
    return [
        np.floor(bbox[0] / spacing) * spacing,
        np.ceil(bbox[1] / spacing) * spacing,
        np.floor(bbox[2] / spacing) * spacing,
        np.ceil(bbox[3] / spacing) * spacing,
    ]


def transform_bbox(snwe_in, dest_crs=4326, src_crs=4326, buffer=100.0):
    """utilFcns.py:586-620: SNWE box in `src_crs` -> SNWE box in `dest_crs`: the identity for equal CRSs, else the extremes of an
    11 x 11 mesh over the box grown by `buffer` metres (1e-5 degrees per metre for a lon / lat source), taken through transformPoints -
    so for the CRSs that function has built in (anything else needs pyproj there, as in the reference)."""
    from .delay import _is_4326, _same_crs, transformPoints
    if _is_4326(src_crs):
        buffer = buffer / 1.0e5
    if _same_crs(dest_crs, src_crs):
        return snwe_in
    xs = np.linspace(snwe_in[2] - buffer, snwe_in[3] + buffer, num=11)
    ys = np.linspace(snwe_in[0] - buffer, snwe_in[1] + buffer, num=11)
    X, Y = np.meshgrid(xs, ys)
    out = transformPoints(Y, X, np.zeros_like(X), src_crs, dest_crs)
    yy, xx = out[..., 0], out[..., 1]
    return [np.nanmin(yy), np.nanmax(yy), np.nanmin(xx), np.nanmax(xx)]


def rio_profile(path):
    """utilFcns.py:140-151: the profile of a raster (`<path>.vrt` preferred)."""
    from pathlib import Path
    from .rawraster import open_raster
    path = Path(path)
    if path.name.startswith('S1-GUNW'):
        raise NotImplementedError('GUNW sub-datasets are read by raider_amd.gunw, not as rasters')
    vrt = Path(f'{path}.vrt')
    with open_raster(vrt if vrt.exists() else path) as src:
        return src.profile


def _gdal_transform(profile):
    gt = profile.get('transform')
    if gt is None:
        raise ValueError('the raster carries no geotransform')
    return tuple(gt.to_gdal()) if hasattr(gt, 'to_gdal') else tuple(gt)


def rio_extents(profile):
    """utilFcns.py:154-161: SNWE of a profile - the coordinates of the first and the last pixel's upper-left corner, as the reference
    computes them."""
    gt = _gdal_transform(profile)
    xSize = profile['width']
    ySize = profile['height']
    W, E = gt[0], gt[0] + (xSize - 1) * gt[1] + (ySize - 1) * gt[2]
    N, S = gt[3], gt[3] + (xSize - 1) * gt[4] + (ySize - 1) * gt[5]
    return S, N, W, E


def rio_stats(path, band=1):
    """utilFcns.py:213-241: (stats, CRS, geotransform) of one band.  stats has .min / .max / .count over the valid pixels (neither NaN
    nor the band's no-data value), reduced on the device (rdr_raster_bounds) - what the reference's callers read of GDAL's
    statistics; the CRS is 4326 when the file names none (the assumption bounds_from_latlon_rasters makes); the geotransform is None
    for a raster without one."""
    from collections import namedtuple
    from pathlib import Path
    from .interpolator import raster_bounds
    from .rawraster import rio_open as _rio_open
    data, profile = _rio_open(Path(path), band=band)
    (lo, hi, count), _ = raster_bounds(data, None, nodata=profile.get('nodata'))
    gt = profile.get('transform')
    if gt is not None:
        gt = _gdal_transform(profile)
    crs = profile.get('crs')
    return namedtuple('Statistics', 'min max count')(lo, hi, count), (4326 if crs is None else crs), gt
