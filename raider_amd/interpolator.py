"""scipy-style callable over the GPU `interpolate` (counterpart of tools/RAiDER/interpolator.py:19-69).

Edge rule = the native extension's, not scipy's: with a fill value, a query lying ON the last node of an axis is
filled (interpolate.h:23-38,58-65); without one, queries outside the grid are linearly extrapolated."""
import numpy as np

from .interpolate import interpolate


class RegularGridInterpolator:
    def __init__(self, grid, values, fill_value=None, assume_sorted=False, max_threads=8):
        self.grid, self.values = grid, values
        self.fill_value, self.assume_sorted, self.max_threads = fill_value, assume_sorted, max_threads

    def __call__(self, points):
        """points: an (..., ndim) array, or a tuple of equally shaped coordinate arrays (one per axis)."""
        if isinstance(points, tuple):
            shapes = {np.shape(p) for p in points}
            assert len(shapes) == 1, 'All dimensions must contain the same number of points!'
            points = np.stack(points, axis=-1)
        points = np.asarray(points)
        lead = points.shape[:-1]
        flat = interpolate(self.grid, self.values, points.reshape(-1, points.shape[-1]), fill_value=self.fill_value,
                           assume_sorted=self.assume_sorted, max_threads=self.max_threads)
        return flat.reshape(lead)


# ---- DEM sampling (interpolator.py:133-184) and raster bounds, on the device ----------------------------------------------------
_RASTER_DTYPES = {'int16': 2, 'float32': 0, 'float64': 1}          # RDR_I16 / RDR_F32 / RDR_F64


def _is_dev(a):
    return hasattr(a, 'data_ptr')


def _points_device(*pts):
    """The GPU the query points live on, or None for host points."""
    return next((t.device for t in pts if _is_dev(t) and t.is_cuda), None)


def _raster_native(a):
    """The raster as the kernels read it: C-contiguous int16 / float32 / float64 in native byte order (anything else as float64)."""
    if _is_dev(a):
        name = str(a.dtype).replace('torch.', '')
        if name not in _RASTER_DTYPES:
            import torch
            a = a.to(torch.float64); name = 'float64'
        return a.contiguous(), _RASTER_DTYPES[name]
    a = np.asarray(a)
    name = a.dtype.name if a.dtype.name in _RASTER_DTYPES else 'float64'
    return np.ascontiguousarray(a, dtype=np.dtype(name)), _RASTER_DTYPES[name]


def _tiff_on_device(dem, device):
    """(tensor, profile) of band 1 of a GeoTIFF decoded on `device`, or None when the file is not one / rasterio is there to read it."""
    import importlib.util
    from pathlib import Path
    from .tifflite import is_tiff, read
    if importlib.util.find_spec('rasterio') is not None or Path(f'{dem}.vrt').exists() or not is_tiff(dem):
        return None
    return read(dem, band=1, device=device)


def _dem_arg(dem, device=None):
    """(array, geotransform) of `dem`: a path (read through rawraster / tifflite: band 1; the file must say where it lies, in lon / lat)
    or an (array, geotransform) pair.  device: where the query points live - a GeoTIFF is then decoded there and never exists on the host."""
    if isinstance(dem, (tuple, list)) and len(dem) == 2 and not isinstance(dem[0], (str, bytes)):
        return dem[0], tuple(float(v) for v in dem[1])
    from .rawraster import rio_open
    from .delay import _is_4326
    got = _tiff_on_device(dem, device) if device is not None else None
    data, prof = got if got is not None else rio_open(dem, band=1)
    gt = prof.get('transform')
    if gt is None:
        raise ValueError(f'{dem}: the raster carries no geotransform (a GeoTIFF tie point, an ENVI `map info` or a VRT <GeoTransform>), so it cannot serve as a DEM')
    gt = tuple(gt.to_gdal()) if hasattr(gt, 'to_gdal') else tuple(float(v) for v in gt)
    crs = prof.get('crs')
    if crs is not None and not _is_4326(crs):
        raise ValueError(f'{dem}: the DEM is in CRS {crs}; only lon / lat (EPSG:4326) DEMs are sampled here - warp it with GDAL first')
    return data, gt


def raster_sample(raster, geotransform, x, y, method='nearest', nodata=None):
    """rdr_raster_sample: the north-up `raster` (2-D; int16 / float32 / float64 are read as they are) with GDAL `geotransform` at the
    points (x, y), any shape.  method 'nearest': the pixel whose cell holds the point; 'linear': bilinear on pixel centres; NaN
    outside.  nodata: a raster value equal to it comes out as NaN.  NumPy points give a NumPy array; float64 torch tensors on the
    GPU give a tensor there (the raster is uploaded when it is not a device tensor already) and nothing touches the host."""
    from . import _lib as L
    meth = {'nearest': L.RASTER_NEAREST, 'linear': L.RASTER_LINEAR}.get(method)
    if meth is None:
        raise ValueError(f"method must be 'nearest' or 'linear', not {method!r}")
    gt = np.array([float(v) for v in geotransform], dtype=np.float64)
    if gt.size != 6:
        raise ValueError('a geotransform has six numbers (GDAL order)')
    if len(raster.shape) != 2:
        raise ValueError(f'a raster is 2-D, not {tuple(raster.shape)}')
    ctx = L.Context.default()
    h, w = (int(v) for v in raster.shape)
    nd = (0, 0.0) if nodata is None else (1, float(nodata))
    if _is_dev(x) or _is_dev(y) or _is_dev(raster):
        import torch
        dev = next((t.device for t in (x, y, raster) if _is_dev(t) and t.is_cuda), None)
        if dev is None:
            raise TypeError('tensors must live on the GPU (NumPy arrays are staged by the library)')
        r, code = _raster_native(raster if _is_dev(raster) else torch.from_numpy(_raster_native(raster)[0]))
        r = r.to(dev)
        xt = torch.as_tensor(x, dtype=torch.float64, device=dev).contiguous()
        yt = torch.as_tensor(y, dtype=torch.float64, device=dev).contiguous()
        if xt.shape != yt.shape:
            raise ValueError(f'x and y differ in shape: {tuple(xt.shape)} and {tuple(yt.shape)}')
        out = torch.empty(xt.shape, dtype=torch.float64, device=dev)
        if xt.numel():
            ctx.adopt_torch_stream(xt)
            L.check(ctx.lib.rdr_raster_sample(ctx.handle, L.ptr(r), code, h, w, L.ptr(gt), L.ptr(xt), L.ptr(yt), xt.numel(), meth, nd[0], nd[1], L.ptr(out),
                                              L.RDR_DEVICE), ctx.handle)
        return out
    r, code = _raster_native(raster)
    xa, ya = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if xa.shape != ya.shape:
        raise ValueError(f'x and y differ in shape: {xa.shape} and {ya.shape}')
    xf, yf = L.f64(xa).ravel(), L.f64(ya).ravel()
    out = np.empty(xf.size)
    if xf.size:
        L.check(ctx.lib.rdr_raster_sample(ctx.handle, L.ptr(r), code, h, w, L.ptr(gt), L.ptr(xf), L.ptr(yf), xf.size, meth, nd[0], nd[1], L.ptr(out), L.RDR_HOST),
                ctx.handle)
    return out.reshape(xa.shape)


def raster_bounds(a, b=None, nodata=None):
    """rdr_raster_bounds: ((min, max, valid count) of a, the same of b) in one pass over both - NaN and `nodata` elements left out,
    min / max NaN when nothing is left - as plain floats / ints (the six numbers are read back).  a, b: equal-sized arrays of one
    dtype, NumPy or torch tensors on the GPU."""
    from . import _lib as L
    ctx = L.Context.default()
    nd = (0, 0.0) if nodata is None else (1, float(nodata))
    ra, code = _raster_native(a)
    rb = None
    if b is not None:
        rb, code_b = _raster_native(b)
        if code_b != code or tuple(rb.shape) != tuple(ra.shape):
            raise ValueError('the two rasters differ in shape or element type')
    n = int(np.prod(tuple(ra.shape)))
    if n == 0:
        return (np.nan, np.nan, 0), (np.nan, np.nan, 0)
    if _is_dev(ra):
        import torch
        out = torch.empty(6, dtype=torch.float64, device=ra.device)
        ctx.adopt_torch_stream(ra)
        L.check(ctx.lib.rdr_raster_bounds(ctx.handle, L.ptr(ra), L.ptr(rb), code, n, nd[0], nd[1], L.ptr(out), L.RDR_DEVICE), ctx.handle)
        out = out.cpu().numpy()
    else:
        out = np.empty(6)
        L.check(ctx.lib.rdr_raster_bounds(ctx.handle, L.ptr(ra), L.ptr(rb), code, n, nd[0], nd[1], L.ptr(out), L.RDR_HOST), ctx.handle)
    return (float(out[0]), float(out[1]), int(out[2])), (float(out[3]), float(out[4]), int(out[5]))


def interpolate_elevation(dem, x, y):
    """interpolator.py:154-184: the DEM pixel each (x = lon, y = lat) falls in, any shape, NaN outside the raster.  dem: a path or an
    (array, geotransform) pair.  No-data heights come through unchanged, as in the reference."""
    raster, gt = _dem_arg(dem, _points_device(x, y))
    return raster_sample(raster, gt, x, y, 'nearest')


def interpolateDEM(dem, outLL, method='nearest'):
    """interpolator.py:133-151: DEM heights at outLL = (lats, lons).  2-D arrays are sampled nearest (interpolate_elevation); 1-D ones
    bilinearly on the pixel centres AT EACH (lat, lon) PAIR.  `method` is accepted and unused, as in the reference, whose two branches
    fix the rule themselves.  The reference's 1-D branch interpolates onto the outer product of np.sort(lats)[::-1] and lons, of which
    StationFile.readZ takes the diagonal - the stations' own heights only for a file listed by descending latitude; this returns what
    that comment means, for any order."""
    lats, lons = outLL
    if len(lats.shape) == 2:
        return interpolate_elevation(dem, lons, lats)
    raster, gt = _dem_arg(dem, _points_device(lons, lats))
    return raster_sample(raster, gt, lons, lats, 'linear')
