"""Weather-model cube producer on the GPU.

Mirrors the processing chain of the reference's WeatherModel.load (tools/RAiDER/models/weatherModel.py:235-262):
``_find_e`` -> ``_uniform_in_z`` -> ``_checkForNans`` -> wet / hydrostatic refractivity -> ``_adjust_grid`` -> ``_getZTD``,
but lands the result directly in the two device cubes the delay kernels read (no NetCDF round trip through
``write()`` / ``getInterpolators``).  Two front ends make the producer's (zs, p, t, hum) columns from a raw state, on the device:
``ecmwf_model_levels`` (ECMWF hybrid model levels) and ``pressure_level_state`` (pressure levels, or levels that carry their own
height field: geopotential -> geometric height, the pressure broadcast, the re-ordering and the flips).  Raw ERA-5 / HRES NetCDF
files of both kinds are read here; the other providers' download formats stay with the caller (they are I/O, not part of this path).
"""
import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import Context, check
from .engine import Cube, _is_dev, f64, ptr

# models/weatherModel.py:25-31 (the TOTAL_LEVELS_IN_MODEL heights every model is resampled to)
_ZMIN = -100.0
_ZREF = 80000.0
MODEL_LEVEL_HEIGHTS = np.array(
    [-100, 0, 50, 100, 150, 200, 250, 300, 350, 400, 450, 500, 600, 700, 800, 900, 1000, 1100, 1200, 1300, 1400, 1500, 1600,
     1700, 1800, 1900, 2000, 2100, 2200, 2300, 2400, 2500, 2600, 2700, 2800, 2900, 3000, 3100, 3200, 3300, 3400, 3500, 3600,
     3700, 3800, 3900, 4000, 4200, 4400, 4600, 4800, 5000, 5250, 5500, 5750, 6000, 6250, 6500, 6750, 7000, 7500, 8000, 8500,
     9000, 9500, 10000, 11000, 12000, 13000, 14000, 15000, 16000, 17000, 18000, 19000, 20000, 25000, 30000, 35000, 40000],
    dtype=np.float64)


class ProcessedModel:
    """What WeatherModel.load leaves behind, GPU-resident: ``pointwise`` = (wet, hydro) refractivity cube (f32),
    ``total`` = (wet_total, hydro_total) zenith-delay cube (f64); ``t``, ``p``, ``e`` (f32, (y, x, z)) when asked for."""

    def __init__(self, pointwise, total, zs, t=None, p=None, e=None, proj=4326):
        self.pointwise, self.total, self.zs = pointwise, total, zs
        self.t, self.p, self.e = t, p, e
        self.proj = proj            # CRS of the x/y axes, as tropo_delay reads it off the model file (delay.py:66-73)

    # mapping view with the processed file's variable names (weatherModel.py:685-693; fields in file order (z, y, x)), so an
    # instance can be handed to tropo_delay / getInterpolators wherever they take a weather-model file
    _KEYS = ('x', 'y', 'z', 'wet', 'hydro', 'wet_total', 'hydro_total', 'proj')

    def keys(self):
        return self._KEYS

    def __contains__(self, k):
        return k in self._KEYS

    def __getitem__(self, k):
        if k == 'x': return self.pointwise.grid[1]
        if k == 'y': return self.pointwise.grid[0]
        if k == 'z': return self.pointwise.grid[2]
        if k == 'proj': return self.proj
        if k in ('wet', 'hydro'): return np.ascontiguousarray(self.pointwise.read()[k == 'hydro'].transpose(2, 0, 1))
        if k in ('wet_total', 'hydro_total'): return np.ascontiguousarray(self.total.read()[k == 'hydro_total'].transpose(2, 0, 1))
        raise KeyError(k)

    def to_netcdf(self, path, time=None, model_name='ERA-5', format='NETCDF4', attrs=None):
        """The processed weather-model file of WeatherModel.write (weatherModel.py:659-724): dims z, y, x; variables wet, hydro
        (f32), wet_total, hydro_total (f64) - and t, p, e (f32) when the model was produced with return_state=True - with the
        reference's units / standard_name / grid_mapping attributes, 2-D latitude / longitude, the `proj` grid-mapping variable
        carrying `crs_wkt`, and the global attributes (plus `attrs`, e.g. Date1 / Date2 of a combined model, cli/raider.py:820-821; the
        pointwise fields of a model combined with per-voxel weights are float64 and are written as such).  format='NETCDF4' (what the reference writes through xarray): HDF5 via
        raider_amd.h5write, coordinate variables typed as in the reference's files (x, y f32; z f64); 'NETCDF3_64BIT': classic
        format through scipy.  Either is read back by tropo_delay / getInterpolators, xarray and netCDF4."""
        import datetime as dt
        from .delay import _builtin_crs
        kind = _builtin_crs(self.proj)
        if kind is None or kind[0] not in ('geodetic', 'cone'):
            raise NotImplementedError(f'ProcessedModel.to_netcdf: the model CRS {self.proj!r} has no CF description here (EPSG:4326, Lambert '
                                      'conformal conic and polar stereographic models do)')
        ys, xs, zs = self.pointwise.grid
        wet, hyd = self.pointwise.read(); wt, ht = self.total.read()                     # (y, x, z)
        zyx = lambda v: np.ascontiguousarray(np.asarray(v).transpose(2, 0, 1))
        ptyp = 'f8' if np.dtype(self.pointwise.dtype) == np.float64 else 'f4'
        fields = [('wet', wet, ptyp, 'dimentionless', 'wet_refractivity'), ('hydro', hyd, ptyp, 'dimentionless', 'hydrostatic_refractivity'),
                  ('wet_total', wt, 'f8', 'm', 'total_wet_refractivity'), ('hydro_total', ht, 'f8', 'm', 'total_hydrostatic_refractivity')]
        if self.t is not None:
            fields = [('t', self.t, 'f4', 'K', 'temperature'), ('p', self.p, 'f4', 'Pa', 'pressure'), ('e', self.e, 'f4', 'Pa', 'humidity')] + fields
        gattrs = dict(Conventions='CF-1.6', title='Weather model data and delay calculations', model_name=str(model_name))
        if time is not None:
            gattrs['datetime'] = time.strftime('%Y_%m_%dT%H_%M_%S')
        gattrs['date_created'] = dt.datetime.now().strftime('%Y_%m_%dT%H_%M_%S')
        gattrs.update(attrs or {})
        # EPSG:4326 as current PROJ releases spell it in WKT2:2019 (what pyproj's CRS.to_cf() puts into the reference's files)
        crs_wkt = ('GEOGCRS["WGS 84",ENSEMBLE["World Geodetic System 1984 ensemble",MEMBER["World Geodetic System 1984 (Transit)"],'
                   'MEMBER["World Geodetic System 1984 (G730)"],MEMBER["World Geodetic System 1984 (G873)"],MEMBER["World Geodetic System 1984 (G1150)"],'
                   'MEMBER["World Geodetic System 1984 (G1674)"],MEMBER["World Geodetic System 1984 (G1762)"],MEMBER["World Geodetic System 1984 (G2139)"],'
                   'ELLIPSOID["WGS 84",6378137,298.257223563,LENGTHUNIT["metre",1]],ENSEMBLEACCURACY[2.0]],PRIMEM["Greenwich",0,'
                   'ANGLEUNIT["degree",0.0174532925199433]],CS[ellipsoidal,2],AXIS["geodetic latitude (Lat)",north,ORDER[1],'
                   'ANGLEUNIT["degree",0.0174532925199433]],AXIS["geodetic longitude (Lon)",east,ORDER[2],ANGLEUNIT["degree",0.0174532925199433]],'
                   'USAGE[SCOPE["Horizontal component of 3D system."],AREA["World."],BBOX[-90,-180,90,180]],ID["EPSG",4326]]')
        proj_attrs = dict(crs_wkt=crs_wkt, semi_major_axis=6378137.0, semi_minor_axis=6356752.314245179, inverse_flattening=298.257223563,
                          reference_ellipsoid_name='WGS 84', longitude_of_prime_meridian=0.0, prime_meridian_name='Greenwich',
                          geographic_crs_name='WGS 84', horizontal_datum_name='World Geodetic System 1984 ensemble', grid_mapping_name='latitude_longitude',
                          grid_mapping='proj')      # (weatherModel.py:716-717 tags every data variable, `proj` included)
        lon2, lat2 = np.meshgrid(xs, ys)
        if kind[0] == 'cone':                                   # projected model (HRRR, HRRR-AK): what CRS.to_cf() writes; geodetic 2-D coordinates
            from .crs import cf_from_crs
            from .utilFcns import conic
            _, cf = cf_from_crs(kind[1])
            proj_attrs = dict(cf, grid_mapping='proj')
            lat2, lon2 = conic(lat2, lon2, kind[1], inverse=True)          # (y, x) metres -> (lat, lon) degrees, on the device
        if format.upper().startswith('NETCDF4'):
            from .h5write import write_netcdf4
            # (the reference's files carry x / y as float32 because its ERA-5 axes ARE float32; axes that are not exactly
            # representable in float32 stay float64 - a rounded axis would move every interpolation weight)
            f32_exact = lambda a: bool(np.array_equal(np.asarray(a, np.float32).astype(np.float64), np.asarray(a, np.float64)))
            hdt = np.float32 if (f32_exact(xs) and f32_exact(ys)) else np.float64
            variables = {'z': (('z',), np.asarray(zs, np.float64), {}), 'y': (('y',), np.asarray(ys, hdt), {}), 'x': (('x',), np.asarray(xs, hdt), {}),
                         'latitude': (('y', 'x'), lat2.astype(hdt), {}), 'longitude': (('y', 'x'), lon2.astype(hdt), {})}
            for name, arr, typ, units, std in fields:
                variables[name] = (('z', 'y', 'x'), zyx(arr).astype(typ), dict(units=units, standard_name=std, grid_mapping='proj', coordinates='latitude longitude'))
            variables['proj'] = ((), np.array(0, dtype=np.int64), proj_attrs)
            write_netcdf4(path, dict(z=np.size(zs), y=np.size(ys), x=np.size(xs)), variables, gattrs)
            return str(path)
        from scipy.io import netcdf_file
        with netcdf_file(str(path), 'w', version=2) as f:
            for k, v in gattrs.items():
                setattr(f, k, v)
            for d, v in (('z', zs), ('y', ys), ('x', xs)):
                f.createDimension(d, int(np.size(v)))
                f.createVariable(d, 'f8', (d,))[:] = np.asarray(v, dtype=np.float64)
            f.createVariable('latitude', 'f8', ('y', 'x'))[:] = lat2
            f.createVariable('longitude', 'f8', ('y', 'x'))[:] = lon2
            for name, arr, typ, units, std in fields:
                v = f.createVariable(name, typ, ('z', 'y', 'x'))
                v[:] = zyx(arr)
                v.units = units; v.standard_name = std; v.grid_mapping = 'proj'
            pj = f.createVariable('proj', 'i4', ())
            pj.data[()] = 0
            for k, v in proj_attrs.items():
                setattr(pj, k, np.float64(v) if isinstance(v, float) else v)      # (a bare Python float is narrowed to float32 by scipy's writer)
        return str(path)

    def interpolators(self, kind='pointwise'):
        """getInterpolators(wm_file, kind) (delayFcns.py:23-58) without the file"""
        from .delayFcns import interpolators_from_cube
        return interpolators_from_cube(self.pointwise if kind == 'pointwise' else self.total)


def cubes_from_model_levels(xs, ys, zs, p, t, hum, humidity_type='q', new_z=None, k1=0.776, k2=0.233, k3=3.75e3,
                            zmin=_ZMIN, return_state=False, ctx=None):
    """zs, p, t, hum: (ny, nx, nlev) model-level heights (m, ascending in the last axis), pressure (Pa), temperature (K)
    and specific ('q') or relative ('rh', %) humidity; xs, ys: the cube's ascending 1-D axes; new_z: output levels
    (default: the reference's fixed 145-level table is model specific; here the caller passes it, or gets
    MODEL_LEVEL_HEIGHTS clipped below the column tops like _uniform_in_z does with _zlevels)."""
    if humidity_type not in ('q', 'rh'):
        raise RuntimeError('Not a valid humidity type')        # weatherModel.py:340-341
    ctx = ctx or Context.default()
    xs, ys = f64(xs), f64(ys)
    dev = _is_dev(zs)
    if dev:
        import torch
        arrs = [a.to(torch.float64).contiguous() for a in (zs, p, t, hum)]
        ctx.adopt_torch_stream(arrs[0])
        shape = tuple(arrs[0].shape)
    else:
        arrs = [f64(a) for a in (zs, p, t, hum)]
        shape = arrs[0].shape
    if len(shape) != 3 or shape[:2] != (ys.size, xs.size) or any(tuple(a.shape) != tuple(shape) for a in arrs):
        raise ValueError(f'model-level arrays must all be (ny, nx, nlev) = ({ys.size}, {xs.size}, nlev); got {shape}')
    if new_z is None:
        new_z = MODEL_LEVEL_HEIGHTS
    new_z = f64(new_z)
    nzo = new_z.size + (1 if zmin < new_z[0] else 0)
    state = [None, None, None]
    if return_state:
        if dev:
            import torch
            state = [torch.empty(shape[:2] + (nzo,), dtype=torch.float32, device=arrs[0].device) for _ in range(3)]
        else:
            state = [np.empty(shape[:2] + (nzo,), np.float32) for _ in range(3)]
    hp, ht = C.c_void_p(), C.c_void_p()
    check(ctx.lib.rdr_cubes_from_model_levels(
        ctx.handle, ptr(ys), ys.size, ptr(xs), xs.size, ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), ptr(arrs[3]),
        0 if humidity_type == 'q' else 1, shape[2], ptr(new_z), new_z.size, float(k1), float(k2), float(k3), float(zmin),
        L.RDR_DEVICE if dev else L.RDR_HOST, C.byref(hp), C.byref(ht),
        ptr(state[0]) if return_state else None, ptr(state[1]) if return_state else None, ptr(state[2]) if return_state else None),
        ctx.handle)
    pw, tot = Cube._from_handle(ctx, hp), Cube._from_handle(ctx, ht)
    return ProcessedModel(pw, tot, pw.grid[2].copy(), *state)


# ------------------------------------------------------------------------------------------------
# ECMWF hybrid model levels (ERA-5 / HRES raw files) -> the producer's inputs
# ------------------------------------------------------------------------------------------------
def ecmwf_l137():
    """ECMWF's L137 hybrid coefficients and the 145 heights ECMWF models are resampled to (models/ecmwf.py:42-46 with the
    tables of models/model_levels.py, shipped as data): dict(a[138], b[138], level_heights[145] descending)."""
    from pathlib import Path
    d = np.load(Path(__file__).resolve().parent / 'data' / 'ecmwf_l137.npz')
    return {k: d[k] for k in d.files}


def read_ecmwf_model_level_file(path, ll_bounds=None):
    """Raw ERA-5 / HRES model-level file as the CDS / MARS write it (NetCDF-3, packed int16 `z, t, q, lnsp` on
    (time, level, latitude, longitude)) -> dict(lats, lons, z, lnsp (ny, nx), t, q (nlev, ny, nx)), float32, latitude and
    longitude ascending, longitudes in [-180, 180), cut to ll_bounds = (S, N, W, E).  Mirrors ECMWF._makeDataCubes and the
    flips of _load_model_level (models/ecmwf.py:305-337, 58-79); host-side I/O (scipy), no GPU work."""
    from scipy.io import netcdf_file
    with netcdf_file(str(path), 'r', mmap=False) as f:
        def decode(name):                     # CF scale/offset decoding in float32, as xarray does for int16 data
            v = f.variables[name]
            raw = np.array(v.data)
            out = raw.astype(np.float32)
            out *= np.float32(getattr(v, 'scale_factor', 1.0))
            out += np.float32(getattr(v, 'add_offset', 0.0))
            fill = getattr(v, '_FillValue', None)
            if fill is not None:
                out[raw == fill] = np.nan
            return np.squeeze(out)
        z, t, q, lnsp = decode('z'), decode('t'), decode('q'), decode('lnsp')
        lats = np.array(f.variables['latitude'].data, dtype=np.float32)
        lons = np.array(f.variables['longitude'].data, dtype=np.float32)
    lons = ((lons + 180) % 360) - 180
    z, lnsp = z[0], lnsp[0]                   # the two surface fields are stored on level 1
    if ll_bounds is not None:
        S, N, W, E = ll_bounds
        my, mx = (S <= lats) & (N >= lats), (W <= lons) & (E >= lons)
        lats, lons = lats[my], lons[mx]
        z, lnsp, t, q = z[my][:, mx], lnsp[my][:, mx], t[:, my][:, :, mx], q[:, my][:, :, mx]
    if z.size == 0:
        raise RuntimeError('There is no data in z, you may have a problem with your mask')           # ecmwf.py:334-335
    if lats.size > 1 and lats[0] > lats[1]:
        z, lnsp, t, q, lats = z[::-1], lnsp[::-1], t[:, ::-1], q[:, ::-1], lats[::-1]
    if lons.size > 1 and lons[0] > lons[1]:
        z, lnsp, t, q, lons = z[..., ::-1], lnsp[..., ::-1], t[..., ::-1], q[..., ::-1], lons[::-1]
    c = np.ascontiguousarray
    return dict(lats=c(lats), lons=c(lons), z=c(z), lnsp=c(lnsp), t=c(t), q=c(q))


def ecmwf_model_levels(z_surf, lnsp, t, q, lats, a=None, b=None, R_d=287.06, ctx=None):
    """utilFcns.calcgeoh + geo_to_ht + the re-ordering of ecmwf.py:92-110 on the GPU (rdr_ecmwf_model_levels): surface
    geopotential and log surface pressure (ny, nx), temperature and specific humidity (nlev, ny, nx) with level 1 = model top,
    latitudes (ny,) -> (p, zs), both (ny, nx, nlev) float64 with the bottom level first (the producer's layout).  NumPy in ->
    NumPy out; torch tensors on the GPU in -> tensors out."""
    ctx = ctx or Context.default()
    if a is None or b is None:
        tab = ecmwf_l137()
        a, b = tab['a'], tab['b']
    a, b = f64(a), f64(b)
    dev = _is_dev(t)
    lats = np.ascontiguousarray(lats.cpu().numpy() if _is_dev(lats) else lats, dtype=np.float32)
    if dev:
        import torch
        zt, lt, tt, qt = (v.to(torch.float32).contiguous() for v in (z_surf, lnsp, t, q))
        ctx.adopt_torch_stream(tt)
        nlev, ny, nx = (int(v) for v in tt.shape)
        p = torch.empty((ny, nx, nlev), dtype=torch.float64, device=tt.device); zs = torch.empty_like(p)
    else:
        zt, lt, tt, qt = (np.ascontiguousarray(v, dtype=np.float32) for v in (z_surf, lnsp, t, q))
        nlev, ny, nx = tt.shape
        p = np.empty((ny, nx, nlev)); zs = np.empty_like(p)
    if tuple(qt.shape) != (nlev, ny, nx) or tuple(zt.shape) != (ny, nx) or tuple(lt.shape) != (ny, nx) or lats.size != ny:
        raise ValueError('ecmwf_model_levels: t, q must be (nlev, ny, nx); z_surf, lnsp (ny, nx); lats (ny,)')
    if a.size != nlev + 1 or b.size != nlev + 1:
        raise ValueError(f'I have here a model with {nlev} levels, but parameters a and b have lengths {a.size} and {b.size} '
                         'respectively. Of course, these three numbers should be equal.')                   # utilFcns.py:813-817
    check(ctx.lib.rdr_ecmwf_model_levels(ctx.handle, ptr(zt), ptr(lt), ptr(tt), ptr(qt), ptr(lats), ptr(a), ptr(b), nlev, ny, nx, float(R_d),
                                         ptr(p), ptr(zs), L.RDR_DEVICE if dev else L.RDR_HOST), ctx.handle)
    return p, zs


def load_ecmwf_model_levels(path, ll_bounds=None, new_z=None, return_state=False, ctx=None):
    """WeatherModel.load for a raw ERA-5 / HRES model-level file (weatherModel.py:235-262 with ECMWF._load_model_level): file ->
    hybrid-level pressures and geometric heights -> e -> uniform z levels -> NaN fill -> refractivities -> padded bottom level ->
    ZTDs, everything after the file read on the GPU.  Returns the ProcessedModel that tropo_delay / getInterpolators take."""
    ctx = ctx or Context.default()
    raw = read_ecmwf_model_level_file(path, ll_bounds)
    tab = ecmwf_l137()
    p, zs = ecmwf_model_levels(raw['z'], raw['lnsp'], raw['t'], raw['q'], raw['lats'], tab['a'], tab['b'], ctx=ctx)
    up = lambda v: np.ascontiguousarray(np.flip(v.transpose(1, 2, 0), axis=2), dtype=np.float64)          # ecmwf.py:98-106
    if new_z is None:
        new_z = np.flipud(tab['level_heights'])                                                            # ecmwf.py:44
    return cubes_from_model_levels(raw['lons'].astype(np.float64), raw['lats'].astype(np.float64), zs, p, up(raw['t']), up(raw['q']), 'q',
                                   new_z=new_z, return_state=return_state, ctx=ctx)


# ------------------------------------------------------------------------------------------------
# Pressure levels, or levels with their own height field -> the producer's inputs
# ------------------------------------------------------------------------------------------------
def ecmwf_pressure_level_heights():
    """The heights ECMWF pressure-level states are resampled to (models/ecmwf.py:38-40: LEVELS_25_HEIGHTS of
    models/model_levels.py, shipped as data: one number per line), descending as the reference's table is."""
    from pathlib import Path
    return np.loadtxt(Path(__file__).resolve().parent / 'data' / 'ecmwf_pl_heights.txt', dtype=np.float64)


def _check_level_state(height, p, t, hum, lats, height_kind):
    """Shapes of a (nlev, ny, nx) state, before anything touches the device: (nlev, ny, nx), p_ndim, lat_ndim."""
    if height_kind not in (0, 1, 2):
        raise ValueError(f'height_kind must be 0 (geopotential), 1 (geopotential height) or 2 (geometric height); got {height_kind!r}')
    shape = tuple(int(v) for v in height.shape)
    if len(shape) != 3 or 0 in shape:
        raise ValueError(f'the height field must be (nlev, ny, nx); got {shape}')
    nlev, ny, nx = shape
    if tuple(t.shape) != shape or tuple(hum.shape) != shape:
        raise ValueError(f'temperature and humidity must have the shape of the height field {shape}; got {tuple(t.shape)} and {tuple(hum.shape)}')
    if tuple(p.shape) not in ((nlev,), shape):
        raise ValueError(f'pressure must be the level list ({nlev},) or a field {shape}; got {tuple(p.shape)}')
    if tuple(lats.shape) not in ((ny,), (ny, nx)):
        raise ValueError(f'latitudes must be ({ny},) or ({ny}, {nx}); got {tuple(lats.shape)}')
    return shape, len(p.shape), len(lats.shape)


def pressure_level_state(height, p, t, hum, lats, height_kind=0, top_first=True, rows_descending=False, cols_descending=False,
                         device_out=False, ctx=None):
    """What the reference holds after ECMWF._load_pressure_level (models/ecmwf.py:252-303), on the GPU (rdr_pressure_level_state):
    height, t, hum (nlev, ny, nx) in file layout; height_kind 0 = geopotential (m2 s-2, / g0 as :284), 1 = geopotential height (m) -
    both through WeatherModel._get_heights / utilFcns.geo_to_ht - 2 = geometric height (m); p the level list (nlev,) in Pa (:292)
    or a field; lats (ny,) or (ny, nx) in the file's order; top_first: the first level is the top; rows_descending /
    cols_descending: latitudes / longitudes run downwards in the file -> (zs, p, t, hum), each (ny, nx, nlev) float64, levels
    surface -> top, rows and columns ascending: the producer's layout.  NumPy in -> NumPy out (tensors on the GPU with
    device_out=True); torch tensors on the GPU in -> tensors out."""
    dev = _is_dev(height)
    as_np = lambda v: v.cpu().numpy() if _is_dev(v) else np.asarray(v)
    if not dev:
        height, p, t, hum, lats = (as_np(v) for v in (height, p, t, hum, lats))
    (nlev, ny, nx), p_ndim, lat_ndim = _check_level_state(height, p, t, hum, lats, height_kind)
    ctx = ctx or Context.default()
    if dev or device_out:
        import torch
    if dev:
        if not height.is_cuda:
            raise TypeError(f'pressure_level_state takes NumPy arrays or tensors on the GPU (got a tensor on {height.device})')
        arrs = [(v if _is_dev(v) else torch.as_tensor(np.asarray(v))).to(device=height.device, dtype=torch.float64).contiguous()
                for v in (height, p, t, hum, lats)]
        device = height.device
    else:
        arrs = [f64(v) for v in (height, p, t, hum, lats)]
        if device_out:
            from .engine import torch_device_or_none
            device = torch_device_or_none()
            if device is None:
                raise RuntimeError('device_out=True needs torch with a GPU for the output tensors')
    if dev or device_out:
        outs = [torch.empty((ny, nx, nlev), dtype=torch.float64, device=device) for _ in range(4)]
        ctx.adopt_torch_stream(outs[0])
    else:
        outs = [np.empty((ny, nx, nlev)) for _ in range(4)]
    check(ctx.lib.rdr_pressure_level_state(
        ctx.handle, ptr(arrs[0]), int(height_kind), ptr(arrs[1]), p_ndim, ptr(arrs[2]), ptr(arrs[3]), ptr(arrs[4]), lat_ndim, nlev, ny, nx,
        int(bool(top_first)), int(bool(rows_descending)), int(bool(cols_descending)), *(ptr(o) for o in outs),
        L.RDR_DEVICE if dev else L.RDR_HOST, L.RDR_DEVICE if (dev or device_out) else L.RDR_HOST), ctx.handle)
    return tuple(outs)


def cubes_from_pressure_levels(xs, ys, height, p, t, hum, lats, height_kind=0, humidity_type='q', new_z=None, proj=4326, top_first=True,
                               rows_descending=False, cols_descending=False, k1=0.776, k2=0.233, k3=3.75e3, zmin=_ZMIN, return_state=False,
                               ctx=None):
    """WeatherModel.load (weatherModel.py:235-262) for a state on pressure levels or with its own height field: pressure_level_state
    -> cubes_from_model_levels, the columns staying on the device in between.  xs, ys: the cube's ascending axes (degrees, or metres
    of the projected CRS `proj`, which the ProcessedModel carries to tropo_delay); the other arguments as in pressure_level_state
    and cubes_from_model_levels.  With return_state=True the model also holds the loaded columns, `levels` = (zs, p, t, hum)."""
    if humidity_type not in ('q', 'rh'):
        raise RuntimeError('Not a valid humidity type')        # weatherModel.py:340-341
    xs, ys = f64(xs), f64(ys)
    dev = _is_dev(height)
    if not dev:
        height, p, t, hum, lats = (v.cpu().numpy() if _is_dev(v) else np.asarray(v) for v in (height, p, t, hum, lats))
    shape, _, _ = _check_level_state(height, p, t, hum, lats, height_kind)
    if shape[1:] != (ys.size, xs.size):
        raise ValueError(f'the state must be (nlev, ny, nx) = (nlev, {ys.size}, {xs.size}); got {shape}')
    ctx = ctx or Context.default()
    levels = pressure_level_state(height, p, t, hum, lats, height_kind, top_first, rows_descending, cols_descending, device_out=True, ctx=ctx)
    m = cubes_from_model_levels(xs, ys, *levels, humidity_type, new_z=new_z, k1=k1, k2=k2, k3=k3, zmin=zmin, return_state=return_state, ctx=ctx)
    m.proj = proj
    if return_state:
        host = (lambda v: v) if dev else (lambda v: v.cpu().numpy())         # NumPy in -> NumPy out
        m.t, m.p, m.e = host(m.t), host(m.p), host(m.e)
        m.levels = tuple(host(v) for v in levels)
    return m


def read_ecmwf_pressure_level_file(path, ll_bounds=None):
    """Raw ERA-5 / HRES pressure-level file as the CDS / MARS write it (NetCDF-3, packed int16 `z, t, q` on (time, level, latitude,
    longitude)) -> dict(z, t, q (nlev, ny, nx), level (nlev,) in Pa, lats (ny,), lons (nx,)) in the FILE's order, float64, with
    longitudes above 180 wrapped and everything cut to ll_bounds = (S, N, W, E); top_first, rows_descending, cols_descending: the
    order flags pressure_level_state takes; ys, xs: the ascending axes of the cube.  Mirrors what ECMWF._load_pressure_level reads
    (models/ecmwf.py:252-279: the values, level * 100, the longitude wrap); its flips are the flags.  The packed values are decoded
    as the CF convention has it for int16 data whose scale and offset are float64: in float64.  Host-side I/O (scipy)."""
    from scipy.io import netcdf_file
    with netcdf_file(str(path), 'r', mmap=False) as f:
        def decode(name):
            v = f.variables[name]
            raw = np.array(v.data)
            out = raw.astype(np.float64)
            out *= np.float64(getattr(v, 'scale_factor', 1.0))
            out += np.float64(getattr(v, 'add_offset', 0.0))
            fill = getattr(v, '_FillValue', None)
            if fill is not None:
                out[raw == fill] = np.nan
            return np.squeeze(out)
        z, t, q = decode('z'), decode('t'), decode('q')
        lats = np.array(f.variables['latitude'].data, dtype=np.float64)
        lons = np.array(f.variables['longitude'].data, dtype=np.float64)
        level = np.array(f.variables['level'].data, dtype=np.float64) * 100          # ecmwf.py:260
    lons[lons > 180] -= 360                                                          # ecmwf.py:279
    if z.ndim != 3 or z.shape != (level.size, lats.size, lons.size):
        raise ValueError(f'{path}: z is {z.shape}, expected one time step on (level, latitude, longitude) = ({level.size}, {lats.size}, {lons.size})')
    if ll_bounds is not None:
        S, N, W, E = ll_bounds
        my, mx = (S <= lats) & (N >= lats), (W <= lons) & (E >= lons)
        lats, lons = lats[my], lons[mx]
        z, t, q = (v[:, my][:, :, mx] for v in (z, t, q))
    if z.size == 0:
        raise RuntimeError('There is no data in z, you may have a problem with your mask')           # ecmwf.py:332-333
    order = {}
    for name, axis in (('level', level), ('lats', lats), ('lons', lons)):
        d = np.diff(axis)
        if not (np.all(d > 0) or np.all(d < 0)):
            raise ValueError(f'{path}: {name} is not strictly monotonic')
        order[name] = bool(axis.size > 1 and d[0] < 0)
    c = np.ascontiguousarray
    return dict(z=c(z), t=c(t), q=c(q), level=level, lats=c(lats), lons=c(lons), ys=np.sort(lats), xs=np.sort(lons),
                top_first=not order['level'], rows_descending=order['lats'], cols_descending=order['lons'])


def load_ecmwf_pressure_levels(path, ll_bounds=None, new_z=None, return_state=False, ctx=None):
    """WeatherModel.load for a raw ERA-5 / HRES pressure-level file (weatherModel.py:235-262 with ECMWF._load_pressure_level,
    models/ecmwf.py:252-303): file -> geometric heights, broadcast pressures, surface-first ascending columns -> e -> uniform z
    levels -> NaN fill -> refractivities -> padded bottom level -> ZTDs, everything after the file read on the GPU.  Returns the
    ProcessedModel that tropo_delay / getInterpolators take.
    For a file as the CDS writes it (latitudes descending, levels top first) the columns are the reference's.  The reference
    re-orders `z` by other statements than `t` and `q` (:262-275); for a file with ascending latitudes those leave its heights
    mirrored in latitude and top first under surface-first temperatures.  Here every field follows the order flags of the file."""
    raw = read_ecmwf_pressure_level_file(path, ll_bounds)
    if new_z is None:
        new_z = np.flipud(ecmwf_pressure_level_heights())                                                  # ecmwf.py:39
    return cubes_from_pressure_levels(raw['xs'], raw['ys'], raw['z'], raw['level'], raw['t'], raw['q'], raw['lats'], height_kind=0,
                                      humidity_type='q', new_z=new_z, top_first=raw['top_first'], rows_descending=raw['rows_descending'],
                                      cols_descending=raw['cols_descending'], return_state=return_state, ctx=ctx)
