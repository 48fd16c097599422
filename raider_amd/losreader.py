"""Line-of-sight types and ray geometry of the delay path (tools/RAiDER/losreader.py).

Same duck-typed LOS protocol as the reference (`is_Zenith`, `is_Projected`, `ray_trace`, `setPoints`,
`setTime`, `__call__`, `getLookVectors`; losreader.py:32-72,89,110,219).  isce3 (orbit -> look vector,
losreader.py:219-255) is outside this build's scope: `Raytracing` here is
ARRAY-BACKED - per-pixel look vectors or incidence/heading - and the geometry kernels
(getTopOfAtmosphere, build_ray) run on the GPU."""
import ctypes as C
from abc import ABC

import numpy as np

from . import _lib as L
from ._lib import Context, check, f64, ptr
from .constants import _ZREF
from .orbits import (cut_times, filter_ESA_orbit_file, get_sv, pick_ESA_orbit_file, read_ESA_Orbit_file,   # noqa: F401  (the reference keeps
                     read_txt_file)                                                                        # the orbit readers in this module)
from .utilFcns import cosd, enu2ecef, sind


class LOS(ABC):
    """The duck-typed line-of-sight protocol of the delay path (losreader.py:32-72): query flags (`is_Zenith`, `is_Projected`,
    `ray_trace`), target points (`setPoints`) and acquisition time (`setTime`).  The target points are kept as one
    (lats, lons, heights) triple; `_lats` / `_lons` / `_heights` are views of it for the subclasses."""

    _KINDS = dict(zenith=(True, False, False), projected=(False, True, False), raytrace=(False, False, True))

    def __init__(self, kind=None):
        self._points = (None, None, None)
        self._look_vecs = None
        self._time = None
        self._is_zenith, self._is_projected, self._ray_trace = self._KINDS.get(kind, (False, False, False))

    _lats = property(lambda self: self._points[0])
    _lons = property(lambda self: self._points[1])
    _heights = property(lambda self: self._points[2])

    def setPoints(self, lats, lons=None, heights=None):
        """Accepts (lats, lons, heights), (lats, lons) - heights then default to zero - or one stacked [..., 3] array."""
        if lats is None and self._points[0] is None:
            raise RuntimeError("You haven't given any point locations yet")
        if lons is None:                                  # stacked llh
            stacked = lats
            self._points = tuple(stacked[..., k] for k in range(3))
        else:
            self._points = (lats, lons, np.zeros((len(lats), 1)) if heights is None else heights)

    def setTime(self, datetime):
        self._time = datetime

    def is_Zenith(self):
        return self._is_zenith

    def is_Projected(self):
        return self._is_projected

    def ray_trace(self):
        return self._ray_trace


class Zenith(LOS):
    """Zenith delays are returned as they are (losreader.py:75-91)."""

    def __init__(self):
        super().__init__('zenith')

    def setLookVectors(self):
        if self._points[0] is None:
            raise ValueError('Target points not set')
        if self._look_vecs is None:
            self._look_vecs = getZenithLookVecs(*self._points)

    def __call__(self, delays):
        return delays


class Conventional(LOS):
    """Zenith delay projected with 1/cos(inc) (losreader.py:94-133).

    `filename` may be an ISCE-style 2-band LOS raster path (rasterio when installed, else raider_amd.rawraster), an orbit /
    state-vector file (losreader.py:122-128: the factor is then cos(look angle) from the zero-Doppler geometry, solved on
    the GPU instead of through isce3), or - array-backed extension - `inc`/`heading` rasters given directly."""

    def __init__(self, filename=None, los_convention='isce', time=None, pad=600, inc=None, heading=None):
        super().__init__('projected')
        self._file = filename
        self._time = time
        self._pad = pad
        self._convention = los_convention
        self._inc = None if inc is None else np.asarray(inc, dtype=np.float64)
        self._hd = None if heading is None else np.asarray(heading, dtype=np.float64)
        if self._convention.lower() != 'isce':
            raise NotImplementedError()
        if self._inc is not None and np.any(self._inc < 0):           # inc_hd_to_enu's check (losreader.py:386-387), once
            raise ValueError('inc_hd_to_enu: Incidence angle cannot be less than 0')
        self._raster = None

    def _divisor_source(self):
        """What `delays` are divided by (losreader.py:116-133), in the form the device kernels take it:
        ('inc', incidence in degrees - scalar or array; LOS_enu[..., -1] = cosd(inc) is evaluated on the device) for incidence /
        heading given as arrays or read from an ISCE-style two-band raster, or ('div', cos(look angle) array) from an orbit /
        state-vector file (state_to_los: the zero-Doppler geometry, solved on the GPU)."""
        if self._inc is not None:
            return 'inc', self._inc
        if self._file is None:
            raise ValueError('LOS file not set')
        if self._raster is not None:
            return self._raster
        from .rawraster import rio_open
        raster_error = None
        try:
            data, _ = rio_open(self._file)
            inc = np.asarray(data[0])
            if np.any(inc < 0):
                raise ValueError('inc_hd_to_enu: Incidence angle cannot be less than 0')
            # A float64 raster: cosd(inc) on the device.  Any other dtype (ISCE's los.rdr is float32): the reference's inc_hd_to_enu
            # evaluates cosd IN THAT DTYPE (losreader.py:393, NumPy keeps float32) and divides the float64 delays by the float32
            # cosine - reproduced by taking the cosine here, in the raster's dtype, once per file, and dividing on the device.
            self._raster = ('inc', inc) if inc.dtype == np.float64 else ('div', cosd(inc).astype(np.float64))
            return self._raster
        except (OSError, TypeError) as e:
            raster_error = e
        from .orbits import get_sv
        try:
            svs = np.stack(get_sv(self._file, self._time, self._pad), axis=-1)
        except ValueError as e:
            raise ValueError(f'{e}; as a line-of-sight raster it could not be read either: {raster_error}') from e
        return 'div', state_to_los(svs, [self._lats, self._lons, self._heights])

    def _enu(self):
        if self._inc is not None:
            hd = self._hd if self._hd is not None else np.zeros_like(self._inc)
            return inc_hd_to_enu(self._inc, hd)
        if self._file is None:
            raise ValueError('LOS file not set')
        # losreader.py:116-121: try the file as a 2-band LOS raster first (rasterio when installed, else the built-in reader of
        # flat-binary rasters with a .vrt / ENVI .hdr side-car: ISCE's los.rdr); anything that cannot be opened that way
        # (OSError / TypeError, exactly what the reference catches) is taken for an orbit / state-vector file.
        from .rawraster import rio_open
        raster_error = None
        try:
            data, _ = rio_open(self._file)
            return inc_hd_to_enu(*data)
        except (OSError, TypeError) as e:
            raster_error = e
        from .orbits import get_sv
        try:
            svs = np.stack(get_sv(self._file, self._time, self._pad), axis=-1)
        except ValueError as e:
            raise ValueError(f'{e}; as a line-of-sight raster it could not be read either: {raster_error}') from e
        return state_to_los(svs, [self._lats, self._lons, self._heights])

    def __call__(self, delays):
        """losreader.py:110-133."""
        if self._lats is None:
            raise ValueError('Target points not set')
        if self._file is None and self._inc is None:
            raise ValueError('LOS file not set')
        kind, arr = self._divisor_source()
        delays = np.asarray(delays)
        ctx = Context.default()
        # losreader.py:130-133: `delays / LOS_enu` when the shapes agree, else `delays / LOS_enu[..., -1]`
        if self._inc is not None or self._raster is not None:          # LOS_enu = (..., 3) ENU vectors; `arr` stands for their last component
            if delays.shape == np.shape(arr) + (3,):
                kind, arr = 'div', self._enu()
        elif delays.shape != np.shape(arr):                            # LOS_enu = cos(look angle) per target (an orbit file)
            arr = np.asarray(arr)[..., -1]
        shape = np.broadcast_shapes(delays.shape, np.shape(arr))
        out = np.array(np.broadcast_to(delays, shape), dtype=np.float64, order='C')            # (a fresh array: the kernel divides in place)
        d = f64(np.broadcast_to(np.asarray(arr, dtype=np.float64), shape))
        fn = ctx.lib.rdr_project_cosinc if kind == 'inc' else ctx.lib.rdr_project_divide
        check(fn(ctx.handle, ptr(out), None, ptr(d), out.size, L.RDR_HOST), ctx.handle)
        return out


class Raytracing(LOS):
    """Full ray tracing (losreader.py:136-255), array-backed.

    Give EITHER `look_vectors` (ny,nx,3) ECEF unit vectors ground->sensor (what the reference's
    getLookVectors returns, delay.py:270; reused for every height slice) OR `inc`/`heading` (deg, scalars or
    (ny,nx) rasters) from which the kernels derive the vectors per pixel (inc_hd_to_enu + enu2ecef).
    With `filename=` (an orbit / state-vector file, as in the reference) the zero-Doppler geometry is solved per pixel
    on the GPU (raider_amd.orbits.Orbit.look_vectors) - no isce3 needed; parity with isce3's geo2rdr is unpinned."""

    def __init__(self, filename=None, los_convention='isce', time=None, look_dir='right', pad=600,
                 look_vectors=None, inc=None, heading=None):
        super().__init__('raytrace')
        self._file = filename
        self._time = time
        self._pad = pad
        self._convention = los_convention
        self._orbit = None
        if self._convention.lower() != 'isce':
            raise NotImplementedError()
        if look_dir.lower() not in ('right', 'left'):
            raise RuntimeError(f'Unknown look direction: {look_dir}')
        self._look_dir = look_dir.lower()
        self._lv = None if look_vectors is None else np.ascontiguousarray(look_vectors, dtype=np.float64)
        self._inc = inc
        self._hd = heading if heading is not None else (0.0 if inc is not None else None)
        if self._lv is None and self._inc is None and self._file is None:
            raise ValueError('Raytracing needs an orbit file, look_vectors= or inc=/heading=')
        if self._file is not None and self._time is not None:
            self._orbit = get_orbit(self._file, self._time, pad=pad)          # losreader.py:188-190

    def setTime(self, time, pad=600):
        """losreader.py:214-217 (called from checkArgs)."""
        self._time = time
        if self._file is not None:
            self._orbit = get_orbit(self._file, self._time, pad=pad)

    def getSensorDirection(self):
        if self._orbit is None:
            raise ValueError('The orbit has not been set')
        return self._orbit.direction()

    def getLookDirection(self):
        return self._look_dir

    def ray_batch(self, xpts, ypts, ht=None):
        """Engine fast path: a `Rays` batch whose look vectors are generated / read on the device."""
        from .engine import Rays
        if self._lv is None and self._inc is None:
            # orbit-based: zero-Doppler solve per pixel on the device (replaces the isce3 loop, losreader.py:230-254)
            if self._orbit is None:
                raise ValueError('The orbit has not been set (call setTime)')
            return self._orbit_rays(xpts, ypts, [float(ht)], slices=0)
        if self._lv is not None:
            return Rays.grid(xpts, ypts, los=self._lv)
        return Rays.grid(xpts, ypts, inc=self._inc, hd=self._hd)

    def _orbit_rays(self, xpts, ypts, hts, slices, crs=None):
        """Orbit-based look vectors for every (height, y, x) target in ONE zero-Doppler launch.  With torch on the GPU the targets,
        the look vectors and the ray batch stay on the device (grid -> ECEF -> look vectors -> Rays, no host round trip: for a
        1000 x 1000 x 8 job the host route spends 20x the kernels' time moving 48 B per target back and forth); otherwise NumPy.
        crs=: a projected output grid (Rays.grid(..., crs=...)): the targets are its nodes' (lat, lon) at each height."""
        import sys
        from .engine import Rays, grid_geodetic, lla2ecef_device, torch_device_or_none
        # (importing torch costs a second or two once per process: worth it for anything but a small one-off job)
        big = np.size(xpts) * np.size(ypts) * np.size(hts) >= 1_000_000
        dev = torch_device_or_none() if (big or 'torch' in sys.modules) else None
        if dev is not None:
            import torch
            xt = torch.as_tensor(np.ascontiguousarray(xpts, dtype=np.float64), device=dev)
            yt = torch.as_tensor(np.ascontiguousarray(ypts, dtype=np.float64), device=dev)
            ht = torch.as_tensor(np.ascontiguousarray(hts, dtype=np.float64), device=dev)
            if crs is None:
                geo = None
                xyz = lla2ecef_device(yt[None, :, None], xt[None, None, :], ht[:, None, None])         # (S, ny, nx, 3)
            else:
                geo = grid_geodetic(crs, xt, yt)
                xyz = lla2ecef_device(geo[0][None], geo[1][None], ht[:, None, None])
            los = self._orbit.look_vectors(xyz)
            del xyz
            return Rays.grid(xt, yt, los=los if slices else los[0], slices=slices, crs=crs, geodetic=geo)
        from .utilFcns import lla2ecef
        if crs is None:
            geo = None
            xx, yy = np.meshgrid(xpts, ypts)
        else:
            geo = grid_geodetic(crs, xpts, ypts, device=None)
            yy, xx = geo
        xyz = np.stack([np.stack(lla2ecef(yy, xx, np.full(yy.shape, float(h))), axis=-1) for h in hts], axis=0)
        los = self._orbit.look_vectors(xyz)
        return Rays.grid(xpts, ypts, los=los if slices else los[0], slices=slices, crs=crs, geodetic=geo)

    def ray_batch_slices(self, xpts, ypts, hts, crs=None):
        """Engine fast path for the whole height loop of _build_cube_ray: ONE `Rays` batch covering every slice.  Look vectors
        given as arrays / incidence + heading are the same for every height (as in getLookVectors); orbit-based ones depend on
        the target height (losreader.py:219-255) and are solved for all slices in one zero-Doppler launch.  crs=: the axes are those
        of a grid in a projected CRS (UTM, LCC, polar stereographic; delay.py:259-263) - an LLH batch on its nodes (Rays.grid)."""
        from .engine import Rays
        hts = np.atleast_1d(np.asarray(hts, dtype=np.float64))
        if self._lv is None and self._inc is None:
            if self._orbit is None:
                raise ValueError('The orbit has not been set (call setTime)')
            return self._orbit_rays(xpts, ypts, hts, slices=hts.size, crs=crs)
        if self._lv is not None:
            return Rays.grid(xpts, ypts, los=self._lv, crs=crs)
        return Rays.grid(xpts, ypts, inc=self._inc, hd=self._hd, crs=crs)

    def getIntersectionWithHeight(self, height):
        """losreader.py:257-263: where the rays from `self._xyz` along `self._look_vecs` reach `height` (getTopOfAtmosphere)."""
        return getTopOfAtmosphere(self._xyz, self._look_vecs, height)

    def getIntersectionWithLevels(self, levels):
        """losreader.py:265-288: (self._lats.shape, len(levels), 3) ray points at the level transitions; NaN where the target
        is above the level."""
        rays = np.zeros(list(np.shape(self._lats)) + [len(levels), 3])
        for ind, z in enumerate(levels):
            value = self.getIntersectionWithHeight(z)
            value[np.asarray(self._heights) > z, :] = np.nan
            rays[..., ind, :] = value
        return rays

    def calculateDelays(self, delays):
        """losreader.py:290-299."""
        raise NotImplementedError

    def getLookVectors(self, ht, llh, xyz, yy):
        """delay.py:270 protocol: (ny,nx,3) unit ECEF vectors."""
        if self._lv is None and self._inc is None:
            if self._orbit is None:
                raise ValueError('The orbit has not been set (call setTime)')
            return self._orbit.look_vectors(xyz)
        if self._lv is not None:
            if self._lv.shape != yy.shape + (3,):
                raise ValueError(f'look_vectors have shape {self._lv.shape}, expected {yy.shape + (3,)}')
            return self._lv
        inc = np.broadcast_to(np.asarray(self._inc, dtype=np.float64), yy.shape)
        hd = np.broadcast_to(np.asarray(self._hd, dtype=np.float64), yy.shape)
        enu = inc_hd_to_enu(inc, hd)
        return enu2ecef(enu[..., 0], enu[..., 1], enu[..., 2], llh[1], llh[0], llh[2])


def get_orbit(orbit_file, ref_time, pad):
    """losreader.py:736-769: state vectors within `pad` seconds of ref_time, unique and time-ordered."""
    from .orbits import Orbit
    return Orbit.from_file(orbit_file, ref_time, pad)


def get_radar_pos(llh, orb):
    """losreader.py:630-703: look angle (deg) between the line of sight and the ellipsoid normal, and the slant range (m), of
    the targets llh[:, (lat, lon, h)] at zero Doppler; NaN targets stay NaN.  `orb` is a raider_amd.orbits.Orbit (the
    reference takes an isce3 Orbit: the geometry solve here is this build's own)."""
    from .utilFcns import lla2ecef
    llh = np.asarray(llh, dtype=np.float64)
    xyz = np.stack(lla2ecef(llh[:, 0], llh[:, 1], llh[:, 2]), axis=-1)
    los, _, sr = orb.look_vectors(xyz, threshold=1.0e-7, maxiter=30, return_geometry=True)
    nv = getZenithLookVecs(llh[:, 0], llh[:, 1], llh[:, 2])              # isce3 Ellipsoid.n_vector(lon, lat)
    ang = np.rad2deg(np.arccos(np.sum(los * nv, axis=-1)))
    bad = np.isnan(llh).any(axis=-1)
    ang[bad] = np.nan; sr = np.where(bad, np.nan, sr)
    return ang, sr


def state_to_los(svs, llh_targets):
    """losreader.py:558-607: cos(look angle) at every (lat, lon, height) target from state vectors svs[n, 7] =
    (t, x, y, z, vx, vy, vz)."""
    from .orbits import Orbit
    svs = np.asarray(svs)
    if np.min(svs.shape) < 4:
        raise RuntimeError('state_to_los: At least 4 state vectors are required for orbit interpolation')
    orb = Orbit(list(svs[:, 0]), svs[:, 1:4].astype(np.float64), svs[:, 4:7].astype(np.float64))
    in_shape = np.shape(llh_targets[0])
    target_llh = np.stack([np.asarray(x, dtype=np.float64).flatten() for x in llh_targets], axis=-1)
    los_ang, _ = get_radar_pos(target_llh, orb)
    return np.cos(np.deg2rad(los_ang)).reshape(in_shape)


def getZenithLookVecs(lats, lons, heights):
    """losreader.py:302-316."""
    x = np.cos(np.radians(lats)) * np.cos(np.radians(lons))
    y = np.cos(np.radians(lats)) * np.sin(np.radians(lons))
    z = np.sin(np.radians(lats))
    return np.stack([x, y, z], axis=-1)


def inc_hd_to_enu(incidence, heading):
    """losreader.py:374-396."""
    if np.any(np.asarray(incidence) < 0):
        raise ValueError('inc_hd_to_enu: Incidence angle cannot be less than 0')
    east = sind(incidence) * cosd(heading + 90)
    north = sind(incidence) * sind(heading + 90)
    up = cosd(incidence)
    return np.stack((east, north, up), axis=-1)


def getTopOfAtmosphere(xyz, look_vecs, toaheight, factor=None):
    """losreader.py:706-733 on the GPU: Newton intersection of rays with the height surface `toaheight`
    (10 iterations with factor 1 if `factor` is None, else 3 iterations with the per-pixel factor)."""
    xyz = np.asarray(xyz, dtype=np.float64)
    shp = xyz.shape
    x = f64(xyz).reshape(-1, 3)
    l = f64(np.broadcast_to(look_vecs, shp)).reshape(-1, 3)
    n = x.shape[0]
    fac = None if factor is None else f64(np.broadcast_to(factor, shp[:-1])).ravel()
    pos = np.empty((n, 3))
    ctx = Context.default()
    check(ctx.lib.rdr_top_of_atmosphere(ctx.handle, ptr(x), ptr(l), n, float(toaheight), ptr(fac), ptr(pos), L.RDR_HOST), ctx.handle)
    return pos.reshape(shp)


def build_ray(model_zs, ht, xyz, LOS, MAX_TROPO_HEIGHT=_ZREF):
    """losreader.py:772-835 on the GPU: (ray_lengths (K,...), low_xyzs (K,...,3), high_xyzs (K,...,3)) or
    (None, None, None) when no model interval contributes.  (The ray tracer proper never materialises
    these - it fuses this computation into the integration kernel.)"""
    model_zs = f64(model_zs).ravel()
    xyz = np.asarray(xyz, dtype=np.float64)
    shp = xyz.shape[:-1]
    x = f64(xyz).reshape(-1, 3)
    l = f64(np.broadcast_to(LOS, xyz.shape)).reshape(-1, 3)
    n = x.shape[0]
    ctx = Context.default()
    K = C.c_int32()
    rc = ctx.lib.rdr_build_ray(ctx.handle, ptr(model_zs), model_zs.size, float(ht), ptr(x), ptr(l), n, float(MAX_TROPO_HEIGHT),
                               C.byref(K), None, None, None, L.RDR_HOST)
    if rc == L.RDR_ERR_NO_LEVELS:
        return None, None, None
    check(rc, ctx.handle)
    k = K.value
    lengths, low, high = np.empty((k, n)), np.empty((k, n, 3)), np.empty((k, n, 3))
    check(ctx.lib.rdr_build_ray(ctx.handle, ptr(model_zs), model_zs.size, float(ht), ptr(x), ptr(l), n, float(MAX_TROPO_HEIGHT),
                                C.byref(K), ptr(lengths), ptr(low), ptr(high), L.RDR_HOST), ctx.handle)
    return lengths.reshape((k,) + shp), low.reshape((k,) + shp + (3,)), high.reshape((k,) + shp + (3,))
