"""Areas of interest as calcDelays builds them - the counterpart of tools/RAiDER/llreader.py:29-430, class for class.

An AOI says where delays are wanted: a bounding box or a geocube (delay cubes on a grid), a station file, a pair of radar-geometry
lat / lon rasters, or a geocoded file (delays at query points).  Arithmetic and rounding are the reference's.  What differs:
  * a CRS is what the rest of this package takes for one (the int 4326 / an EPSG code, a PROJ string or dict, a pyproj.CRS when pyproj
    is installed), not necessarily a pyproj object;
  * the bounds of lat / lon rasters and the DEM heights of pixels and stations are computed on the device (interpolator.raster_bounds,
    interpolateDEM);
  * nothing is downloaded: where the reference would fetch a DEM (RAiDER.dem.download_dem) a FileNotFoundError says that none was
    given.
"""
import os
from pathlib import Path

import numpy as np

from .logger import logger


def _file_part(filestr):
    """The file of a `file;band` string (utilFcns.get_file_and_band)."""
    from .utilFcns import get_file_and_band
    return get_file_and_band(str(filestr))[0]


def _read_raster(filestr):
    """rio_open of `file` (every band, squeezed, as the reference reads it) or of the one band `file;band` names."""
    from .utilFcns import get_file_and_band, rio_open
    path, band = get_file_and_band(str(filestr))
    return rio_open(path, band=band if ';' in str(filestr) else None)[0]


def _stations(station_file):
    """The station table, one row per (Lat, Lon) (llreader.py:206,211,428)."""
    import pandas as pd
    return pd.read_csv(station_file).drop_duplicates(subset=['Lat', 'Lon'])


def _no_dem(what):
    return FileNotFoundError(f'{what}: no DEM was given (or the file does not exist), and the DEM download step of the reference '
                             '(RAiDER.dem.download_dem) is not part of this package - pass the path of a lon / lat DEM')


class AOI:
    """llreader.py:29-191: the generic AOI.

    Attributes:
       _bounding_box    - S N W E bounding box
       _proj            - CRS (EPSG:4326)
       _type            - Type of AOI
    """

    def __init__(self, cube_spacing_in_m=None):
        self._output_directory = os.getcwd()
        self._bounding_box = None
        self._proj = 4326
        self._geotransform = None
        self._cube_spacing_m = cube_spacing_in_m

    def __repr__(self):
        return f'AOI: {self.__class__.__name__}({self._bounding_box}, {self._type})'

    def type(self):
        return self._type

    def bounds(self):
        return list(self._bounding_box).copy()

    def geotransform(self):
        return self._geotransform

    def projection(self):
        return self._proj

    def get_output_spacing(self, crs=4326):
        """Return the output spacing in desired units: degrees for a lon / lat CRS, else metres at 1e5 m per degree."""
        from .delay import _is_4326
        output_spacing_deg = self._output_spacing
        return output_spacing_deg if _is_4326(crs) else output_spacing_deg * 1e5

    def set_output_spacing(self, ll_res=None):
        """The spacing of the output grid: the requested cube spacing if there is one, else the weather model's own."""
        assert ll_res or self._cube_spacing_m, 'Must pass lat/lon resolution if _cube_spacing_m is None'
        out_spacing = self._cube_spacing_m / 1e5 if self._cube_spacing_m else ll_res
        logger.debug(f'Output cube spacing: {out_spacing} degrees')
        self._output_spacing = out_spacing

    def add_buffer(self, ll_res, digits=2):
        """llreader.py:91-128: grow the box by 1.5 weather-model cells, clip it outwards to a multiple of the output spacing, round."""
        from .utilFcns import clip_bbox

        S, N, W, E = self.bounds()
        buffer = 1.5 * ll_res
        S, N = np.max([S - buffer, -90]), np.min([N + buffer, 90])
        W, E = W - buffer, E + buffer  # (dateline crossings are not handled, as in the reference)

        self.set_output_spacing(ll_res)
        S, N, W, E = clip_bbox([S, N, W, E], self._output_spacing)

        if np.max([np.abs(W), np.abs(E)]) > 180:
            logger.warning('Bounds extend past +/- 180. Results may be incorrect.')

        self._bounding_box = [np.round(a, digits) for a in (S, N, W, E)]

    def calc_buffer_ray(self, direction, lookDir='right', incAngle=30, maxZ=80, digits=2):
        """llreader.py:131-168: the east-west buffer ray tracing needs on the side nearest the sensor (maxZ in km)."""
        direction = direction.lower()
        try:
            lookDir = lookDir.name.lower()       # (an isce LookSide)
        except AttributeError:
            lookDir = lookDir.lower()

        assert direction in 'asc desc'.split(), f'Incorrection orbital direction: {direction}. Choose asc or desc.'
        # The reference's list really is 'right light': 'left' fails this assertion there too, and does here - the branch for it below
        # is as unreachable as the reference's.
        assert lookDir in 'right light'.split(), f'Incorrection look direction: {lookDir}. Choose right or left.'

        S, N, W, E = self.bounds()

        lat_max = np.max([np.abs(S), np.abs(N)])
        near = maxZ * np.tan(np.deg2rad(incAngle))
        buffer = near / (np.cos(np.deg2rad(lat_max)) * 100)

        if (lookDir == 'right' and direction == 'asc') or (lookDir == 'left' and direction == 'desc'):
            W = W - buffer
        else:
            E = E + buffer

        bounds = [np.round(a, digits) for a in (S, N, W, E)]
        if np.max([np.abs(W), np.abs(E)]) > 180:
            logger.warning('Bounds extend past +/- 180. Results may be incorrect.')
        return bounds

    def set_output_directory(self, output_directory):
        self._output_directory = output_directory

    def set_output_xygrid(self, dst_crs=4326):
        """llreader.py:173-191: the nodes delays are returned on, in `dst_crs`."""
        from .utilFcns import transform_bbox
        out_proj = dst_crs
        if isinstance(dst_crs, str) and dst_crs.upper().startswith('EPSG:'):
            out_proj = int(dst_crs.split(':')[-1])

        out_snwe = transform_bbox(self.bounds(), src_crs=4326, dest_crs=out_proj)
        logger.debug(f'Output SNWE: {out_snwe}')

        out_spacing = self.get_output_spacing(out_proj)
        self.xpts = np.arange(out_snwe[2], out_snwe[3] + out_spacing, out_spacing)
        self.ypts = np.arange(out_snwe[1], out_snwe[0] - out_spacing, -out_spacing)


class StationFile(AOI):
    """Use a .csv file containing at least Lat, Lon, and optionally Hgt_m columns."""

    def __init__(self, station_file, demFile=None, cube_spacing_in_m=None):
        super().__init__(cube_spacing_in_m)
        self._filename = station_file
        self._demfile = demFile
        self._bounding_box = bounds_from_csv(station_file)
        self._type = 'station_file'

    def readLL(self):
        """Read the station lat/lons from the csv file."""
        df = _stations(self._filename)
        return df['Lat'].to_numpy(), df['Lon'].to_numpy()

    def readZ(self):
        """The station heights: the file's Hgt_m column, else sampled from `demFile` and written back to the file."""
        df = _stations(self._filename)
        if 'Hgt_m' in df.columns:
            return df['Hgt_m'].values
        from .interpolator import interpolateDEM
        if self._demfile is None or not os.path.exists(self._demfile):
            raise _no_dem(f'{self._filename} has no Hgt_m column')
        # (the reference takes the diagonal of an outer-product interpolation here; interpolateDEM returns the stations' own heights)
        z_out = interpolateDEM(self._demfile, self.readLL())
        if np.isnan(z_out).all():
            raise Exception('DEM interpolation failed. Check DEM bounds and station coords.')
        df['Hgt_m'] = z_out
        df.to_csv(self._filename, index=False)
        self.__init__(self._filename)
        return z_out


class RasterRDR(AOI):
    """Use a 2-band raster file containing lat/lon coordinates."""

    def __init__(self, lat_file, lon_file=None, hgt_file=None, dem_file=None, convention='isce', cube_spacing_in_m=None):
        super().__init__(cube_spacing_in_m)
        self._type = 'radar_rasters'
        self._latfile = lat_file
        self._lonfile = lon_file

        if (self._latfile is None) and (self._lonfile is None):
            raise ValueError('You need to specify a 2-band file or two single-band files')

        if not os.path.exists(_file_part(self._latfile)):
            raise ValueError(f'{self._latfile} cannot be found!')

        try:
            bpg = bounds_from_latlon_rasters(lat_file, lon_file)
            self._bounding_box, self._proj, self._geotransform = bpg
        except Exception as e:
            raise ValueError(f'Could not read lat/lon rasters: {e}')

        self._hgtfile = hgt_file
        self._demfile = dem_file
        self._convention = convention

    def readLL(self):
        lats = _read_raster(self._latfile)
        if self._lonfile is None:
            return lats, None                 # (a 2-band lat / lon raster)
        return lats, _read_raster(self._lonfile)

    def readZ(self):
        """The pixel heights: `hgt_file` when it exists, else `dem_file` sampled at the pixels (nearest, on the device)."""
        from .utilFcns import rio_open
        if self._hgtfile is not None and os.path.exists(self._hgtfile):
            logger.info('Using existing heights at: %s', self._hgtfile)
            hgts, _ = rio_open(self._hgtfile)
            return hgts
        from .interpolator import interpolateDEM
        if self._demfile is None or not os.path.exists(self._demfile):
            raise _no_dem('RasterRDR without a height raster')
        return interpolateDEM(self._demfile, self.readLL())


class BoundingBox(AOI):
    """Parse a bounding box AOI."""

    def __init__(self, bbox, cube_spacing_in_m=None):
        super().__init__(cube_spacing_in_m)
        self._bounding_box = bbox
        self._type = 'bounding_box'


class GeocodedFile(AOI):
    """Parse a Geocoded file for coordinates."""

    def __init__(self, path, is_dem=False, cube_spacing_in_m=None):
        super().__init__(cube_spacing_in_m)

        from .utilFcns import _gdal_transform, rio_extents, rio_profile

        self._filename = path
        self.p = rio_profile(Path(path))
        self._bounding_box = rio_extents(self.p)
        self._is_dem = is_dem
        # (the reference takes these two from rio_stats and drops the statistics; the profile holds them without a pass over the pixels)
        self._proj = 4326 if self.p.get('crs') is None else self.p['crs']
        self._geotransform = _gdal_transform(self.p)
        self._type = 'geocoded_file'
        try:
            self.crs = self.p['crs']
        except KeyError:
            self.crs = None

    def readLL(self):
        # ll_bounds are SNWE
        S, N, W, E = self._bounding_box
        w, h = self.p['width'], self.p['height']
        px = (E - W) / w
        py = (N - S) / h
        x = np.array([W + (t * px) for t in range(w)])
        y = np.array([S + (t * py) for t in range(h)])
        X, Y = np.meshgrid(x, y)
        return Y, X  # lats, lons

    def readZ(self):
        """Heights at readLL(): the file itself when it is a DEM."""
        from .interpolator import interpolateDEM
        if not self._is_dem:
            raise _no_dem(f'{self._filename} is not a DEM')
        return interpolateDEM(self._filename, self.readLL())


class Geocube(AOI):
    """Pull lat/lon/height from a georeferenced data cube."""

    def __init__(self, path_cube, cube_spacing_in_m=None):
        super().__init__(cube_spacing_in_m)
        self.path = path_cube
        self._type = 'Geocube'
        self._bounding_box = self.get_extent()
        # (the reference asks rio_stats = GDAL for the cube's CRS and geotransform; here the cube is taken to be in lon / lat and the
        # geotransform follows from its two axes: nodes are pixel centres)
        lats, lons = self._axes()
        if lats.size > 1 and lons.size > 1:
            dx, dy = float(lons[1] - lons[0]), float(lats[1] - lats[0])
            self._geotransform = (float(lons[0]) - dx / 2, dx, 0.0, float(lats[0]) - dy / 2, 0.0, dy)

    def _read(self, name):
        """One variable of the cube file (NetCDF-4 through h5lite, NetCDF-3 through scipy, xarray when it is installed)."""
        from .delayFcns import _load_fields
        return np.asarray(_load_fields(self.path)[1](name))

    def _axes(self):
        return self._read('latitude'), self._read('longitude')

    def get_extent(self):
        lats, lons = self._axes()
        return [float(lats.min()), float(lats.max()), float(lons.min()), float(lons.max())]

    def readLL(self):
        """The mesh of the cube's two axes (the reference's version is marked untested and misspells `latitude`)."""
        lats, lons = self._axes()
        Lats, Lons = np.meshgrid(lats, lons)
        return Lats, Lons

    def readZ(self):
        return self._read('heights')


def bounds_from_latlon_rasters(lat_filestr, lon_filestr):
    """llreader.py:397-420: (SNWE, CRS, geotransform) of a lat and a lon raster; the four extremes come from ONE device pass over both
    rasters (NaN and no-data pixels left out)."""
    from .interpolator import raster_bounds
    from .rawraster import rio_open
    from .utilFcns import get_file_and_band

    latinfo = get_file_and_band(lat_filestr)
    loninfo = get_file_and_band(lon_filestr)
    lat, lat_prof = rio_open(latinfo[0], band=latinfo[1])
    lon, lon_prof = rio_open(loninfo[0], band=loninfo[1])
    lat_proj, lon_proj = lat_prof.get('crs'), lon_prof.get('crs')
    lat_gt, lon_gt = lat_prof.get('transform'), lon_prof.get('transform')

    assert lat_proj == lon_proj, 'Projection information for Latitude and Longitude files does not match'
    assert lat_gt == lon_gt, 'Affine transform for Latitude and Longitude files does not match'
    assert lat.shape == lon.shape, 'Latitude and Longitude files differ in size'

    if lat_prof.get('nodata') == lon_prof.get('nodata') and lat.dtype == lon.dtype:
        lat_stats, lon_stats = raster_bounds(lat, lon, nodata=lat_prof.get('nodata'))
    else:                                                   # (two no-data values or element types: a pass each)
        lat_stats = raster_bounds(lat, None, nodata=lat_prof.get('nodata'))[0]
        lon_stats = raster_bounds(lon, None, nodata=lon_prof.get('nodata'))[0]
    if lat_stats[2] == 0 or lon_stats[2] == 0:
        raise ValueError('a lat / lon raster holds no valid pixel')

    # (dateline crossings are not handled, as in the reference)
    snwe = (lat_stats[0], lat_stats[1], lon_stats[0], lon_stats[1])

    if lat_proj is None:
        logger.debug('Assuming lat/lon files are in EPSG:4326')
        lat_proj = 4326
    if lat_gt is not None:
        lat_gt = tuple(lat_gt.to_gdal()) if hasattr(lat_gt, 'to_gdal') else tuple(lat_gt)

    return snwe, lat_proj, lat_gt


def bounds_from_csv(station_file):
    """station_file: a comma-delimited file with at least "Lat" and "Lon" columns in EPSG:4326."""
    stats = _stations(station_file)
    snwe = [stats['Lat'].min(), stats['Lat'].max(), stats['Lon'].min(), stats['Lon'].max()]
    return snwe
