"""A RAiDER run-configuration file (`raider.py run.yaml`) read into the objects the driver works on.

The counterpart of tools/RAiDER/cli/types.py (the groups of a configuration), tools/RAiDER/cli/validators.py (what turns their
strings into dates, times, heights, an AOI and a line of sight) and tools/RAiDER/cli/raider.py:68-156 (read_run_config_file,
drop_nans).  What is shared with the reference is its interface: key names, defaults, function names, exception classes and
messages, and the arithmetic (golden g18).  Two things differ, both because nothing here may touch the network: a DEM is never
downloaded (`require_dem` raises DEMNotFound with the path at which one is expected), and the AOI classes are raider_amd.llreader's,
whose heights and raster bounds come from the device.
"""
import contextlib
import dataclasses
import datetime as dt
import os
import re
import time as _time
from pathlib import Path
from typing import Any, Optional

import numpy as np

from .llreader import AOI, BoundingBox, GeocodedFile, Geocube, RasterRDR, StationFile
from .logger import logger
from .losreader import LOS, Conventional, Raytracing, Zenith
from .models import WeatherModel, parse_weather_model

_CUBE_SPACING_IN_M = float(2000)          # constants.py:20
_BUFFER_SIZE = 0.2                        # validators.py:35: buffer in lat / lon degrees around a DEM's extent
GROUPS = ('date_group', 'time_group', 'aoi_group', 'height_group', 'los_group', 'runtime_group')
_DEM_NAME = 'GLO30.dem'                   # validators.py:94,117: what the reference would download into the output directory


class DEMNotFound(FileNotFoundError):
    """A run needs terrain heights, no DEM file is where one is expected, and the reference's DEM download is not part of this package."""

    def __init__(self, path, why):
        self.path = Path(path)
        super().__init__(f'{why}: a DEM is expected at {self.path} and is not there. The DEM download of the reference '
                         '(RAiDER.dem.download_dem) is not part of this package - put a lon / lat DEM at that path, give heights '
                         '(a Hgt_m column, height_file_rdr) or ask for height_levels')


# ---- the groups of a configuration (cli/types.py) --------------------------------------------------------------------------------
@dataclasses.dataclass
class DateGroupUnparsed:
    date_start: Any = None
    date_end: Any = None
    date_step: Any = None
    date_list: Any = None


@dataclasses.dataclass
class DateGroup:
    # (after parsing only the list is valid: dates from read_run_config_file, datetimes after checkArgs)
    date_list: list


class TimeGroup:
    """types.py:34-105: the acquisition time, the end of the acquisition window (30 s after it unless given) and the temporal
    interpolation method.  A time is read in the first spelling of TIME_FORMATS x TIMEZONE_FORMATS that fits."""
    _DEFAULT_ACQUISITION_WINDOW_SEC = 30
    TIME_FORMATS = ('', 'T%H:%M:%S.%f', 'T%H%M%S.%f', '%H%M%S.%f', 'T%H:%M:%S', '%H:%M:%S', 'T%H%M%S', '%H%M%S', 'T%H:%M', 'T%H%M',
                    '%H:%M', 'T%H')
    TIMEZONE_FORMATS = ('', 'Z', '%z')

    def __init__(self, time=None, end_time=None, interpolate_time=None):
        if time is None:
            raise ValueError('You must specify a "time" in the input config file')
        self.interpolate_time = interpolate_time
        self.time = self._as_time(time)
        note = ''
        if end_time is None:
            seconds = self._DEFAULT_ACQUISITION_WINDOW_SEC
            # a window that runs past midnight wraps to a small time of day, and is then refused below like an end before the start
            self.end_time = (dt.datetime.combine(dt.date(1900, 1, 1), self.time) + dt.timedelta(seconds=seconds)).time()
            note = f' (with default window of {seconds} seconds)'
        else:
            self.end_time = self._as_time(end_time)
        if self.end_time < self.time:
            raise ValueError(f'Acquisition start time must be before end time. Provided start time {self.time} is later than end time '
                             f'{self.end_time}{note}')

    @classmethod
    def _as_time(cls, value):
        return value if isinstance(value, dt.time) else cls.coerce_into_time(value)

    @staticmethod
    def coerce_into_time(val):
        """Hours, minutes and whole seconds of `val` (fractions and the zone are read and dropped)."""
        text = str(val)
        for spelling in TimeGroup._SPELLINGS:
            with contextlib.suppress(ValueError):
                return dt.time(*_time.strptime(text, spelling)[3:6])
        raise ValueError(f'Unable to coerce "{text}" to a time. Try T%H:%M:%S')


TimeGroup._SPELLINGS = tuple(clock + zone for clock in TimeGroup.TIME_FORMATS for zone in TimeGroup.TIMEZONE_FORMATS)


@dataclasses.dataclass
class AOIGroupUnparsed:
    bounding_box: Any = None
    geocoded_file: Optional[str] = None
    lat_file: Optional[str] = None
    lon_file: Optional[str] = None
    station_file: Optional[str] = None
    geo_cube: Optional[str] = None


@dataclasses.dataclass
class AOIGroup:
    aoi: AOI


@dataclasses.dataclass
class HeightGroupUnparsed:
    dem: Optional[str] = None
    use_dem_latlon: bool = False
    height_file_rdr: Optional[str] = None
    height_levels: Any = None


@dataclasses.dataclass
class HeightGroup:
    dem: Any
    use_dem_latlon: bool
    height_file_rdr: Optional[str]
    height_levels: Optional[list]


@dataclasses.dataclass
class LOSGroupUnparsed:
    ray_trace: bool = False
    los_file: Optional[str] = None
    los_convention: str = 'isce'
    los_cube: Optional[str] = None
    orbit_file: Optional[str] = None
    zref: Optional[float] = None


@dataclasses.dataclass
class LOSGroup:
    los: LOS
    ray_trace: bool = False
    los_file: Optional[str] = None
    los_convention: str = 'isce'
    los_cube: Optional[str] = None
    orbit_file: Optional[str] = None
    zref: Optional[float] = None


@dataclasses.dataclass
class RuntimeGroup:
    """types.py:157-188: formats, projection, cube spacing and the two directories (Paths; the weather-model directory defaults to
    `weather_files` under the output directory)."""
    raster_format: str = 'GTiff'
    file_format: str = 'GTiff'
    verbose: bool = True
    output_projection: str = 'EPSG:4326'
    cube_spacing_in_m: float = _CUBE_SPACING_IN_M
    download_only: bool = False
    output_directory: Any = '.'
    weather_model_directory: Any = None

    def __post_init__(self):
        self.output_directory = Path(self.output_directory)
        wm = self.weather_model_directory
        self.weather_model_directory = self.output_directory / 'weather_files' if wm is None else Path(wm)


@dataclasses.dataclass
class RunConfig:
    weather_model: WeatherModel
    date_group: DateGroup
    time_group: TimeGroup
    aoi_group: AOIGroup
    height_group: HeightGroup
    los_group: LOSGroup
    runtime_group: RuntimeGroup
    look_dir: str = 'right'
    cube_spacing_in_m: Optional[float] = None  # deprecated
    wetFilenames: Optional[list] = None
    hydroFilenames: Optional[list] = None


# ---- from strings to objects (cli/validators.py) -------------------------------------------------------------------------------
def get_los(los_group):
    """validators.py:54-78.  `ray_trace` picks the class; an orbit file comes before a line-of-sight file; a line-of-sight cube is
    refused; nothing given means zenith."""
    kind = Raytracing if los_group.ray_trace else Conventional
    if los_group.orbit_file is not None:
        return kind(los_group.orbit_file)
    if los_group.los_file is not None:
        return kind(los_group.los_file, los_group.los_convention)
    if los_group.los_cube is not None:
        raise NotImplementedError('LOS_cube is not yet implemented')
    return Zenith()


def _expected_dem(height_group, aoi_group, runtime_group):
    """Where the run expects its DEM (validators.py:90-117): the user's file, except that a station file without a Hgt_m column, or a
    run with neither a DEM nor a height raster, looks for GLO30.dem in the output directory.  A user's DEM that exists must hold a
    bounding-box AOI within _BUFFER_SIZE degrees."""
    fallback = runtime_group.output_directory / _DEM_NAME
    if height_group.dem is None:
        return fallback if height_group.height_file_rdr is None else None
    if aoi_group.station_file is not None:
        import pandas as pd
        return height_group.dem if 'Hgt_m' in pd.read_csv(aoi_group.station_file) else fallback
    if aoi_group.bounding_box is not None and Path(height_group.dem).exists():
        from .utilFcns import rio_extents, rio_profile
        S, N, W, E = rio_extents(rio_profile(height_group.dem))
        if isOutside(parse_bbox(aoi_group.bounding_box), getBufferedExtent((S, N), (W, E), buffer_size=_BUFFER_SIZE)):
            raise ValueError('Existing DEM does not cover the area of the input lat/lon points; either move the DEM, delete '
                             'it, or change the input points.')
    return height_group.dem


def _height_levels(spec):
    """`height_levels` as a list of floats (validators.py:119-131): a string gives its runs of digits and minus signs."""
    if spec is None:
        return None
    tokens = re.findall('[-0-9]+', spec) if isinstance(spec, str) else spec
    levels = np.array([float(tok) for tok in tokens])
    if np.any(levels < 0):
        logger.warning('Weather model only extends to the surface topography; '
                       'height levels below the topography will be interpolated from the surface and may be inaccurate.')
    return list(levels)


def get_heights(height_group, aoi_group, runtime_group):
    """validators.py:81-133: the height group of a run; `dem` becomes the path at which the run expects a DEM (_expected_dem)."""
    return HeightGroup(dem=_expected_dem(height_group, aoi_group, runtime_group), use_dem_latlon=height_group.use_dem_latlon,
                       height_file_rdr=height_group.height_file_rdr, height_levels=_height_levels(height_group.height_levels))


def _is_dem_name(path):
    """validators.py:168-173: a geocoded file whose name starts with SRTM or GLO is a DEM."""
    is_dem = path.name.upper().startswith(('SRTM', 'GLO'))
    if is_dem:
        logger.debug('Using user DEM: %s', path.name.upper())
    return is_dem


def get_query_region(aoi_group, height_group, cube_spacing_in_m):
    """validators.py:136-184: the AOI of a run.  The first that applies: the DEM's own grid (use_dem_latlon), lat / lon rasters (both
    or neither), a station file, a bounding box, a geocoded file, a geo cube."""
    spacing = dict(cube_spacing_in_m=cube_spacing_in_m)
    if height_group.use_dem_latlon:
        return GeocodedFile(Path(height_group.dem), is_dem=True, **spacing)
    rasters = (aoi_group.lat_file, aoi_group.lon_file)
    if any(f is not None for f in rasters):
        if None in rasters:
            raise ValueError('A lon_file must be specified if a lat_file is specified')
        return RasterRDR(*rasters, height_group.height_file_rdr, height_group.dem, **spacing)
    if aoi_group.station_file is not None:
        return StationFile(aoi_group.station_file, **spacing)
    if aoi_group.bounding_box is not None:
        snwe = parse_bbox(aoi_group.bounding_box)
        if np.min(snwe[0]) < -90 or np.max(snwe[1]) > 90:
            raise ValueError('Lats are out of N/S bounds; are your lat/lon coordinates switched? Should be SNWE')
        return BoundingBox(snwe, **spacing)
    if aoi_group.geocoded_file is not None:
        path = Path(aoi_group.geocoded_file)
        return GeocodedFile(path, is_dem=_is_dem_name(path), **spacing)
    if aoi_group.geo_cube is not None:
        return Geocube(aoi_group.geo_cube, cube_spacing_in_m)
    raise ValueError('No valid query points or bounding box found in the configuration file')


def parse_bbox(bbox):
    """validators.py:187-212: 'S N W E' as a string or a sequence -> (S, N, W, E): four numbers, a box with an area, inside the globe."""
    numbers = [float(v) for v in (bbox.split() if isinstance(bbox, str) else bbox)]
    if len(numbers) != 4:
        raise ValueError('bounding box must have 4 elements!')
    south, north, west, east = numbers
    if north <= south or east <= west:
        raise ValueError('Bounding box has no size; make sure you use "S N W E"')
    if any(lat < -90 or lat > 90 for lat in (south, north)):
        raise ValueError('Lats are out of S/N bounds (-90 to 90).')
    if any(lon < -180 or lon > 180 for lon in (west, east)):
        raise ValueError('Lons are out of W/E bounds (-180 to 180); Lons in the format of (0 to 360) are not supported.')
    return south, north, west, east


_DATE_SPELLINGS = ('%Y-%m-%d', '%Y%m%d', '%d', '%j')          # 2020-01-30, 20200130, a day of the month, a day of the year


def coerce_into_date(val):
    """validators.py:251-266: `val` read in the first of the four date spellings that fits."""
    for spelling in _DATE_SPELLINGS:
        with contextlib.suppress(ValueError):
            return dt.datetime.strptime(str(val), spelling).date()
    raise ValueError(f'Unable to coerce {val} to a date. Try %Y-%m-%d')


def _listed_dates(spec):
    """`date_list`: a string gives its runs of digits, one int stands for itself, a sequence is taken as it is."""
    if isinstance(spec, str):
        spec = re.findall('[0-9]+', spec)
    elif isinstance(spec, int):
        spec = [spec]
    return [coerce_into_date(item) for item in spec]


def _date_range(first, last, step):
    """Every `step`-th day from `first` to `last` inclusive (`last` defaults to `first`, `step` to one day)."""
    if first is None:
        raise ValueError('Inputs must include either date_list or date_start')
    start = coerce_into_date(first)
    days = (coerce_into_date(last) - start).days if last is not None else 0
    return [start + dt.timedelta(days=n) for n in range(0, days + 1, int(step) if step else 1)]


def parse_dates(date_group):
    """validators.py:215-248: `date_list` when given, else date_start [date_end [date_step]]."""
    if date_group.date_list is not None:
        return DateGroup(date_list=_listed_dates(date_group.date_list))
    return DateGroup(date_list=_date_range(date_group.date_start, date_group.date_end, date_group.date_step))


def getBufferedExtent(lats, lons, buffer_size=0.0):
    """validators.py:289-296: the SNWE box around lats / lons, grown by buffer_size."""
    return (min(lats) - buffer_size, max(lats) + buffer_size, min(lons) - buffer_size, max(lons) + buffer_size)


def isOutside(extent1, extent2):
    """validators.py:299-309: some edge of SNWE extent1 lies beyond that edge of extent2 (equal edges do not)."""
    s1, n1, w1, e1 = extent1
    s2, n2, w2, e2 = extent2
    return s1 < s2 or n1 > n2 or w1 < w2 or e1 > e2


def isInside(extent1, extent2):
    """validators.py:312-322: extent1 reaches at least as far as extent2 on every edge, as the reference compares them."""
    s1, n1, w1, e1 = extent1
    s2, n2, w2, e2 = extent2
    return s1 <= s2 and n1 >= n2 and w1 <= w2 and e1 >= e2


# ---- the file (cli/raider.py:68-156) ---------------------------------------------------------------------------------------------
def drop_nans(d):
    """raider.py:146-156: keys whose value is unset leave the mapping and its sub-mappings (one level), in place."""
    def unset(mapping):
        return [k for k, v in mapping.items() if v is None]
    for key in unset(d):
        del d[key]
    for group in d.values():
        if isinstance(group, dict):
            for key in unset(group):
                del group[key]
    return d


def _load_yaml(path):
    import yaml
    with Path(path).open() as stream:
        try:
            return yaml.safe_load(stream)
        except yaml.YAMLError as exc:
            print(exc)
            raise ValueError(f'Something is wrong with the yaml file {path}')


def read_run_config_file(path):
    """raider.py:68-143: the run configuration at `path` as a RunConfig: unset keys dropped, every group present, the look direction
    checked, the deprecated top-level cube_spacing_in_m moved into the runtime group, each group parsed."""
    raw = drop_nans(_load_yaml(path))
    group = {name: raw.get(name) or {} for name in GROUPS}

    look_dir = raw['look_dir']
    if not (isinstance(look_dir, str) and look_dir.lower() in ('right', 'left')):
        raise ValueError(f'Unknown look direction {look_dir}')
    if 'cube_spacing_in_m' in raw:
        logger.warning('Run config option cube_spacing_in_m is deprecated. Please use runtime_group.cube_spacing_in_m instead.')
        group['runtime_group']['cube_spacing_in_m'] = raw['cube_spacing_in_m']

    runtime = RuntimeGroup(**group['runtime_group'])
    heights, where = HeightGroupUnparsed(**group['height_group']), AOIGroupUnparsed(**group['aoi_group'])
    aoi = get_query_region(where, heights, cube_spacing_in_m=runtime.cube_spacing_in_m)
    model = parse_weather_model(raw['weather_model'], aoi)
    dates = parse_dates(DateGroupUnparsed(**group['date_group']))
    times = TimeGroup(**group['time_group'])
    height_group = get_heights(height_group=heights, aoi_group=where, runtime_group=runtime)
    los = get_los(LOSGroupUnparsed(**group['los_group']))
    return RunConfig(weather_model=model, date_group=dates, time_group=times, aoi_group=AOIGroup(aoi=aoi), height_group=height_group,
                     los_group=LOSGroup(los=los, **group['los_group']), runtime_group=runtime, look_dir=look_dir.lower())


# ---- where the reference would download a DEM ----------------------------------------------------------------------------------
def require_dem(run_config):
    """Before delays are computed at query points: make sure their heights can be had without a download.  A station file with a
    Hgt_m column, radar rasters with a height raster, a DEM AOI and every cube AOI need nothing.  Otherwise the DEM the height group
    names (`dem`: the user's, or GLO30.dem in the output directory, validators.py:94,117) must exist and is handed to the AOI;
    DEMNotFound names that path."""
    aoi, hg = run_config.aoi_group.aoi, run_config.height_group
    kind = aoi.type()
    if hg.height_levels is not None or kind in ('bounding_box', 'Geocube'):
        return
    if kind == 'station_file':
        import pandas as pd
        if 'Hgt_m' in pd.read_csv(aoi._filename):
            return
        why = f'the station file {aoi._filename} has no Hgt_m column'
    elif kind == 'radar_rasters':
        if aoi._hgtfile is not None and os.path.exists(aoi._hgtfile):
            return
        if aoi._demfile is not None and os.path.exists(aoi._demfile):
            return
        why = 'the lat / lon rasters come without a height raster'
    elif kind == 'geocoded_file':
        if aoi._is_dem:
            return
        why = f'the geocoded file {aoi._filename} is not a DEM'
    else:
        return
    dem = hg.dem if hg.dem is not None else run_config.runtime_group.output_directory / _DEM_NAME
    if not os.path.exists(dem):
        raise DEMNotFound(dem, why)
    if hasattr(aoi, '_demfile'):
        aoi._demfile = str(dem)
