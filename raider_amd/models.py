"""What the run-configuration driver needs to know about a weather model, without any fetcher: names, resolutions, time steps,
valid ranges, projections, and the bounds / file-name / containment arithmetic of tools/RAiDER/models/weatherModel.py.

One class serves every model; the per-model facts are the table `_FACTS` (mirrors the constructors of models/era5.py, era5t.py,
erai.py, hres.py, gmao.py, merra2.py, hrrr.py, ncmr.py).  Nothing here downloads or loads model data: raw files are processed by
raider_amd.weather, through raider_amd.processWM.

The one intended difference from the reference: HRRR / HRRR-AK validity (models/hrrr.py:323-356) is decided there against a
coverage polygon held in its source; here the AOI is tested against the extent of the model's own grid in the model's own
projection (the grid definitions NCEP publishes: first node, node counts, 3 km spacing), through the conic / stereographic
transforms of raider_amd.utilFcns.  The outcomes are the same three - covered, partly covered (logged as critical), not covered
(HRRR then tries HRRR-AK, then raises) - but the edge of "covered" is the grid's true edge, not a hand-drawn quadrilateral.
"""
import calendar
import datetime as dt
import os
from pathlib import Path

import numpy as np

from .logger import logger

_UTC = dt.timezone(offset=dt.timedelta())


# ---- models/customExceptions.py --------------------------------------------------------------------------------------------
class DatetimeOutsideRange(Exception):
    def __init__(self, model, time):
        super().__init__(f'Time {time} is outside the available date range for weather model {model}')


class ExistingWeatherModelTooSmall(Exception):
    def __init__(self):
        super().__init__('The weather model passed does not cover all of the input points; you may need to download a larger area.')


# ---- the per-model facts -------------------------------------------------------------------------------------------------
_HRRR_PROJ = '+proj=lcc +lat_1=38.5 +lat_2=38.5 +lat_0=38.5 +lon_0=262.5 +x_0=0 +y_0=0 +a=6371229 +b=6371229 +units=m +no_defs'  # hrrr.py:248-259
_HRRRAK_PROJ = ('+proj=stere +ellps=sphere +a=6371229.0 +b=6371229.0 +lat_0=90 +lon_0=225.0 +x_0=0.0 +y_0=0.0 +lat_ts=60.0 '
                '+no_defs +type=crs')                                                                                             # hrrr.py:22-25
# The two grids as their GRIB grid definitions give them: (latitude, longitude of the first node, nx, ny, spacing in m).  The CONUS
# line is the one models/hrrr.py:245 quotes; the Alaska grid is NCEP's 3 km polar-stereographic Alaska domain.
_GRIDS = {'HRRR': (21.138123, 237.280472, 1799, 1059, 3000.0), 'HRRR-AK': (41.612949, 185.117126, 1299, 919, 3000.0)}

#            _Name      _dataset   _classname  dtime  lat_res     lon_res     valid from        until     lag                      levels  projection
_FACTS = {
    'ERA5':   ('ERA-5',   'era5',    'ea',       1,     0.25,       0.25,       (1950, 1, 1),     'era5',   None,                    'ml',   4326),
    'ERA5T':  ('ERA-5T',  'era5t',   'ea',       1,     0.25,       0.25,       (1950, 1, 1),     'now',    dt.timedelta(days=1),    'ml',   4326),
    'ERAI':   ('ERA-I',   'interim', 'ei',       1,     0.25,       0.25,       (1979, 1, 1),     (2019, 8, 31), dt.timedelta(days=30), 'ml', 4326),
    'HRES':   ('HRES',    'hres',    'od',       6,     9.0 / 111,  9.0 / 111,  (1983, 4, 20),    'now',    dt.timedelta(hours=6),   'ml',   4326),
    'GMAO':   ('GMAO',    'gmao',    'gmao',     3,     0.25,       0.3125,     (2014, 2, 20),    'now',    dt.timedelta(hours=24),  'ml',   4326),
    'MERRA2': ('MERRA2',  'merra2',  'merra2',   1,     0.5,        0.625,      (1980, 1, 1),     'now',    'merra2',                'ml',   4326),
    'HRRR':   ('HRRR',    'hrrr',    'hrrr',     1,     3.0 / 111,  3.0 / 111,  (2016, 7, 15),    'now',    dt.timedelta(hours=3),   'nat',  _HRRR_PROJ),
    'HRRRAK': ('HRRR-AK', 'hrrrak',  'hrrrak',   3,     3.0 / 111,  3.0 / 111,  (2018, 7, 13),    'now',    dt.timedelta(hours=3),   'nat',  _HRRRAK_PROJ),
    'NCMR':   ('NCMR',    'ncmr',    'ncmr',     1,     0.11718750, 0.17578125, (2015, 12, 1),    'now',    dt.timedelta(hours=6),   'ml',   4326),
}
# What parse_weather_model resolves: the reference imports `RAiDER.models.<name>` (validators.py:269-286), and there is no module
# for HRRR-AK - that model is reached only by HRRR casting itself (hrrr.py:284-298).
_PARSEABLE = ('ERA5', 'ERA5T', 'ERAI', 'HRES', 'GMAO', 'MERRA2', 'HRRR', 'NCMR')


def _months_back(t, months):
    """t - relativedelta(months=months): the calendar month moves, the day is clipped to the month's length."""
    y, m = divmod(t.year * 12 + (t.month - 1) - months, 12)
    return t.replace(year=y, month=m + 1, day=min(t.day, calendar.monthrange(y, m + 1)[1]))


class _MonthsLag:
    """The `relativedelta(months=3)` lag of ERA-5 (era5.py:23-31): `now - lag` steps back by calendar months."""

    def __init__(self, months):
        self.months = months

    def __rsub__(self, t):
        return _months_back(t, self.months)

    def __repr__(self):
        return f'relativedelta(months=+{self.months})'


class WeatherModel:
    """The driver's view of one weather model (weatherModel.py:35-101 without the data arrays)."""

    def __init__(self, key):
        key = str(key).upper().replace('-', '')
        if key not in _FACTS:
            raise KeyError(key)
        self._wmLoc = None
        self._time = None
        self._bbox = None
        self._ll_bounds = None
        self._set_facts(key)

    def _set_facts(self, key):
        name, dataset, classname, step, lat_res, lon_res, start, until, lag, levels, proj = _FACTS[key]
        self._key, self._Name, self._dataset, self._classname = key, name, dataset, classname
        self._time_res = step
        self._lat_res, self._lon_res = lat_res, lon_res
        self._model_level_type = levels
        self._proj = proj
        now = dt.datetime.now(dt.timezone.utc)
        if until == 'era5':                                                         # era5.py:23-31
            lag = _MonthsLag(3)
            end = _months_back(dt.datetime.today(), 3).replace(tzinfo=_UTC)
        elif until == 'now':
            end = now
        else:
            end = dt.datetime(*until).replace(tzinfo=_UTC)
        if lag == 'merra2':                                                         # merra2.py:41-49
            enddate = dt.datetime(now.year, now.month, 15) - dt.timedelta(days=60)
            enddate = dt.datetime(enddate.year, enddate.month, calendar.monthrange(enddate.year, enddate.month)[1])
            lag = dt.timedelta(days=(now - enddate.replace(tzinfo=_UTC)).days)
        self._valid_range = (dt.datetime(*start).replace(tzinfo=_UTC), end)
        self._lag_time = lag

    def __repr__(self):
        return f'WeatherModel({self._Name})'

    # -- weatherModel.py:134-144 -----------------------------------------------------------------------------------------
    def Model(self):
        """Returns the name of the weather model."""
        return self._Name

    def dtime(self):
        """Returns the availability of the weather model in hours."""
        return self._time_res

    def getLLRes(self):
        """Returns the grid spacing."""
        return np.max([self._lat_res, self._lon_res])

    def getProjection(self):
        return self._proj

    # -- weatherModel.py:171-184 -----------------------------------------------------------------------------------------
    def getTime(self):
        return self._time

    def setTime(self, time, fmt='%Y-%m-%dT%H:%M:%S'):
        """The model time: a datetime, or a string in `fmt`; a time without a zone is taken as UTC."""
        when = dt.datetime.strptime(time, fmt) if isinstance(time, str) else time
        if not isinstance(when, dt.datetime):
            raise ValueError('"time" must be a string or a datetime object')
        self._time = when if when.tzinfo is not None else when.replace(tzinfo=_UTC)
        self._bbox = None                          # (the extent is read off the processed file of THIS time)

    def setLevelType(self, levelType):
        """weatherModel.py:310-320, without the level tables (raider_amd.weather ships those)."""
        if levelType not in 'ml pl nat prs'.split():
            raise RuntimeError(f'Level type {levelType} is not recognized')
        if levelType in ('pl', 'prs'):
            if self._key == 'ERAI':
                raise RuntimeError('ERA-I does not use pressure levels, you need to use model levels')             # erai.py:31-32
            if self._key in ('HRRR', 'HRRRAK'):
                raise NotImplementedError('Pressure levels do not go high enough for HRRR.')                       # hrrr.py:267-268
        self._model_level_type = levelType

    # -- weatherModel.py:186-232 -----------------------------------------------------------------------------------------
    def get_latlon_bounds(self):
        """Returns the bounds of the weather model."""
        return self._ll_bounds

    def set_latlon_bounds(self, ll_bounds, Nextra=2, output_spacing=None):
        """weatherModel.py:190-220: the SNWE box to ask the provider for.  `Nextra` model cells are added on every side - six for
        HRRR, HRRR-AK and HRES, whatever is passed; the other models add one more cell of longitude - and every side keeps that same
        margin from the poles and the date line; with `output_spacing` the box is then clipped outwards to its multiples.  (The
        order of the additions is the reference's: the results are compared with its own bit for bit, golden g18.)"""
        from .utilFcns import clip_bbox
        wide = self._Name in ('HRRR', 'HRRR-AK', 'HRES')
        cells = 6 if wide else Nextra
        more_lon = 0.0 if wide else self._lon_res
        dlat, dlon = cells * self._lat_res, cells * self._lon_res
        south, north, west, east = ll_bounds
        box = [np.max([south - dlat, -90.0 + dlat]), np.min([north + dlat, 90.0 - dlat]),
               np.max([west - (dlon + more_lon), -180.0 + (dlon + more_lon)]), np.min([east + (dlon + more_lon), 180.0 - dlon - more_lon])]
        self._ll_bounds = np.array(box if output_spacing is None else clip_bbox(box, output_spacing))

    def get_wmLoc(self):
        """Get the path to the directory with the weather model files."""
        return os.path.join(os.getcwd(), 'weather_files') if self._wmLoc is None else self._wmLoc

    def set_wmLoc(self, weather_model_directory):
        """Set the path to the directory with the weather model files."""
        self._wmLoc = weather_model_directory

    # -- weatherModel.py:278-308 -----------------------------------------------------------------------------------------
    def checkTime(self, time):
        """DatetimeOutsideRange unless `time` lies in the model's valid range and is older than its availability lag."""
        if not isinstance(time, dt.datetime):
            raise ValueError(f'"time" should be a Python datetime object, instead it is {time}')
        first, last = self._valid_range
        logger.info('Weather model %s is available from %s to %s', self.Model(), first, last)
        when = time.replace(tzinfo=_UTC)                      # (naive and aware datetimes do not compare)
        newest = dt.datetime.now(dt.timezone.utc) - self._lag_time
        if when < first or when > last or when > newest:
            raise DatetimeOutsideRange(self.Model(), when)

    # -- weatherModel.py:631-657 -----------------------------------------------------------------------------------------
    def out_file(self, outLoc):
        """The processed (cropped) model file of the model's time and bounds."""
        return os.path.join(outLoc, make_weather_model_filename(self._Name, self._time, self._ll_bounds))

    # -- weatherModel.py:418-531 -----------------------------------------------------------------------------------------
    @property
    def bbox(self):
        """(xmin, ymin, xmax, ymax) of the processed model file in lon / lat (weatherModel.py:418-456): the extremes of its x and y
        axes, for a projected model the four corners taken back to lon / lat.  ValueError when the file does not exist."""
        if self._bbox is None:
            path = self.out_file(self.get_wmLoc())
            if not Path(path).exists():
                raise ValueError('Need to save cropped weather model as netcdf')
            self._bbox = file_bbox(path, self._proj)
        return self._bbox

    def checkValidBounds(self, ll_bounds):
        """weatherModel.py:458-471: ValueError unless the SNWE box (or the box moved by 360 degrees) meets the model's domain - the
        whole globe for the lon / lat models.  HRRR: models/hrrr.py:323-356 on the grid's own extent (see the module text)."""
        S, N, W, E = ll_bounds
        if self._key in ('HRRR', 'HRRRAK'):
            return self._check_valid_bounds_hrrr(S, N, W, E)
        world = (-180, -90, 180, 90)
        if not _boxes_meet((W, S, E, N), world):
            if not _boxes_meet((360 + W, S, 360 + E, N), world):
                raise ValueError(f'The requested location is unavailable for {self._Name}')

    def _check_valid_bounds_hrrr(self, S, N, W, E):
        cover = grid_coverage(self._Name, (S, N, W, E))
        if cover == 'inside':
            return
        if cover == 'partial':
            logger.critical(f'The {self._Name} weather model extent does not completely cover your AOI!')
            return
        if self._key == 'HRRRAK':
            raise ValueError(f'The requested location is unavailable for {self._Name}')
        logger.info('The HRRR weather model extent does not include your AOI!')
        logger.info('Checking the HRRR-AK model.')
        cover = grid_coverage('HRRR-AK', (S, N, W, E))
        if cover == 'outside':
            raise ValueError('The requested location is unavailable for HRRR')
        self._cast_to_hrrrak()
        logger.info('Casting self to the HRRR-AK weather model.')
        if cover == 'partial':
            logger.critical('The HRRR-AK weather model extent does not completely cover your AOI!')

    def _cast_to_hrrrak(self):
        """hrrr.py:284-298: the model becomes HRRR-AK (name, data set, projection, time step, valid range)."""
        self._set_facts('HRRRAK')

    def checkContainment(self, ll_bounds, buffer_deg=1e-5):
        """weatherModel.py:473-531: True when the processed model file covers the SNWE box `ll_bounds`.  A model extent that leaves
        the world box is taken together with its copies moved by +-360 degrees, each grown by `buffer_deg`; a model that covers the
        whole world covers everything.  (Boxes only, so interval arithmetic serves where the reference builds shapely polygons; the
        rounded corners shapely gives a grown box are left square: they lie within buffer_deg of the model's own corner.)"""
        ymin_input, ymax_input, xmin_input, xmax_input = ll_bounds
        xmin, ymin, xmax, ymax = self.bbox
        logger.info('Extent of the weather model is (xmin, ymin, xmax, ymax):' + ', '.join(f'{x:1.2f}' for x in (xmin, ymin, xmax, ymax)))
        logger.info('Extent of the input is (xmin, ymin, xmax, ymax): ' + ', '.join(f'{x:1.2f}' for x in (xmin_input, ymin_input, xmax_input, ymax_input)))
        covered, world = box_containment((xmin, ymin, xmax, ymax), (xmin_input, ymin_input, xmax_input, ymax_input), buffer_deg)
        if world:
            # (the reference assigns to its read-only `bbox` property here, weatherModel.py:525, which cannot succeed; what that line
            # means to do is done)
            self._bbox = (-180, -90, 180, 90)
            return True
        return covered


# ---- the six model names as the reference's classes are called ----------------------------------------------------------------
def _named(key):
    def make():
        return WeatherModel(key)
    make.__name__ = key
    make.__doc__ = f'The {_FACTS[key][0]} weather model (models/{key.lower()}.py).'
    return make


ERA5, ERA5T, ERAI, HRES, GMAO, MERRA2, HRRR, HRRRAK, NCMR = (_named(k) for k in ('ERA5', 'ERA5T', 'ERAI', 'HRES', 'GMAO', 'MERRA2', 'HRRR',
                                                                                  'HRRRAK', 'NCMR'))


def parse_weather_model(weather_model_name, aoi):
    """validators.py:38-51: the model of a configuration's `weather_model`, checked against the AOI's bounds."""
    weather_model_name = weather_model_name.upper().replace('-', '')
    if weather_model_name not in _PARSEABLE:
        raise NotImplementedError(f'Model {weather_model_name} is not yet fully implemented, please contribute!')
    model = WeatherModel(weather_model_name)
    model.checkValidBounds(aoi.bounds())
    return model


# ---- file names (weatherModel.py:727-747) -------------------------------------------------------------------------------------
def _edge(value, outwards, negative, positive):
    """One edge of a bounds tag: the bound rounded outwards to a whole degree, with its hemisphere letter."""
    whole = outwards(value)
    return f'{np.abs(whole):.0f}{negative}' if whole < 0 else f'{whole:.0f}{positive}'


def make_weather_model_filename(name, time, ll_bounds):
    """weatherModel.py:727-740: `<name>_<time>_<S>_<N>_<W>_<E>.nc`, e.g. ERA-5_2020_01_30_T13_52_45_32N_35N_120W_115W.nc."""
    south, north, west, east = ll_bounds[:4]
    tag = '_'.join([_edge(south, np.floor, 'S', 'N'), _edge(north, np.ceil, 'S', 'N'), _edge(west, np.floor, 'W', 'E'), _edge(east, np.ceil, 'W', 'E')])
    return f'{name}_{time.strftime("%Y_%m_%d_T%H_%M_%S")}_{tag}.nc'


def make_raw_weather_data_filename(outLoc, name, time):
    """Filename generator for the raw downloaded weather model data."""
    return os.path.join(outLoc, f'{name}_{dt.datetime.strftime(time, "%Y_%m_%d_T%H_%M_%S")}.nc')


# ---- boxes -------------------------------------------------------------------------------------------------------------------
def _boxes_meet(a, b):
    """Two closed (xmin, ymin, xmax, ymax) boxes share at least a point (shapely's `intersects` on boxes)."""
    return a[0] <= b[2] and b[0] <= a[2] and a[1] <= b[3] and b[1] <= a[3]


def _box_in(inner, outer):
    return outer[0] <= inner[0] and inner[2] <= outer[2] and outer[1] <= inner[1] and inner[3] <= outer[3]


def box_containment(model_box, input_box, buffer_deg=1e-5):
    """The geometry of weatherModel.py:510-531 on (xmin, ymin, xmax, ymax) boxes: (the model covers the input box, the model covers
    the whole world)."""
    world = (-180, -90, 180, 90)
    xmin, ymin, xmax, ymax = model_box
    if _box_in(model_box, world):
        return _box_in(input_box, model_box), _box_in(world, model_box)
    logger.info('Considering x-translates of weather model +/-360 as bounding box outside of -180, -90, 180, 90')
    # the union of the three grown copies: they share their y interval, so the union is that interval times the union of the three x
    # intervals, merged where they touch
    ylo, yhi = ymin - buffer_deg, ymax + buffer_deg
    spans = []
    for off in (-360, 0, 360):
        lo, hi = xmin + off - buffer_deg, xmax + off + buffer_deg
        if spans and lo <= spans[-1][1]:
            spans[-1][1] = max(spans[-1][1], hi)
        else:
            spans.append([lo, hi])
    inside = lambda b: ylo <= b[1] and b[3] <= yhi and any(lo <= b[0] and b[2] <= hi for lo, hi in spans)
    return inside(input_box), inside(world)


def file_bbox(path, proj=4326):
    """(W, S, E, N) of a processed model file in lon / lat: the extremes of `x` / `y` (or `longitude` / `latitude`), for a projected
    model the lon / lat of the four corners (weatherModel.py:438-454)."""
    from .delay import _builtin_crs
    from .delayFcns import _read_cube_file
    var = _read_cube_file(path)
    try:
        xs, ys = np.asarray(var['x'][:], dtype=np.float64), np.asarray(var['y'][:], dtype=np.float64)
    except KeyError:
        xs, ys = np.asarray(var['longitude'][:], dtype=np.float64), np.asarray(var['latitude'][:], dtype=np.float64)
    xmin, xmax, ymin, ymax = xs.min(), xs.max(), ys.min(), ys.max()
    kind = _builtin_crs(proj)
    lons, lats = np.array([xmin, xmin, xmax, xmax]), np.array([ymin, ymax, ymin, ymax])
    if kind is not None and kind[0] == 'cone':
        from .utilFcns import conic
        lats, lons = conic(lats, lons, kind[1], inverse=True)
    elif kind is None or kind[0] != 'geodetic':
        raise NotImplementedError(f'no lon / lat extent for a model in the CRS {proj!r}')
    return float(np.min(lons)), float(np.min(lats)), float(np.max(lons)), float(np.max(lats))


def grid_extent(name):
    """(xmin, ymin, xmax, ymax) in metres of the HRRR / HRRR-AK grid in its own projection: the first node projected, plus
    (nodes - 1) spacings."""
    from .delay import _builtin_crs
    from .utilFcns import conic
    lat1, lon1, nx, ny, d = _GRIDS[name]
    params = _builtin_crs(_HRRR_PROJ if name == 'HRRR' else _HRRRAK_PROJ)[1]
    y0, x0 = conic(np.array([lat1]), np.array([lon1]), params)
    return float(x0[0]), float(y0[0]), float(x0[0]) + (nx - 1) * d, float(y0[0]) + (ny - 1) * d


def grid_coverage(name, snwe, n=21):
    """'inside', 'partial' or 'outside': how the HRRR / HRRR-AK grid covers the SNWE box.  An n x n mesh over the box goes through the
    model's projection and is held against the grid's extent; a box no mesh node of which falls on the grid may still hold the grid,
    so the grid's edge goes back to lon / lat and is held against the box."""
    from .delay import _builtin_crs
    from .utilFcns import conic
    S, N, W, E = (float(v) for v in snwe)
    params = _builtin_crs(_HRRR_PROJ if name == 'HRRR' else _HRRRAK_PROJ)[1]
    xmin, ymin, xmax, ymax = grid_extent(name)
    lon, lat = np.meshgrid(np.linspace(W, E, n), np.linspace(S, N, n))
    y, x = conic(lat, lon, params)
    on = (x >= xmin) & (x <= xmax) & (y >= ymin) & (y <= ymax)
    if on.all():
        return 'inside'
    if on.any():
        return 'partial'
    ex, ey = np.linspace(xmin, xmax, n), np.linspace(ymin, ymax, n)
    px = np.concatenate([ex, ex, np.full(n, xmin), np.full(n, xmax)])
    py = np.concatenate([np.full(n, ymin), np.full(n, ymax), ey, ey])
    glat, glon = conic(py, px, params, inverse=True)
    in_lon = np.mod(glon - W, 360.0) <= E - W if E - W < 360 else np.ones(glon.shape, dtype=bool)   # (the box may be given in 0..360)
    return 'partial' if np.any((glat >= S) & (glat <= N) & in_lon) else 'outside'
