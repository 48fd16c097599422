"""prepareWeatherModel: the processed weather-model file of one model time, from what is on disk.

The counterpart of tools/RAiDER/processWM.py:23-134 with every outcome that needs no download.  The reference looks for the
processed (cropped) file, then for the raw file, then fetches; here the third step raises WeatherModelFileNotFound - which the
driver treats as the reference treats a failed preparation (cli/raider.py:316-330).  A raw ECMWF model-level or pressure-level
file (ERA-5, ERA-5T, ERA-I, HRES) is processed - the producer on the device - and written as the reference writes it.
"""
import os

import numpy as np

from .logger import logger
from .models import DatetimeOutsideRange, ExistingWeatherModelTooSmall, make_raw_weather_data_filename  # noqa: F401 (re-exported)

_ECMWF = ('ERA5', 'ERA5T', 'ERAI', 'HRES')
_PROJECTED = 'HRRR HRRR-AK'.split()           # (the reference lists the class names `HRRR HRRRAK` against Model(), processWM.py:92, so
#                                               HRRR-AK never matches there; both projected models are meant, and both are exempt here)


class TryToKeepGoingError(Exception):
    """models/customExceptions.py:25-31."""

    def __init__(self, date=None):
        super().__init__('I will try to keep going' if date is None else
                         f'The weather model does not exist for date {date}, so I will try to use the closest available date.')


class CriticalError(Exception):
    """models/customExceptions.py:34-37."""

    def __init__(self):
        super().__init__('I have experienced a critical error, please take a look at the log files')


class WeatherModelFileNotFound(FileNotFoundError):
    """Neither the processed nor the raw file of a model time is on disk, and nothing is downloaded here."""

    def __init__(self, model, time, processed, raw):
        self.processed, self.raw = str(processed), str(raw)
        super().__init__(f'Weather model {model} for {time}: neither the processed file {self.processed} nor the raw file {self.raw} '
                         'exists, and this package downloads nothing - put one of them there')


# ---- a raw file -> a processed model -----------------------------------------------------------------------------------------
def ecmwf_model_levels_float32(z_surf, lnsp, t, q, lats, a, b, R_d=287.06, g0=9.80665):
    """weather.ecmwf_model_levels in the REFERENCE's precision, on the host: utilFcns.calcgeoh (:781-859) and geo_to_ht (:378-410) as
    the reference really runs them on a raw file - float32 arrays decoded from the packed file meeting Python-float constants, so
    every operation rounds to float32.  That evaluation loses 3-4 digits in log(P1) - log(P0) and lands metres from the float64 one
    of the device kernel (which prefers float64 for that reason) - but a processed file that stands in for one the real
    RAiDER writes from the same raw file has to carry the reference's round-off, not a better one.  It is also as platform
    dependent as the reference itself: a NumPy / libm whose float32 log or exp differs in the last bit moves a height by
    centimetres and the resampled fields by ~1e-6 relative (what _CHAIN_TOL of tests/test_ref_files.py allows for).
    A sweep over the levels of NumPy operations on (ny, nx) arrays, a few milliseconds for a raw file; everything downstream - the
    producer - runs on the device.  Arguments and layout as weather.ecmwf_model_levels: t, q (nlev, ny, nx) with level 1 = model
    top; returns (p, zs), (ny, nx, nlev) float32 with the bottom level first."""
    f = np.float32
    t, q, z_surf, lnsp = (np.asarray(v, dtype=f) for v in (t, q, z_surf, lnsp))
    nlev = t.shape[0]
    if len(a) != nlev + 1 or len(b) != nlev + 1:
        raise ValueError(f'I have here a model with {nlev} levels, but parameters a and b have lengths {len(a)} and {len(b)} '
                         'respectively. Of course, these three numbers should be equal.')                   # utilFcns.py:813-817
    a, b = [f(v) for v in a], [f(v) for v in b]
    surface_p = np.exp(lnsp)
    pressure, geopotential_height = np.empty_like(t), np.empty_like(t)
    below = f(0)                                       # geopotential (less the surface's) at the half level under the current level
    for lev in range(nlev, 0, -1):                     # from the surface (level nlev) up to the model top (level 1)
        k = lev - 1
        p_top, p_bottom = a[k] + b[k] * surface_p, a[lev] + b[lev] * surface_p
        pressure[k] = p_top
        if lev == 1:
            dlogp, alpha = np.log(p_bottom / f(0.1)), f(np.log(2))
        else:
            dlogp = np.log(p_bottom) - np.log(p_top)
            alpha = 1 - (p_top / (p_bottom - p_top)) * dlogp
        rt_moist = t[k] * (1 + f(0.609133) * q[k]) * f(R_d)
        geopotential_height[k] = (below + rt_moist * alpha + z_surf) / f(g0)
        below = below + rt_moist * dlogp
    gh = geopotential_height.transpose(1, 2, 0)
    lat = np.broadcast_to(np.asarray(lats, dtype=f)[:, None, None], gh.shape)
    cos2 = np.cos(np.radians(2 * lat))
    gravity = f(9.80616) * (1 - f(0.002637) * cos2 + f(0.0000059) * cos2 ** 2)                              # _get_g_ll
    radius = np.sqrt(1 / (np.cos(np.radians(lat)) ** 2 / f(6378137 ** 2) + np.sin(np.radians(lat)) ** 2 / f(6356752 ** 2)))   # get_Re
    height = (gh * radius) / (gravity / f(g0) * radius - gh)
    assert height.dtype == f and pressure.dtype == f
    return np.ascontiguousarray(np.flip(pressure.transpose(1, 2, 0), axis=2)), np.ascontiguousarray(np.flip(height, axis=2))


def load_model_levels_as_the_reference(path, ll_bounds=None):
    """weather.load_ecmwf_model_levels with the level pressures and heights of ecmwf_model_levels_float32: the raw model-level file
    cut to `ll_bounds` (ECMWF._makeDataCubes, models/ecmwf.py:305-335) -> weather.ProcessedModel with t, p, e."""
    from . import weather
    raw = weather.read_ecmwf_model_level_file(path, ll_bounds)
    tab = weather.ecmwf_l137()
    p, zs = ecmwf_model_levels_float32(raw['z'], raw['lnsp'], raw['t'], raw['q'], raw['lats'], tab['a'], tab['b'])
    bottom_first = lambda v: np.ascontiguousarray(np.flip(v.transpose(1, 2, 0), axis=2), dtype=np.float64)          # ecmwf.py:98-106
    return weather.cubes_from_model_levels(raw['lons'].astype(np.float64), raw['lats'].astype(np.float64), zs, p, bottom_first(raw['t']),
                                           bottom_first(raw['q']), 'q', new_z=np.flipud(tab['level_heights']), return_state=True)


def load_raw_model(weather_model, path_wm_raw, ll_bounds):
    """WeatherModel.load (weatherModel.py:235-261) of a raw file: -> weather.ProcessedModel with t, p, e.  Model-level files are cut
    to the model's bounds and get the reference's float32 level heights (load_model_levels_as_the_reference); pressure-level files
    are taken whole, as ECMWF._load_pressure_level takes them (:252-303).  Raw files of the other providers (GRIB2 through herbie,
    OPeNDAP subsets) have no sample to build a reader against and raise."""
    from . import weather
    if weather_model._key not in _ECMWF:
        raise NotImplementedError(f'raw {weather_model.Model()} files are not read here (ERA-5, ERA-5T, ERA-I and HRES model-level or '
                                  f'pressure-level files are): process {path_wm_raw} with the reference, or give the processed file')
    if weather_model._model_level_type in ('pl', 'prs'):
        return weather.load_ecmwf_pressure_levels(path_wm_raw, return_state=True)
    return load_model_levels_as_the_reference(path_wm_raw, ll_bounds)


# ---- one model time ----------------------------------------------------------------------------------------------------------
def _covers(weather_model, ll_bounds):
    """The processed file of the model's time must hold the AOI; the projected models are let through (processWM.py:91-93,131-132)."""
    if not weather_model.checkContainment(ll_bounds) and weather_model.Model() not in _PROJECTED:
        raise ExistingWeatherModelTooSmall


def _process_raw(weather_model, path_wm_raw, path_wm_crop, ll_bounds):
    """Raw file -> processed file on disk, checked against the AOI.  A failure to write or to read back is a CriticalError."""
    model = load_raw_model(weather_model, path_wm_raw, weather_model.get_latlon_bounds())
    ys, xs, zs = model.pointwise.grid
    logger.debug('Weather model: %s', weather_model.Model())
    logger.debug('Number of weather model nodes: %s', ys.size * xs.size * zs.size)
    logger.debug(f'Shape of weather model: {(ys.size, xs.size, zs.size)}')
    logger.debug('Bounds of the weather model: %.2f/%.2f/%.2f/%.2f (SNWE)', ys.min(), ys.max(), xs.min(), xs.max())
    try:
        written = model.to_netcdf(path_wm_crop, time=weather_model.getTime(), model_name=weather_model.Model())
        covered = weather_model.checkContainment(ll_bounds)
    except Exception as e:
        logger.exception('Unable to save weathermodel to file')
        logger.exception(e)
        raise CriticalError
    if not covered and weather_model.Model() not in _PROJECTED:
        raise ExistingWeatherModelTooSmall
    return written


def prepareWeatherModel(weather_model, time, ll_bounds, download_only=False, makePlots=False, force_download=False):
    """processWM.py:23-134: the path of the processed weather-model file for `time`, which holds the SNWE box `ll_bounds`.

    The processed file exists: it is used (ExistingWeatherModelTooSmall when it does not hold `ll_bounds`, except for the projected
    models).  The raw file exists: it is processed, written and checked in the same way.  Neither: TryToKeepGoingError for a time
    outside the model's range (what a fetch would find, weatherModel.py:156), else WeatherModelFileNotFound.  With `download_only`
    the answer is None once a file has been found.  `makePlots` is accepted and ignored (the debug plots are not part of this
    package); `force_download` cannot be honoured and raises.
    """
    if force_download:
        raise NotImplementedError('force_download: this package downloads nothing')
    if weather_model.get_latlon_bounds() is None:
        weather_model.set_latlon_bounds(ll_bounds)
    weather_model.setTime(time)
    where = weather_model.get_wmLoc()
    path_wm_crop = weather_model.out_file(where)
    path_wm_raw = make_raw_weather_data_filename(where, weather_model.Model(), time)

    found = next((kind for kind, path in (('processed', path_wm_crop), ('raw', path_wm_raw)) if os.path.exists(path)), None)
    if found is None:
        try:
            weather_model.checkTime(time)
        except DatetimeOutsideRange:
            raise TryToKeepGoingError
        raise WeatherModelFileNotFound(weather_model.Model(), time, path_wm_crop, path_wm_raw)
    # (For a raw file the reference also asks checkContainment_raw, weatherModel.py:791-857, which answers False for every raw file
    # that lies within the world box without covering all of it - and then fetches again.  With no fetch to fall back on the raw file
    # is used, and the containment check of the processed file decides.)
    logger.warning('%s weather model already exists, please remove it ("%s") if you want to download a new one.',
                   'Processed' if found == 'processed' else 'Raw', path_wm_crop if found == 'processed' else path_wm_raw)
    if download_only:
        logger.warning('download_only flag selected. No further processing will happen.')
        return None
    if found == 'raw':
        return _process_raw(weather_model, path_wm_raw, path_wm_crop, ll_bounds)
    logger.warning('The processed weather model file already exists, so I will use that.')
    _covers(weather_model, ll_bounds)
    return path_wm_crop
