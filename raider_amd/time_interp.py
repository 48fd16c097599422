"""Temporal interpolation of weather models, as calcDelays does it per date (mirror of tools/RAiDER/cli/raider.py:282-343,
725-916 and the time helpers of tools/RAiDER/utilFcns.py:307-339, 419-428, 871-925).

The date loop of cli/raider.py:159-400 does three things per acquisition date: it picks the model times around the acquisition
(``interpolate_time``: 'none', 'center_time' - what every template YAML of the reference ships - or 'azimuth_time_grid', the HRRR /
GUNW workflow), it combines the model files that came back (``getWeatherFile`` / ``combine_weather_files``) and it calls
``tropo_delay`` on the result.  ``tropo_delay_interp`` / ``tropo_delay_interp_series`` are that loop; the model files of a date are
looked up in a mapping {model datetime: file or model} instead of being downloaded (download and ``prepareWeatherModel`` are I/O and
stay with the caller).

The combination runs on the device: 'center_time' is ``Cube.blend`` on both cube pairs; 'azimuth_time_grid' is ONE kernel from the
orbit to the combined cubes (``s1_azimuth_timing.combine_cubes_azimuth_time``, rdr_cube_blend_azimuth_time) when the orbit's state
vectors fit its LDS tables, the staged chain of ``s1_azimuth_timing`` otherwise.
"""
import datetime as dt
import os
from pathlib import Path

import numpy as np

from .logger import logger

_THRESHOLD_SECONDS = 1 * 60          # constants.py:23: closer than this to a model time, that one model time is used
EXPECTED_NUM_FILES = {'none': 1, 'center_time': 2, 'azimuth_time_grid': 3}          # cli/raider.py:740
STYLE = {'center_time': '_timeInterp_', 'azimuth_time_grid': '_timeInterpAziGrid_'}  # cli/raider.py:794
AZ_TIME_ALLOWED_MODELS = 'hrrr hrrrak hrrr-ak'.split()                               # cli/raider.py:897


# ---- models/customExceptions.py ------------------------------------------------------------------------------------------
class DatetimeFailed(Exception):
    def __init__(self, model, time):
        super().__init__(f'Weather model {model} failed to download for datetime {time}')


class WrongNumberOfFiles(Exception):
    def __init__(self, Nexp, Navail):
        # (customExceptions.py:40-44: the second line of the message is a statement of its own there, so it never reaches the text)
        super().__init__('The number of files downloaded does not match the requested, ')


class NoWeatherModelData(Exception):
    def __init__(self, custom_msg=None):
        super().__init__('No weather model files were available to download, aborting' if custom_msg is None else custom_msg)


# ---- utilFcns.py time helpers --------------------------------------------------------------------------------------------
def get_dt(t1, t2):
    """utilFcns.py:907-925: absolute difference in seconds between two datetimes."""
    return np.abs((t1 - t2).total_seconds())


def round_date(date, precision):
    """utilFcns.py:307-339: `date` rounded to the nearest multiple of the timedelta `precision`; a tie rounds down."""
    T0 = dt.datetime.min
    try:
        datedelta = T0 - date
    except TypeError:
        T0 = T0.replace(tzinfo=dt.timezone(offset=dt.timedelta()))
        datedelta = T0 - date
    round_up = date + datedelta % precision
    round_down = date - (date - T0) % precision
    return round_up if (round_up - date) < (date - round_down) else round_down


def round_time(datetime, roundTo=60):
    """utilFcns.py:419-428: `datetime` rounded to the closest `roundTo` seconds of its day; a tie rounds up."""
    seconds = (datetime.replace(tzinfo=None) - datetime.min).seconds
    rounding = (seconds + roundTo / 2) // roundTo * roundTo
    return datetime + dt.timedelta(0, rounding - seconds, -datetime.microsecond)


def get_nearest_wmtimes(t0, time_delta):
    """utilFcns.py:871-904: the one or two model times (step `time_delta` hours) closest to t0, in time order; one when t0 lies
    within _THRESHOLD_SECONDS of a model time.

    >>> get_nearest_wmtimes(dt.datetime(2020, 1, 1, 11, 35, 0), 3)
    [datetime.datetime(2020, 1, 1, 9, 0), datetime.datetime(2020, 1, 1, 12, 0)]
    """
    tclose = round_time(t0, roundTo=time_delta * 60 * 60)
    t2_1 = tclose + dt.timedelta(hours=time_delta)
    t2_2 = tclose - dt.timedelta(hours=time_delta)
    t2 = t2_1 if get_dt(t2_1, t0) < get_dt(t2_2, t0) else t2_2
    if get_dt(tclose, t0) < _THRESHOLD_SECONDS:
        return [tclose]
    return [tclose, t2] if t2 > tclose else [t2, tclose]


def get_weights_time_interp(times, time):
    """cli/raider.py:877-888: inverse linear weights of the two model times; None (and the reference's log line) when they do not
    sum to one."""
    date1, date2 = times
    wgts = [1 - get_dt(time, date1) / get_dt(date2, date1), 1 - get_dt(date2, time) / get_dt(date2, date1)]
    try:
        assert np.isclose(np.sum(wgts), 1)
    except AssertionError:
        logger.error('Time interpolation weights do not sum to one; something is off with query datetime: %s', time)
        return None
    return wgts


# ---- the model files of one date ------------------------------------------------------------------------------------------
def _is_path(f):
    return isinstance(f, (str, os.PathLike))


def _file_datetime(wfile):
    """The `datetime` global attribute of a processed weather-model file (cli/raider.py:800-802)."""
    if not _is_path(wfile):
        attrs = getattr(wfile, 'attrs', None)
        if attrs is not None and 'datetime' in attrs:
            return dt.datetime.strptime(str(attrs['datetime']), '%Y_%m_%dT%H_%M_%S')
        raise ValueError('combine_weather_files: an in-memory weather model carries no `datetime` attribute: pass times=')
    with open(wfile, 'rb') as fh:
        magic = fh.read(4)
    if magic[:3] == b'CDF':
        from scipy.io import netcdf_file
        with netcdf_file(str(wfile), 'r', mmap=False) as f:
            stamp = f.datetime
        stamp = stamp.decode() if isinstance(stamp, bytes) else str(stamp)
    else:
        from . import h5lite
        stamp = h5lite.File(wfile).attrs['datetime']
        stamp = stamp.decode() if isinstance(stamp, bytes) else str(stamp)
    return dt.datetime.strptime(stamp, '%Y_%m_%dT%H_%M_%S')


def _model_cubes(wfile, ctx=None):
    """(pointwise Cube, total Cube, CRS, variables) of a processed-cube path, a ProcessedModel or a mapping tropo_delay accepts."""
    from .delayFcns import _load_fields, getInterpolators
    if hasattr(wfile, 'pointwise') and hasattr(wfile, 'total'):
        return wfile.pointwise, wfile.total, wfile.proj, wfile
    var, _ = _load_fields(wfile)
    try:
        pj = var['proj']
        if isinstance(pj, (str, dict, int)):
            proj = pj
        else:
            from .crs import crs_from_proj_var
            proj = crs_from_proj_var(pj.attrs)
    except (KeyError, AttributeError, TypeError):
        proj = 4326
    src = wfile if _is_path(wfile) else var
    pw = getInterpolators(src, 'pointwise', ctx=ctx)[0].cube
    tot = getInterpolators(src, 'total', ctx=ctx)[0].cube
    return pw, tot, proj, var


def _latlon_2d(cube, proj, var):
    """The 2-D latitude / longitude of a model on its cube's (ascending) axes: read from the file (cli/raider.py:900-901) or made as
    ProcessedModel.to_netcdf makes them."""
    ys, xs, _ = cube.grid
    try:
        lat2, lon2 = np.array(var['latitude'][:], dtype=np.float64), np.array(var['longitude'][:], dtype=np.float64)
        fy, fx = np.asarray(var['y'][:], dtype=np.float64), np.asarray(var['x'][:], dtype=np.float64)
        if fy.size > 1 and fy[0] > fy[-1]:
            lat2, lon2 = lat2[::-1], lon2[::-1]
        if fx.size > 1 and fx[0] > fx[-1]:
            lat2, lon2 = lat2[:, ::-1], lon2[:, ::-1]
        if lat2.shape == (ys.size, xs.size):
            return np.ascontiguousarray(lat2), np.ascontiguousarray(lon2)
    except (KeyError, AttributeError, TypeError, IndexError):
        pass
    from .delay import _builtin_crs
    lon2, lat2 = np.meshgrid(xs, ys)
    kind = _builtin_crs(proj)
    if kind is not None and kind[0] == 'cone':
        from .utilFcns import conic
        lat2, lon2 = conic(lat2, lon2, kind[1], inverse=True)
    elif kind is None or kind[0] != 'geodetic':
        raise NotImplementedError(f'azimuth_time_grid: no geodetic coordinates for the model CRS {proj!r}')
    return np.ascontiguousarray(lat2, dtype=np.float64), np.ascontiguousarray(lon2, dtype=np.float64)


def combined_file_name(first_file, time, interp_method):
    """cli/raider.py:824-830: the name of the combined file beside the first model file."""
    first = Path(first_file)
    return first.parent / (first.name.split('_')[0] + '_' + time.strftime('%Y_%m_%dT%H_%M_%S') + STYLE[interp_method]
                           + '_'.join(first.name.split('_')[-4:]))


def combine_weather_files(wfiles, time, model, interp_method='center_time', orbit=None, write=False, times=None, ctx=None):
    """cli/raider.py:792-835: the weather models `wfiles` (paths of processed cubes, ProcessedModels, or the mappings tropo_delay
    accepts) interpolated to the acquisition `time`.  Returns a weather.ProcessedModel with the combined pointwise and total cubes
    on the device, the first file's axes and CRS, `model_times` (the model datetimes used) and `interpolation_method`; with
    write=True also the file the reference writes (`path`).  The model datetimes come from the files' `datetime` attribute, or from
    `times` (in-memory models).  'azimuth_time_grid' needs `orbit` (an orbits.Orbit, or an orbit file path)."""
    from .weather import ProcessedModel
    if interp_method not in STYLE:
        if interp_method == 'none':
            raise ValueError('Interpolating weather files is not available with interpolation method "none"')
        raise KeyError(interp_method)
    wfiles = list(wfiles)
    times = [_file_datetime(f) for f in wfiles] if times is None else list(times)
    if len(times) == 0:
        raise NoWeatherModelData()
    if len(times) != len(wfiles):
        raise ValueError(f'{len(wfiles)} weather models but {len(times)} model times')
    models = [_model_cubes(f, ctx) for f in wfiles]
    pw0, tot0, proj, var0 = models[0]
    if interp_method == 'center_time':
        wgts = get_weights_time_interp(times, time)
        w1, w2 = wgts                                      # (None - weights off: TypeError, as zip(None, ...) in the reference)
        pointwise = pw0.blend(w1, models[1][0], w2)
        total = tot0.blend(w1, models[1][1], w2)
    else:
        if str(model).lower() not in AZ_TIME_ALLOWED_MODELS:
            raise NotImplementedError('Azimuth Time is currently only implemented for HRRR')
        pointwise, total = _combine_azimuth_time([m[0] for m in models], [m[1] for m in models], times, time, proj, var0, orbit, ctx)
    out = ProcessedModel(pointwise, total, pointwise.grid[2].copy(), proj=proj)
    out.model_times, out.interpolation_method, out.path = list(times), interp_method, None
    if write:
        if not _is_path(wfiles[0]):
            raise ValueError('combine_weather_files(write=True) names the product after the first model FILE: pass paths')
        path = combined_file_name(wfiles[0], time, interp_method)
        out.to_netcdf(path, time=times[0], model_name=str(model), attrs=dict(Date1=0, Date2=0))
        out.path = path
    return out


def _combine_azimuth_time(pw_cubes, tot_cubes, times, time, proj, var0, orbit, ctx):
    from . import _lib as L
    from . import s1_azimuth_timing as S
    from .orbits import Orbit
    if orbit is None:
        raise NotImplementedError('the SLC / orbit-file lookup (asf_search, s1_orbits) needs the network: pass orbit=')
    if not isinstance(orbit, Orbit):
        orbit = Orbit.from_file(orbit, time, pad=600)
    lat2, lon2 = _latlon_2d(pw_cubes[0], proj, var0)
    if orbit.time.size <= L.ORBIT_LDS_MAX_SV:
        pointwise, total, _ = S.combine_cubes_azimuth_time(pw_cubes, tot_cubes, times, lat2, lon2, orbit, ctx=ctx)
        return pointwise, total
    # more state vectors than the kernel's LDS tables hold: the staged chain
    zs = pw_cubes[0].grid[2]
    m, (n, p) = zs.size, lat2.shape
    grid = S.get_azimuth_time_grid(np.broadcast_to(lon2, (m, n, p)), np.broadcast_to(lat2, (m, n, p)),
                                   np.broadcast_to(zs[:, None, None], (m, n, p)), orbit, ctx=ctx)
    return S.combine_weather_cubes_azimuth_time(pw_cubes, tot_cubes, times, grid, ctx=ctx)


def getWeatherFile(wfiles, times, time, model, interp_method='none', orbit=None, file_times=None, write=False):
    """cli/raider.py:726-789: the weather model of one date from the files that came back for the model `times` asked for - the
    file itself, or the combination (a ProcessedModel; `orbit`, `file_times` and `write` go to combine_weather_files); None when
    there is no file."""
    Nfiles = len(wfiles)
    Ntimes = len(times)
    try:
        Nfiles_expected = EXPECTED_NUM_FILES[interp_method]
    except KeyError:
        raise ValueError(f'getWeatherFile: interp_method {interp_method} is not known')
    Nmatch = Nfiles_expected == Nfiles
    Tmatch = Nfiles == Ntimes
    kw = dict(orbit=orbit, times=file_times, write=write)
    if Nfiles == 0:                                                      # Case 1: no files
        logger.error('No weather model data was successfully processed.')
        return None
    if interp_method == 'none':                                          # Case 2
        return wfiles[0]
    if interp_method == 'center_time':
        if Nmatch:                                                       # Case 3: two files
            return combine_weather_files(wfiles, time, model, interp_method='center_time', **kw)
        if Tmatch:                                                       # Case 4: the exact time is available
            logger.warning('Time interpolation is not needed as exact time is available')
            return wfiles[0]
        if Nfiles == 1:                                                  # Case 5: one file is missing
            logger.warning('getWeatherFile: One datetime is not available to download, defaulting to nearest available date')
            return wfiles[0]
        raise WrongNumberOfFiles(Nfiles_expected, Nfiles)
    if Nmatch or Tmatch:                                                 # Case 6: all files
        return combine_weather_files(wfiles, time, model, interp_method='azimuth_time_grid', **kw)
    raise WrongNumberOfFiles(Nfiles_expected, Nfiles)


# ---- the date loop -------------------------------------------------------------------------------------------------------
def model_times_for(datetime, interpolate_time='center_time', time_step_hours=None):
    """cli/raider.py:282-304: the model times one acquisition date asks for."""
    from .s1_azimuth_timing import get_times_for_azimuth_interpolation
    step = 6 if time_step_hours is None else time_step_hours
    if interpolate_time is None:
        interpolate_time = 'none'
    if interpolate_time == 'none':
        return [round_date(datetime, dt.timedelta(hours=step))]          # what the model classes make of `[t]` (e.g. models/hrrr.py:273)
    if interpolate_time == 'center_time':
        return get_nearest_wmtimes(datetime, step)
    if interpolate_time == 'azimuth_time_grid':
        return get_times_for_azimuth_interpolation(datetime, step)
    raise NotImplementedError('Only none, center_time, and azimuth_time_grid are accepted values for interp_method.')


def _weather_model_for(datetime, models, interpolate_time, time_step_hours, model_name, orbit):
    """cli/raider.py:282-343 for one date: (weather model or None, the model times asked for)."""
    method = 'none' if interpolate_time is None else interpolate_time
    times = model_times_for(datetime, method, time_step_hours)
    wfiles, used = [], []
    for tt in times:
        if tt not in models:                                             # a preparation that failed (cli/raider.py:316-320)
            if method in ('azimuth_time_grid', 'none'):
                raise DatetimeFailed(model_name, tt)
            continue
        wfiles.append(models[tt]); used.append(tt)
    if len(wfiles) == 0:
        logger.error('No weather model data was successfully processed.')
        raise NoWeatherModelData('Weather model processing failed for all times')
    return getWeatherFile(wfiles, times, datetime, model_name, method, orbit=orbit, file_times=used), times


def _provenance(result, model_name, times, method):
    """cli/raider.py:378-380 on a cube result"""
    ds, hydro = result
    if hydro is None and ds is not None:
        attrs = dict(model_name=model_name, model_times_used=[t.strftime('%Y%m%dT%H:%M:%S') for t in sorted(times)], interpolation_method=method)
        if hasattr(ds, 'assign_attrs'):
            ds = ds.assign_attrs(**attrs)
        else:
            ds.attrs.update(attrs)
    return ds, hydro


def tropo_delay_interp_series(datetimes, models, aoi, los, height_levels=None, out_proj=4326, zref=None, interpolate_time='center_time',
                              time_step_hours=None, model_name=None, orbit=None):
    """The date loop of cli/raider.py:159-400 with its temporal interpolation: per date the model times are chosen
    (model_times_for), looked up in `models` = {model datetime: processed-cube path / ProcessedModel / mapping}, combined
    (getWeatherFile), and the list of weather models goes to tropo_delay_series (cube AOI) or tropo_delay_point_series (points AOI)
    unchanged - dates whose combined cubes share a grid take the stacked routes those offer.  Returns their SeriesResult; an entry
    is None for a date getWeatherFile gives no model for; cube results carry the provenance attributes of cli/raider.py:378-380."""
    from .delay import SeriesResult, _is_cube_aoi, tropo_delay_point_series, tropo_delay_series
    method = 'none' if interpolate_time is None else interpolate_time
    datetimes = list(datetimes)
    picked = [_weather_model_for(t, models, method, time_step_hours, model_name, orbit) for t in datetimes]
    keep = [i for i, (wm, _) in enumerate(picked) if wm is not None]
    series = tropo_delay_series if _is_cube_aoi(aoi) else tropo_delay_point_series
    got = series([datetimes[i] for i in keep], [picked[i][0] for i in keep], aoi, los, height_levels, out_proj, zref) if keep else SeriesResult()
    res = SeriesResult([None] * len(datetimes))
    routes = [None] * len(datetimes)
    for k, i in enumerate(keep):
        res[i] = _provenance(got[k], model_name, picked[i][1], method)
        routes[i] = got.routes[k]
    res.routes = routes
    return res


def tropo_delay_interp(datetime, models, aoi, los, height_levels=None, out_proj=4326, zref=None, interpolate_time='center_time',
                       time_step_hours=None, model_name=None, orbit=None):
    """One date of tropo_delay_interp_series: what tropo_delay returns on the weather model interpolated to `datetime`."""
    from .delay import tropo_delay
    method = 'none' if interpolate_time is None else interpolate_time
    wm, times = _weather_model_for(datetime, models, method, time_step_hours, model_name, orbit)
    if wm is None:
        return None
    return _provenance(tropo_delay(datetime, wm, aoi, los, height_levels, out_proj, zref), model_name, times, method)
