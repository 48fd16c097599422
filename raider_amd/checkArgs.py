"""checkArgs: a parsed run configuration made ready to run - directories, datetimes, the line of sight's time, output file names.

The counterpart of tools/RAiDER/checkArgs.py:21-133: the same function names, file names, warning and error texts (golden g18).
"""
import datetime as dt

from .llreader import BoundingBox, StationFile
from .logger import logger
from .losreader import Zenith

# What get_raster_ext answers: the reference inverts rasterio's {extension: driver} table (checkArgs.py:99-110), so a driver with
# several extensions gets the one listed last - `tiff`, not `tif`, for GTiff: the name its own test reads the raster from
# (test/test_intersect.py:56, `..._ztd.tiff`).  Held here for the formats writeDelays can write: GTiff through raider_amd.tifflite,
# ENVI / ISCE as flat binary with a header.
_RASTER_EXT = {'GTIFF': 'tiff', 'ENVI': '.dat', 'ISCE': '.dat'}
_CUBE_FORMATS = ('.nc', '.h5', 'h5', 'hdf5', '.hdf5', 'nc')          # checkArgs.py:76


def _station_copy(aoi, path):
    """The station file goes to the output directory, one row per (Lat, Lon); writeDelays adds the delay columns to that copy."""
    import pandas as pd
    pd.read_csv(aoi._filename).drop_duplicates(subset=['Lat', 'Lon']).to_csv(path, index=False)


def _cube_ext(file_format):
    """`nc` or `h5` for a delay cube; any format that is neither NetCDF nor HDF5 (the default GTiff too) means `nc`."""
    if file_format in _CUBE_FORMATS:
        return file_format.strip('.').replace('df', '')
    logger.debug('Invalid extension %s for cube. Defaulting to .nc', file_format)
    return 'nc'


def _names_for(d, run_config):
    """(wet file name, hydro file name) of one datetime: a station AOI has one CSV (and an empty hydro name), a bounding box a cube,
    everything else a pair of rasters."""
    rt, aoi = run_config.runtime_group, run_config.aoi_group.aoi
    dataset = run_config.weather_model._dataset.upper()
    if isinstance(aoi, StationFile):
        csv = str(rt.output_directory / f'{dataset}_Delay_{d:%Y%m%dT%H%M%S}_ztd.csv')
        _station_copy(aoi, csv)
        return csv, ''
    ext = _cube_ext(rt.file_format) if isinstance(aoi, BoundingBox) else get_raster_ext(rt.file_format)
    return makeDelayFileNames(d, run_config.los_group.los, ext, dataset, rt.output_directory)


def checkArgs(run_config):
    """checkArgs.py:21-96: make the two directories and tell the model where its files are; turn the dates into datetimes at the
    acquisition time; warn that one orbit file serves every date; give the line of sight the first datetime; name the outputs."""
    rt = run_config.runtime_group
    for directory in (rt.output_directory, rt.weather_model_directory):
        directory.mkdir(exist_ok=True)
    run_config.weather_model.set_wmLoc(str(rt.weather_model_directory))

    when = run_config.time_group.time
    datetimes = run_config.date_group.date_list = [dt.datetime.combine(day, when) for day in run_config.date_group.date_list]
    if run_config.los_group.orbit_file is not None and len(datetimes) > 1:
        logger.warning('Only one orbit file is being used to get the look vectors for all requested times. If you want to use '
                       'separate orbit files you will need to run RAiDER separately for each time.')
    run_config.los_group.los.setTime(datetimes[0])

    names = [_names_for(d, run_config) for d in datetimes]
    run_config.wetFilenames = [wet for wet, _ in names]
    run_config.hydroFilenames = [hydro for _, hydro in names]
    return run_config


def get_raster_ext(fmt):
    """checkArgs.py:99-110: the file extension of a raster format; ValueError for one that cannot be written."""
    ext = _RASTER_EXT.get(fmt.upper())
    if ext is None:
        raise ValueError(f'{fmt} is not a valid gdal/rasterio file format for rasters')
    return ext


def makeDelayFileNames(date, los, outformat, weather_model_name, out):
    """checkArgs.py:113-133: names for the wet and hydrostatic delays: `<model>_{wet,hydro}_[<date>_]{ztd,std}.<ext>` under `out`,
    `ztd` for a zenith (or no) line of sight.

    >>> from pathlib import Path
    >>> makeDelayFileNames(dt.datetime(2020, 1, 1, 0, 0, 0), None, "h5", "model_name", Path("some_dir"))
    ('some_dir/model_name_wet_20200101T000000_ztd.h5', 'some_dir/model_name_hydro_20200101T000000_ztd.h5')
    >>> makeDelayFileNames(None, None, "h5", "model_name", Path("some_dir"))
    ('some_dir/model_name_wet_ztd.h5', 'some_dir/model_name_hydro_ztd.h5')
    """
    stamp = '' if date is None else f'{date:%Y%m%dT%H%M%S}_'
    kind = 'ztd' if los is None or isinstance(los, Zenith) else 'std'
    return tuple(str(out / f'{weather_model_name}_{part}_{stamp}{kind}.{outformat}') for part in ('wet', 'hydro'))
