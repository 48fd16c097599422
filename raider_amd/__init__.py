"""raider_amd - MI355X-native engine for RAiDER's tropospheric-delay hot path.

Public surface mirrors the reference modules for that path (tools/RAiDER/{delay,delayFcns,losreader,
utilFcns,interpolator}.py and the `interpolate` / `makePoints` extensions); all arithmetic runs in
hand-written HIP kernels behind the C ABI of include/raider_hip.h.  No CPU fallback exists.
"""
__version__ = '0.1.0'

from ._lib import Context, NoLevels, load as load_library  # noqa: F401
from .engine import (Cube, Rays, grid_geodetic, interp_project_epochs, nparts_from_maxlen, point_delays_epochs, raytrace_epochs,  # noqa: F401
                     raytrace_slices_epochs, raytrace_slices_epochs_to_cubes)
from .llreader import AOI, BoundingBox, GeocodedFile, Geocube, RasterRDR, StationFile, bounds_from_csv, bounds_from_latlon_rasters  # noqa: F401
from .time_interp import (DatetimeFailed, NoWeatherModelData, WrongNumberOfFiles, combine_weather_files, get_dt, get_nearest_wmtimes,  # noqa: F401
                          get_weights_time_interp, getWeatherFile, round_date, round_time, tropo_delay_interp, tropo_delay_interp_series)
from .variogram import (GridVariograms, PairVariogram, StationGrid, VariogramFits, deramp, fit_variogram, fit_variograms, grid_variograms, pair_variogram, station_grid,  # noqa: F401
                        station_variograms, utm_common_center)
from .station_stats import (GridStatistics, grid_statistics, load_gridfile, read_station_csv, save_gridfile, station_table)  # noqa: F401
from .seasonal import GridSeasonal, SeasonalFits, grid_seasonal, seasonal_fits  # noqa: F401
