"""Gridded station statistics of `raiderStats` (cli/statsPlot.py, RaiderStats.create_DF :1423-1794) on the device.

The reference reads a long station table (one row per station and time stamp), sends every station to a grid cell and builds seven
maps with two pandas groupby passes each.  Here the table becomes a [D, N] series with NaN = no row (`station_table`,
`read_station_csv`), and ONE device call (rdr_grid_stats, csrc/grid_stats_kernels.h) gives every station's and every cell's count,
mean, median and standard deviation:

  grid_statistics   - the seven maps over the grid of `station_grid`, with the per-station and per-cell arrays behind them
  station_table     - long table -> (ids, lon, lat, when, values [D, N]) with the filters of `_reader` / `create_DF`
  read_station_csv  - the reference's CSV layout -> station_table, through the standard library's csv
  save_gridfile / load_gridfile - the GeoTIFF files of `--grid_to_raster` (:436-541), through tifflite

The seasonal fits and their maps are in seasonal.py.  Not here: the `seasonalinterval` filter, the per-station debug plots, the plots.
"""
import csv
import os
import re

import numpy as np

from . import _lib as L
from ._lib import Context, check, ptr
from .variogram import MAX_DATES, MAX_POINTS, _is_tensor, station_grid

MAPS = ('grid_heatmap', 'grid_delay_mean', 'grid_delay_median', 'grid_delay_stdev', 'grid_delay_absolute_mean', 'grid_delay_absolute_median',
        'grid_delay_absolute_stdev')
_SI = {'mm': 0.001, 'cm': 0.01, 'm': 1.0, 'km': 1000.0, 'mm^2': 1e-6, 'cm^2': 1e-4, 'm^2': 1.0, 'km^2': 1e6}
_TIME_UNITS = ('minute', 'hour', 'day', 'year')


def convert_SI(val, unit_in, unit_out):
    """`convert_SI` (:399-417) for arrays and numbers: val * SI[unit_in] / SI[unit_out]; a time unit as output leaves val as it is."""
    if unit_out in _TIME_UNITS:
        return val
    if unit_out not in _SI:
        raise ValueError(f'User-specified output unit {unit_out} not recognized.')
    return val * _SI[unit_in] / _SI[unit_out]


class GridStatistics:
    """What grid_statistics returns.  grid: the StationGrid (G cells).  Per station, in the CALLER's order [N]: st_nobs (int64), st_mean,
    st_median, st_stdev (NaN / 0 for a station outside the grid).  Per cell [G]: nstations, cell_nobs (int64), mean_of_means,
    mean_of_medians, mean_of_stdevs, abs_mean, abs_median, abs_stdev.  The seven maps [ny, nx], row 0 in the north, named as in the
    reference: grid_heatmap (float, NaN for a cell without a station that has a row), grid_delay_mean / _median / _stdev (the mean over
    the cell's stations of the station statistic), grid_delay_absolute_mean / _median / _stdev (over all rows of the cell).  NumPy arrays
    or GPU tensors, as the inputs were.  medians: False when the three medians were skipped (their arrays and maps are NaN)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def plotbbox(self):
        """[W, E, S, N], the reference's `plotbbox`."""
        return [float(v) for v in self.grid.extent]

    def maps(self):
        """{name: map} of the maps that were computed."""
        skip = () if self.medians else ('grid_delay_median', 'grid_delay_absolute_median')
        return {k: getattr(self, k) for k in MAPS if k not in skip}

    def to_rasters(self, workdir, col_name, unit='m', stationsongrids=False, time_lines=False):
        """`--grid_to_raster`: <workdir>/<col_name>_<map>.tif for every map that was computed, with the dtype, nodata and colour-bar
        format of the reference's call sites (the heatmap int16 with nodata 0 and '%1i', the others float32 with NaN and '%.2f').
        -> {map name: path}."""
        os.makedirs(workdir, exist_ok=True)
        out = {}
        for name, a in self.maps().items():
            a = a.cpu().numpy() if _is_tensor(a) else a
            path = os.path.join(str(workdir), f'{col_name}_{name}.tif')
            kw = dict(colorbarfmt='%1i', dtype='int16', noData=0) if name == 'grid_heatmap' else dict(colorbarfmt='%.2f', dtype='float32')
            save_gridfile(a, name, path, self.plotbbox, self.grid.spacing, unit, stationsongrids=stationsongrids, time_lines=time_lines, **kw)
            out[name] = path
        return out


def grid_statistics(lon, lat, values, spacing=1.0, bbox=None, medians=True, ctx=None):
    """The gridded statistics of `raiderStats` (create_DF, :1571-1794) for stations lon / lat [N] (degrees) and values [D, N] (NaN = no
    row; every other value counts) -> GridStatistics.  lon, lat, values are all NumPy arrays or all GPU tensors (values then never visits
    the host; lon and lat do, for the gridding).

    station_grid(lon, lat, spacing, bbox) places the stations; they are sorted by cell and ONE rdr_grid_stats call computes, per station,
    the count, mean, median (pandas' (s[(m - 1) // 2] + s[m // 2]) / 2, bit for bit) and standard deviation (ddof = 1, NaN for a single
    row), and per cell the stations with a row, the means of those station statistics (NaN ones left out, NaN if none is left) and the
    same three statistics over all rows of the cell.  medians=False skips the three selections: their arrays and maps are NaN.
    float32 values are widened to float64.  There is no CPU fallback."""
    tensors = [_is_tensor(a) for a in (lon, lat, values)]
    if any(tensors) and not all(tensors):
        raise TypeError('lon, lat and values must be all NumPy arrays or all GPU tensors')
    on_device = all(tensors)
    if on_device:
        import torch
        if not (lon.is_cuda and lat.is_cuda and values.is_cuda):
            raise TypeError('tensors must live on the GPU')
        lon_h = lon.detach().to(torch.float64).cpu().numpy().reshape(-1); lat_h = lat.detach().to(torch.float64).cpu().numpy().reshape(-1)
        v = values if values.ndim == 2 else values[None, :]
    else:
        lon_h = np.asarray(lon, dtype=np.float64).reshape(-1); lat_h = np.asarray(lat, dtype=np.float64).reshape(-1)
        v = np.asarray(values)
        v = v if v.ndim == 2 else v[None, :]
    if v.ndim != 2 or v.shape[1] != lon_h.size or lat_h.size != lon_h.size:
        raise ValueError('lon, lat [N] and values [N] or [D, N] must agree in N')
    nd, ntot = int(v.shape[0]), int(v.shape[1])
    if not 1 <= nd <= MAX_DATES:
        raise ValueError(f'1 .. {MAX_DATES} dates (got {nd})')
    grid = station_grid(lon_h, lat_h, spacing, bbox)
    order, start = grid.order, grid.start
    n, ng = int(order.size), int(start.size) - 1
    if not 1 <= n <= MAX_POINTS:
        raise ValueError(f'1 .. {MAX_POINTS} stations inside the grid (got {n})')
    ctx = ctx or Context.default()
    if on_device:
        od = torch.from_numpy(np.ascontiguousarray(order)).to(v.device)
        vs = v.to(torch.float64).index_select(1, od).contiguous()
        sd = torch.from_numpy(np.ascontiguousarray(start)).to(v.device)
        ctx.adopt_torch_stream(vs)
        new = lambda size, dtype, fill: torch.full((size,), fill, dtype=dtype, device=v.device)
        f64, i64 = torch.float64, torch.int64
    else:
        od = order
        vs = np.ascontiguousarray(v[:, order], dtype=np.float64)
        sd = np.ascontiguousarray(start, dtype=np.int64)
        new = lambda size, dtype, fill: np.full(size, fill, dtype=dtype)
        f64, i64 = np.float64, np.int64
    nan = float('nan')
    st = dict(st_nobs=new(n, i64, 0), st_mean=new(n, f64, nan), st_median=new(n, f64, nan), st_stdev=new(n, f64, nan))
    ce = dict(nstations=new(ng, i64, 0), mean_of_means=new(ng, f64, nan), mean_of_medians=new(ng, f64, nan), mean_of_stdevs=new(ng, f64, nan),
              cell_nobs=new(ng, i64, 0), abs_mean=new(ng, f64, nan), abs_median=new(ng, f64, nan), abs_stdev=new(ng, f64, nan))
    med = lambda a: ptr(a) if medians else None
    check(ctx.lib.rdr_grid_stats(ctx.handle, ptr(vs), n, nd, ptr(sd), ng, ptr(st['st_nobs']), ptr(st['st_mean']), med(st['st_median']), ptr(st['st_stdev']),
                                 ptr(ce['nstations']), ptr(ce['mean_of_means']), med(ce['mean_of_medians']), ptr(ce['mean_of_stdevs']),
                                 ptr(ce['cell_nobs']), ptr(ce['abs_mean']), med(ce['abs_median']), ptr(ce['abs_stdev']),
                                 L.RDR_DEVICE if on_device else L.RDR_HOST), ctx.handle)
    res = GridStatistics(grid=grid, medians=bool(medians), **ce)
    for k, a in st.items():                                 # back to the caller's station order; NaN / 0 outside the grid
        full = new(ntot, a.dtype, 0 if k == 'st_nobs' else nan)
        full[od] = a
        setattr(res, k, full)
    gmap = lambda a: a.reshape(grid.grid_dim[0], grid.grid_dim[1]).T
    ns = ce['nstations']
    if on_device:
        heat = torch.where(ns > 0, ns.to(torch.float64), torch.full_like(ns, nan, dtype=torch.float64))
    else:
        heat = np.where(ns > 0, ns.astype(np.float64), np.nan)
    res.grid_heatmap = gmap(heat)
    res.grid_delay_mean = gmap(ce['mean_of_means']); res.grid_delay_median = gmap(ce['mean_of_medians']); res.grid_delay_stdev = gmap(ce['mean_of_stdevs'])
    res.grid_delay_absolute_mean = gmap(ce['abs_mean']); res.grid_delay_absolute_median = gmap(ce['abs_median'])
    res.grid_delay_absolute_stdev = gmap(ce['abs_stdev'])
    return res


# ---- the station table: long rows -> a [D, N] series ---------------------------------------------------------------------------------
def _day(t):
    return np.asarray(t, dtype='datetime64[ns]').astype('datetime64[D]')


def station_table(ids, lon, lat, when, values, sigma=None, obs_errlimit=np.inf, timeinterval=None, unit='m'):
    """The long table of `_reader` / `create_DF` (one row per station and time stamp: ids, lon, lat, when, values [R]; values in metres)
    -> (ids [N] sorted, lon [N], lat [N], when [D] sorted datetime64[ns], values [D, N] with NaN = no row).

    In the reference's order: values (and sigma) go from metres to `unit` (`convert_SI`; an unknown unit is refused with its message);
    with `sigma`, rows with sigma > obs_errlimit are dropped - obs_errlimit is in metres and converted like sigma (:1414-1417); rows
    with a NaN in any column (NaT in `when`) are dropped (:1430); `timeinterval` = 'YYYY-MM-DD YYYY-MM-DD' or two dates keeps the rows
    whose DAY lies in the closed interval (:1435-1437).  ValueError: an ID with two different coordinates (the reference "assumes
    station locations don't change", and one column per station needs it); two rows of one ID at one time stamp."""
    ids = np.asarray(ids).reshape(-1)
    lon = np.asarray(lon, dtype=np.float64).reshape(-1); lat = np.asarray(lat, dtype=np.float64).reshape(-1)
    when = np.asarray(when, dtype='datetime64[ns]').reshape(-1)
    val = np.asarray(values, dtype=np.float64).reshape(-1)
    r = ids.size
    if not (lon.size == lat.size == when.size == val.size == r):
        raise ValueError('ids, lon, lat, when and values must have the same length')
    val = convert_SI(val, 'm', unit)
    keep = ~(np.isnan(lon) | np.isnan(lat) | np.isnat(when) | np.isnan(val))
    if ids.dtype.kind == 'f':
        keep &= ~np.isnan(ids)
    if sigma is not None:
        sig = np.asarray(sigma, dtype=np.float64).reshape(-1)
        if sig.size != r:
            raise ValueError('sigma must have the length of the table')
        sig = convert_SI(sig, 'm', unit)
        with np.errstate(invalid='ignore'):
            keep &= sig <= convert_SI(float(obs_errlimit), 'm', unit)      # (a NaN sigma fails the comparison: the row goes, as dropna has it)
    if timeinterval is not None:
        t = timeinterval.split() if isinstance(timeinterval, str) else list(timeinterval)
        t0, t1 = _day(t[0]), _day(t[-1])
        day = when.astype('datetime64[D]')
        with np.errstate(invalid='ignore'):
            keep &= (day >= t0) & (day <= t1)
    ids, lon, lat, when, val = ids[keep], lon[keep], lat[keep], when[keep], val[keep]
    uid, first, col = np.unique(ids, return_index=True, return_inverse=True)
    col = col.reshape(-1)
    ulon, ulat = lon[first], lat[first]
    moved = (lon != ulon[col]) | (lat != ulat[col])
    if moved.any():
        k = int(np.flatnonzero(moved)[0])
        raise ValueError(f'station {ids[k]} has more than one location: ({ulon[col[k]]}, {ulat[col[k]]}) and ({lon[k]}, {lat[k]})')
    uwhen, row = np.unique(when, return_inverse=True)
    row = row.reshape(-1)
    slot = row.astype(np.int64) * max(uid.size, 1) + col
    us, cnt = np.unique(slot, return_counts=True)
    if (cnt > 1).any():
        k = int(us[cnt > 1][0])
        raise ValueError(f'station {uid[k % uid.size]} has {int(cnt[cnt > 1][0])} rows at {uwhen[k // uid.size]}')
    out = np.full((uwhen.size, uid.size), np.nan)
    out[row, col] = val
    return uid, ulon, ulat, uwhen, out


def read_station_csv(path, col_name, **kw):
    """The reference's station CSV (`_reader`, :1389-1421): columns ID, Lat, Lon, Datetime (the time stamp of a row) or Date, the column
    `col_name`, optionally sigZTD -> station_table(...), whose keywords (obs_errlimit, timeinterval, unit) pass through.  An empty
    field is a NaN and drops the row.  Read with the standard library's csv: pandas is not needed."""
    with open(path, newline='') as f:
        rd = csv.reader(f)
        try:
            head = [h.strip() for h in next(rd)]
        except StopIteration:
            head = []
        rows = [r for r in rd if r]
    if col_name not in head:
        raise Exception(f'User-specified key {col_name} not found in input file {path}. Must specify valid key.')
    tcol = 'Datetime' if 'Datetime' in head else 'Date'
    for need in ('ID', 'Lat', 'Lon', tcol):
        if need not in head:
            raise ValueError(f'{path}: no column {need}')
    col = lambda name: [r[head.index(name)].strip() if head.index(name) < len(r) else '' for r in rows]
    num = lambda name: np.array([float(x) if x else np.nan for x in col(name)], dtype=np.float64)
    when = np.array([np.datetime64(x.replace(' ', 'T').replace('Z', '')) if x else np.datetime64('NaT') for x in col(tcol)], dtype='datetime64[ns]') \
        if rows else np.zeros(0, dtype='datetime64[ns]')
    ids = np.array(col('ID'), dtype=str) if rows else np.zeros(0, dtype=str)
    sigma = num('sigZTD') if 'sigZTD' in head else None
    val = num(col_name)
    if rows:                                              # an empty ID is a missing cell too
        val = np.where(ids == '', np.nan, val)
    return station_table(ids, num('Lon'), num('Lat'), when, val, sigma=sigma, **kw)


# ---- the raster files of --grid_to_raster --------------------------------------------------------------------------------------------
def save_gridfile(array, gridfile_type, path, plotbbox, spacing, unit, colorbarfmt='%.2f', stationsongrids=False, time_lines=False, dtype='float32',
                  noData=np.nan):
    """`save_gridfile` (:436-487): `array` [ny, nx] as a one-band GeoTIFF with the transform Affine(spacing, 0, plotbbox[0], 0, -spacing,
    plotbbox[-1]), CRS 4326, nodata `noData`, samples of `dtype`, and the reference's metadata items (gridfile_type, plotbbox, spacing,
    unit, colorbarfmt, stationsongrids, time_lines) as GDAL metadata -> the metadata dict.  NaN cells of an integer raster get noData."""
    from . import tifflite
    meta = {'gridfile_type': gridfile_type, 'plotbbox': ' '.join(str(i) for i in plotbbox), 'spacing': str(spacing), 'unit': unit}
    if unit in _TIME_UNITS:
        colorbarfmt = '%1i'
    meta['colorbarfmt'] = colorbarfmt
    meta['stationsongrids'] = ' '.join(str(i) for i in stationsongrids) if stationsongrids else 'False'
    meta['time_lines'] = ' '.join(str(i) for i in time_lines) if time_lines else 'False'
    a = np.asarray(array, dtype=np.float64)
    if np.dtype(dtype).kind in 'iu':
        a = np.where(np.isnan(a), 0 if noData != noData else noData, a)
    tifflite.write(path, a.astype(dtype), transform=(float(plotbbox[0]), float(spacing), 0.0, float(plotbbox[-1]), 0.0, -float(spacing)), crs=4326,
                   nodata=noData, tags=meta)
    return meta


def load_gridfile(path, unit):
    """`load_gridfile` (:490-541): -> (array in `unit`, plotbbox, spacing, colorbarfmt, stationsongrids, time_lines).  0, NaN and inf
    read as NaN (NaN and inf only when `unit` is a time unit); the file's own unit comes from its metadata."""
    from . import tifflite
    try:
        a, prof = tifflite.read(path)
    except (TypeError, tifflite.NotATIFF):
        raise ValueError('fname is not a valid file')
    a = np.asarray(a).astype(float)
    meta = prof['tags']
    bad = [np.nan, np.inf] if unit in _TIME_UNITS else [0, np.nan, np.inf]
    for b in bad:
        a = np.where(a == b, np.nan, a)
    plotbbox = [float(i) for i in meta['plotbbox'].split()]
    spacing = float(meta['spacing'])
    inputunit = meta['unit']
    if '^2' in inputunit:
        unit = unit.split('^2')[0] + '^2'
    a = convert_SI(a, inputunit, unit)
    sog = meta.get('stationsongrids', 'False')
    tl = meta.get('time_lines', 'False')
    floats = lambda s: [float(i) for i in re.findall(r'[-+]?[0-9.]+(?:[eE][-+]?[0-9]+)?', s)]      # (lists are written with their brackets)
    sog = False if sog == 'False' else floats(sog)
    tl = False if tl == 'False' else floats(tl)
    return a, plotbbox, spacing, meta['colorbarfmt'], sog, tl
