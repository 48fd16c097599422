"""Seasonal sinusoids of `raiderStats` (cli/statsPlot.py: `_amplitude_and_phase`, :2311-2479, and the fourteen `grid_seasonal_*` maps of
create_DF, :1796-2309) on the device, as exact least squares.

The reference fits `A sin(w t + p) + c` to every station's series with one `scipy.optimize.curve_fit` per station.  Here ONE device
call (rdr_seasonal_fit, csrc/seasonal_kernels.h) gives, per station, the least-squares solution in closed form:

  fixed period  (`period_limit` years, the reference's `period_limit != 0`): the problem is linear in (a, b, c) of
                a sin(w tau) + b cos(w tau) + c; this is the reference's answer, to the accuracy of its optimiser.
  free period   (`period_range=(lo, hi)` years, for the reference's `period_limit == 0`): the least-squares sinusoid over the band, found
                by an exhaustive scan of R(w) on the grid w_k = w_lo + k delta, delta = 2 pi / (oversample * T), T the span of `when`, and
                a golden-section refinement around the grid minimum.  The reference's Levenberg-Marquardt run starts from one FFT bin
                and phase 0 with t in POSIX seconds; it ends in this minimum often, not always, and where it ends otherwise depends on
                MINPACK's step history.  So free-period results equal the reference's ONLY where its optimiser reaches the least-squares
                minimum (tests/golden/g23 records for which stations it did); elsewhere this fit has the lower residual.

  seasonal_fits  - per station: amplitude, phase, offset, period, their sigmas, rmse            -> SeasonalFits
  grid_seasonal  - the fourteen maps over the grid of `station_grid`, with the SeasonalFits behind them -> GridSeasonal

Differences from the reference, on purpose: A >= 0 always, with the phase of that sign (the reference adds 3.14159, not pi, when its
optimiser ends at A < 0); a station needs P + 1 rows (P = 3 parameters for a fixed period, 4 for a free one) - the reference accepts
P rows and reports an infinite covariance; the covariance comes from the analytic Jacobian, not from MINPACK's forward differences.
Reproduced on purpose: the labels of the three `*_c` columns, see SeasonalFits.as_reference.

Not here: the `seasonalinterval` filter (the reference itself raises there), the per-station debug plots (`phaseamp_per_station`), the
plots.  There is no CPU fallback.
"""
import math
import os

import numpy as np

from . import _lib as L
from ._lib import Context, check, ptr
from .station_stats import save_gridfile
from .variogram import MAX_DATES, MAX_POINTS, _is_tensor, station_grid

YEAR = 31556952.0                                  # the reference's seconds per year
MAX_FREQS = 4096
STATION_ROWS = ('nobs', 'span_years', 'fitted', 'at_edge', 'amplitude', 'phase', 'offset', 'omega', 'rss', 'rmse', 'sigma_amplitude', 'sigma_omega',
                'sigma_phase', 'sigma_offset', 'kstar', 'iterations')
REF_COLUMNS = ('phsfit', 'ampfit', 'periodfit', 'phsfit_c', 'ampfit_c', 'periodfit_c', 'seasonalfit_rmse')
# map -> (reference column, unit or None for the data's unit, colour-bar format), from the fourteen call sites (:1873-2309)
_MAPS = (('phase', 'phsfit', 'days', '%.1i'), ('amplitude', 'ampfit', None, '%.3f'), ('period', 'periodfit', 'years', '%.2f'),
         ('phase_stdev', 'phsfit_c', 'days', '%.1i'), ('amplitude_stdev', 'ampfit_c', None, '%.3f'), ('period_stdev', 'periodfit_c', 'years', '%.2e'),
         ('fit_rmse', 'seasonalfit_rmse', None, '%.3f'))
MAPS = tuple(f'grid_seasonal_{m[0]}' for m in _MAPS) + tuple(f'grid_seasonal_absolute_{m[0]}' for m in _MAPS)
MAP_COLUMNS = {f'grid_seasonal_{a}{m[0]}': m[1] for a in ('', 'absolute_') for m in _MAPS}
MAP_FILES = {f'grid_seasonal_{a}{m[0]}': (m[2], '%.2e' if (a and m[0] == 'fit_rmse') else m[3]) for a in ('', 'absolute_') for m in _MAPS}


class _Annual(float):
    """the default of `period_limit`: one year unless a `period_range` is given"""


_ANNUAL = _Annual(1.0)


class SeasonalFits:
    """What seasonal_fits returns, per station in the CALLER's order [N] (NumPy arrays or GPU tensors, as the inputs were):
    nobs (int64), span_years, fitted (bool), at_edge (bool: the scan's minimum is at the first or last grid frequency - the band's edge,
    not a spectral line), amplitude (>= 0), phase (radians in (-pi, pi], of A sin(w t + phase) with t in POSIX seconds), offset, omega
    (rad / s), period (years, 1 / ((omega / 2 pi) * 31556952) as at :2404-2405), frequency (1 / period, cycles per year), rss (the residual
    sum of squares), rmse (sqrt(rss / (nobs - 2)), as at :2428-2431), sigma_amplitude, sigma_phase, sigma_offset, sigma_frequency (cycles per
    year; NaN for a fixed period) and sigma_omega (rad / s; NaN for a fixed period).  An unfitted station has NaN everywhere but in nobs,
    span_years, fitted and at_edge.  scan: True for a free period; omega_grid: the frequencies of the call."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def as_reference(self):
        """The reference's seven station columns {ampfit, phsfit, periodfit, ampfit_c, phsfit_c, periodfit_c, seasonalfit_rmse}, AS THE
        REFERENCE LABELS THEM: phsfit = (365.25 / 2) sin(phase) "days", periodfit in years, and ampfit_c, periodfit_c, phsfit_c the square
        roots of the covariance entries [0, 0], [1, 1], [2, 2] (:2424-2426).  With a free period the parameters are (A, w, p, c), so these
        are the sigmas of A, of w (rad / s - not a period) and of p.  With a fixed period they are (A, p, c): `periodfit_c` is the PHASE's
        sigma and `phsfit_c` the OFFSET's.  That quirk is reproduced, since the reference's maps and files carry it."""
        sin = self.phase.sin() if _is_tensor(self.phase) else np.sin(self.phase)
        period_c, phase_c = (self.sigma_omega, self.sigma_phase) if self.scan else (self.sigma_phase, self.sigma_offset)
        return dict(ampfit=self.amplitude, phsfit=(365.25 / 2) * sin, periodfit=self.period, ampfit_c=self.sigma_amplitude, phsfit_c=phase_c,
                    periodfit_c=period_c, seasonalfit_rmse=self.rmse)


class GridSeasonal:
    """What grid_seasonal returns.  grid: the StationGrid; fits: the SeasonalFits of all stations (one outside the grid is unfitted);
    cell_means [14, G]; and the fourteen maps [ny, nx], row 0 in the north, named as in the reference: grid_seasonal_phase, _amplitude,
    _period, _phase_stdev, _amplitude_stdev, _period_stdev, _fit_rmse (the mean over the cell's fitted stations of the reference's station
    column) and their grid_seasonal_absolute_* counterparts (the mean over the cell's ROWS: each fitted station weighted by its row count).
    NaN for a cell without a fitted station."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def plotbbox(self):
        return [float(v) for v in self.grid.extent]

    def maps(self):
        return {k: getattr(self, k) for k in MAPS}

    def to_rasters(self, workdir, col_name, unit='m', stationsongrids=False, time_lines=False):
        """`--grid_to_raster`: <workdir>/<col_name>_<map>.tif for the fourteen maps, float32, with the unit and the colour-bar format of the
        reference's call sites: 'days' and '%.1i' for the phases, 'years' for the periods ('%.2f', '%.2e' for their stdev), `unit` and '%.3f'
        for the others ('%.2e' for grid_seasonal_absolute_fit_rmse).  -> {map name: path}."""
        os.makedirs(workdir, exist_ok=True)
        out = {}
        for name, a in self.maps().items():
            a = a.cpu().numpy() if _is_tensor(a) else a
            u, fmt = MAP_FILES[name]
            path = os.path.join(str(workdir), f'{col_name}_{name}.tif')
            save_gridfile(a, name, path, self.plotbbox, self.grid.spacing, u or unit, colorbarfmt=fmt, stationsongrids=stationsongrids,
                          time_lines=time_lines, dtype='float32')
            out[name] = path
        return out


def posix_seconds(when):
    """`when` [D] as float64 POSIX seconds: datetime64 of any unit, or numbers that already are seconds."""
    w = np.asarray(when)
    if w.dtype.kind == 'M':
        if np.isnat(w).any():
            raise ValueError('when holds NaT')
        return (w.astype('datetime64[ns]').astype(np.int64) / 1e9).reshape(-1)
    if w.dtype.kind not in 'fiu':
        raise TypeError('when must be datetime64 or POSIX seconds')
    w = w.astype(np.float64).reshape(-1)
    if not np.isfinite(w).all():
        raise ValueError('when must be finite')
    return w


def frequency_grid(t, period_limit=_ANNUAL, period_range=None, oversample=8):
    """The angular frequencies (rad / s) of a call over the date axis t [D] (POSIX seconds) -> (omega [K], scan).
    Fixed: one frequency, 2 pi / (period_limit * 31556952).  Scan: w_k = w_lo + k delta from 2 pi / (hi * 31556952) up to at most
    2 pi / (lo * 31556952), delta = 2 pi / (oversample * T), T = max t - min t (one frequency, w_lo, when T is 0).  ValueError: both or neither
    of period_limit / period_range, a period that is not finite and > 0, lo >= hi, oversample < 1, more than MAX_FREQS = 4096 frequencies."""
    if period_range is not None and period_limit is _ANNUAL:
        period_limit = None
    if (period_limit is None) == (period_range is None):
        raise ValueError('give exactly one of period_limit (years) and period_range=(lo, hi) years')
    if period_limit is not None:
        p = float(period_limit)
        if not (math.isfinite(p) and p > 0):
            raise ValueError(f'period_limit must be a period in years > 0 (got {period_limit}); for a free period give period_range')
        return np.array([(1 / p) * (1 / YEAR) * (2.0 * np.pi)]), False
    try:
        lo, hi = (float(v) for v in period_range)
    except (TypeError, ValueError):
        raise ValueError('period_range must be (lo, hi) in years')
    if not (math.isfinite(lo) and math.isfinite(hi) and 0 < lo < hi):
        raise ValueError(f'period_range needs 0 < lo < hi years (got {period_range})')
    if not (math.isfinite(oversample) and oversample >= 1):
        raise ValueError(f'oversample must be >= 1 (got {oversample})')
    w_lo, w_hi = 2.0 * np.pi / (hi * YEAR), 2.0 * np.pi / (lo * YEAR)
    span = float(t.max() - t.min()) if t.size else 0.0
    if span <= 0:
        return np.array([w_lo]), True
    delta = 2.0 * np.pi / (float(oversample) * span)
    k = int(math.floor((w_hi - w_lo) / delta)) + 1
    if k > MAX_FREQS:
        raise ValueError(f'the scan has {k} frequencies, more than {MAX_FREQS}: narrow period_range or lower oversample')
    return w_lo + np.arange(k) * delta, True


def _prepare(when, values, fit_args):
    """the argument checks of both entry points, before a device is needed -> (t, v [D, N], on_device, omega, scan, min_span, min_frac)"""
    known = dict(period_limit=_ANNUAL, period_range=None, oversample=8, min_span=2.0, min_frac=0.6)
    bad = set(fit_args) - set(known)
    if bad:
        raise TypeError(f'unknown argument(s) {sorted(bad)}')
    known.update(fit_args)
    if _is_tensor(when):
        raise TypeError('when is the date axis: a host array (datetime64 or POSIX seconds), also for GPU values')
    t = posix_seconds(when)
    on_device = _is_tensor(values)
    if on_device:
        if not values.is_cuda:
            raise TypeError('tensors must live on the GPU')
        v = values if values.ndim == 2 else values[None, :]
    else:
        v = np.asarray(values)
        v = v if v.ndim == 2 else v[None, :]
    if v.ndim != 2 or v.shape[0] != t.size:
        raise ValueError(f'when [D] and values [N] or [D, N] must agree in D (got {t.size} and {tuple(v.shape)})')
    if not 1 <= t.size <= MAX_DATES:
        raise ValueError(f'1 .. {MAX_DATES} dates (got {t.size})')
    if not 1 <= v.shape[1] <= MAX_POINTS:
        raise ValueError(f'1 .. {MAX_POINTS} stations (got {v.shape[1]})')
    min_span, min_frac = float(known['min_span']), float(known['min_frac'])
    if not (math.isfinite(min_span) and min_span >= 0):
        raise ValueError(f'min_span must be >= 0 years (got {min_span})')
    if not math.isfinite(min_frac):
        raise ValueError(f'min_frac must be finite (got {min_frac})')
    omega, scan = frequency_grid(t, known['period_limit'], known['period_range'], known['oversample'])
    return t, v, on_device, omega, scan, min_span, min_frac


def _fit_call(ctx, t, vs, omega, scan, min_span, min_frac, start, on_device):
    """rdr_seasonal_fit on values vs [D, n] (float64, contiguous; stations sorted by cell when `start` [G + 1] is given)
    -> (station [16, n], cells [14, G] or None)"""
    nd, n = int(vs.shape[0]), int(vs.shape[1])
    ng = 0 if start is None else int(start.shape[0]) - 1
    if on_device:
        import torch
        ctx.adopt_torch_stream(vs)
        new = lambda *shape: torch.empty(shape, dtype=torch.float64, device=vs.device)
    else:
        new = lambda *shape: np.empty(shape, dtype=np.float64)
    st = new(len(STATION_ROWS), n)
    ce = None if start is None else new(2 * len(REF_COLUMNS), ng)
    t = np.ascontiguousarray(t, dtype=np.float64); omega = np.ascontiguousarray(omega, dtype=np.float64)
    check(ctx.lib.rdr_seasonal_fit(ctx.handle, ptr(t), ptr(vs), n, nd, ptr(omega), int(omega.size), int(scan), min_span, min_frac,
                                   None if start is None else ptr(start), ng, ptr(st), None if ce is None else ptr(ce),
                                   L.RDR_DEVICE if on_device else L.RDR_HOST), ctx.handle)
    return st, ce


def _fits_of(st, scan, omega):
    """the station block [16, N] -> SeasonalFits"""
    row = {k: st[i] for i, k in enumerate(STATION_ROWS)}
    two_pi = 2.0 * np.pi
    if _is_tensor(st):
        import torch
        as_int, as_bool = (lambda a: a.to(torch.int64)), (lambda a: a != 0)
        two_pi = torch.full((), two_pi, dtype=torch.float64, device=st.device)          # (a tensor divides; a Python scalar would multiply by 1 / x)
    else:
        as_int, as_bool = (lambda a: a.astype(np.int64)), (lambda a: a != 0)
    freq = (row['omega'] / two_pi) * YEAR
    return SeasonalFits(nobs=as_int(row['nobs']), span_years=row['span_years'], fitted=as_bool(row['fitted']), at_edge=as_bool(row['at_edge']),
                        amplitude=row['amplitude'], phase=row['phase'], offset=row['offset'], omega=row['omega'], period=1 / freq, frequency=freq,
                        rss=row['rss'], rmse=row['rmse'], sigma_amplitude=row['sigma_amplitude'], sigma_phase=row['sigma_phase'],
                        sigma_offset=row['sigma_offset'], sigma_omega=row['sigma_omega'], sigma_frequency=(row['sigma_omega'] / two_pi) * YEAR,
                        kstar=row['kstar'], iterations=row['iterations'], scan=bool(scan), omega_grid=omega)


def seasonal_fits(when, values, period_limit=_ANNUAL, period_range=None, oversample=8, min_span=2.0, min_frac=0.6, ctx=None):
    """The seasonal fit of every station (`_amplitude_and_phase`, :2311-2479): when [D] (datetime64 or POSIX seconds, on the host - what
    station_table returns), values [N] or [D, N] (NaN = no row; NumPy, or a GPU tensor that never visits the host) -> SeasonalFits.

    Exactly one of period_limit (years > 0; the default, one year, steps aside for a period_range) and period_range=(lo, hi) years selects
    the mode - see the module's docstring and frequency_grid; oversample sets the scan's grid.  A station is fitted when its rows span
    at least min_span years, hold at least min_frac of the days of that span (:2346-2347), and number P + 1 or more (P = 3 parameters
    for a fixed period, 4 for a free one; the reference accepts P rows, with an infinite covariance).  float32 values are widened."""
    t, v, on_device, omega, scan, min_span, min_frac = _prepare(when, values, dict(period_limit=period_limit, period_range=period_range,
                                                                                  oversample=oversample, min_span=min_span, min_frac=min_frac))
    ctx = ctx or Context.default()
    if on_device:
        import torch
        vs = v.to(torch.float64).contiguous()
    else:
        vs = np.ascontiguousarray(v, dtype=np.float64)
    st, _ = _fit_call(ctx, t, vs, omega, scan, min_span, min_frac, None, on_device)
    return _fits_of(st, scan, omega)


def grid_seasonal(lon, lat, when, values, spacing=1.0, bbox=None, ctx=None, **fit_args):
    """The fourteen `grid_seasonal_*` maps of `raiderStats` (create_DF, :1796-2309) for stations lon / lat [N] (degrees), dates when [D]
    and values [D, N] -> GridSeasonal.  lon, lat, values are all NumPy arrays or all GPU tensors (lon and lat visit the host for the
    gridding); fit_args are seasonal_fits' (period_limit, period_range, oversample, min_span, min_frac).  station_grid places the
    stations; they are sorted by cell and ONE rdr_seasonal_fit call fits them and averages the reference's seven station columns per
    cell.  If no station is fitted, the reference's exception is raised with its message (:1838-1841)."""
    tensors = [_is_tensor(a) for a in (lon, lat, values)]
    if any(tensors) and not all(tensors):
        raise TypeError('lon, lat and values must be all NumPy arrays or all GPU tensors')
    t, v, on_device, omega, scan, min_span, min_frac = _prepare(when, values, fit_args)
    if on_device:
        import torch
        if not (lon.is_cuda and lat.is_cuda):
            raise TypeError('tensors must live on the GPU')
        lon_h = lon.detach().to(torch.float64).cpu().numpy().reshape(-1); lat_h = lat.detach().to(torch.float64).cpu().numpy().reshape(-1)
    else:
        lon_h = np.asarray(lon, dtype=np.float64).reshape(-1); lat_h = np.asarray(lat, dtype=np.float64).reshape(-1)
    if v.shape[1] != lon_h.size or lat_h.size != lon_h.size:
        raise ValueError('lon, lat [N] and values [N] or [D, N] must agree in N')
    grid = station_grid(lon_h, lat_h, spacing, bbox)
    order, start = grid.order, grid.start
    n, ntot = int(order.size), int(v.shape[1])
    if n < 1:
        raise ValueError('no station inside the grid')
    ctx = ctx or Context.default()
    nan = float('nan')
    if on_device:
        od = torch.from_numpy(np.ascontiguousarray(order)).to(v.device)
        vs = v.to(torch.float64).index_select(1, od).contiguous()
        sd = torch.from_numpy(np.ascontiguousarray(start, dtype=np.int64)).to(v.device)
        full = torch.full((len(STATION_ROWS), ntot), nan, dtype=torch.float64, device=v.device)
    else:
        od = order
        vs = np.ascontiguousarray(v[:, order], dtype=np.float64)
        sd = np.ascontiguousarray(start, dtype=np.int64)
        full = np.full((len(STATION_ROWS), ntot), nan)
    st, ce = _fit_call(ctx, t, vs, omega, scan, min_span, min_frac, sd, on_device)
    full[:4] = 0.0                                         # a station outside the grid: no rows counted, not fitted
    full[1] = nan
    full[:, od] = st
    fits = _fits_of(full, scan, omega)
    if not bool(fits.fitted.any()):
        raise Exception(f'No valid data values, adjust --min_span inputs for time span in years {min_span} and/or fractional obs. {min_frac}')
    res = GridSeasonal(grid=grid, fits=fits, cell_means=ce)
    gmap = lambda a: a.reshape(grid.grid_dim[0], grid.grid_dim[1]).T
    for a, off in (('', 0), ('absolute_', len(REF_COLUMNS))):
        for m in _MAPS:
            setattr(res, f'grid_seasonal_{a}{m[0]}', gmap(ce[off + REF_COLUMNS.index(m[1])]))
    return res
