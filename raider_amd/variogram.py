"""Empirical variograms of station delays over ALL pairs (cli/statsPlot.py:573-719, VariogramAnalysis).

The reference lists every station pair, shuffles the list and keeps 1000 (`_get_samples`), because all pairs of a GNSS network
are out of NumPy's reach.  Here the N (N - 1) / 2 pairs are evaluated on the GPU (csrc/variogram_kernels.h: rdr_pair_variogram),
for every date of a [D, N] series in one call, the distance of a pair shared by the dates of a group:

  pair_variogram      - per date and bin: pair count, sum of lags h, sum of semivariances 0.5 (v_i - v_j)^2 (the sums behind
                        `_binned_vario`, :633-659), with the reference's default bins from the largest pair distance of the date
  deramp              - the plane removal of `_emp_vario` (:620-624), per date over its valid points (host, N x 3 least squares)
  utm_common_center   - WGS84_to_UTM(common_center=True) (:621): metres in the UTM zone of the median lon / lat
  fit_variogram       - `_fit_vario` with Nparm=3 (:661-701) through scipy.optimize.least_squares (host)
  station_variograms  - the chain _emp_vario + _binned_vario + _fit_vario for every date of a series, on all pairs

With no more than 1000 pairs (N <= 45) the reference keeps every pair too and both give the same binned variogram.
"""
from collections import namedtuple

import numpy as np

from . import _lib as L
from ._lib import Context, check, ptr

TILE = 256                # points of a tile = lanes of a workgroup (csrc/variogram_kernels.h VG_TILE)
MAX_BINS = 64
MAX_POINTS = 1 << 20
MAX_DATES = 4096


def _is_tensor(a):
    return hasattr(a, 'data_ptr')


class PairVariogram:
    """Sums of an all-pair variogram.  count [D, B] (int64), lag_sum and gamma_sum [D, B] (float64), edges [1 or D, B + 1];
    hmax [D] (the largest pair distance per date) when the default bins were asked for, else None.  NumPy arrays or GPU tensors,
    as the inputs were."""

    def __init__(self, count, lag_sum, gamma_sum, edges, hmax=None):
        self.count, self.lag_sum, self.gamma_sum, self.edges, self.hmax = count, lag_sum, gamma_sum, edges, hmax

    @property
    def ndates(self):
        return int(self.count.shape[0])

    def binned(self, d=0):
        """(hExp, expVario) of date d: the bins' mean lag and mean semivariance, empty bins dropped - what `_binned_vario`
        returns (:633-659)."""
        c = self.count[d]
        keep = c > 0
        n = c[keep]
        return self.lag_sum[d][keep] / n, self.gamma_sum[d][keep] / n


def _check_edges_host(edges, nd):
    e = np.asarray(edges, dtype=np.float64)
    if e.ndim == 1:
        e = e[None, :]
    if e.ndim != 2 or e.shape[1] < 2:
        raise ValueError(f'edges must be [B + 1] or [D, B + 1] with B >= 1 (got shape {np.shape(edges)})')
    if e.shape[1] - 1 > MAX_BINS:
        raise ValueError(f'at most {MAX_BINS} bins (got {e.shape[1] - 1})')
    if e.shape[0] not in (1, nd):
        raise ValueError(f'edges must have one row, or one row per date ({nd}); got {e.shape[0]} rows')
    if not np.isfinite(e).all() or not (np.diff(e, axis=1) > 0).all():
        raise ValueError('every row of edges must be finite and strictly ascending')
    return np.ascontiguousarray(e)


def default_edges(hmax, nbins=19):
    """The reference's default bins per date: linspace(0, 0.67 * hmax[d], nbins + 1) (:638, where nbins + 1 = 20).  [D, nbins + 1]."""
    hmax = np.atleast_1d(np.asarray(hmax, dtype=np.float64))
    return np.stack([np.linspace(0, h * 0.67, nbins + 1) for h in hmax])


def _usable_rows(edges):
    """Rows the kernel takes: a date without a pair (hmax NaN) or with all points in one place (hmax 0) has no ascending default
    row; nothing can fall into its bins anyway (no pair, or only pairs with h = 0 <= edges[0]), so any valid row stands in."""
    e = edges.copy()
    bad = ~(np.isfinite(e).all(axis=1) & (np.diff(e, axis=1) > 0).all(axis=1))
    e[bad] = np.linspace(0.0, 1.0, e.shape[1])
    return e


def pair_variogram(x, y, values, edges=None, nbins=19, ctx=None):
    """All-pair variogram sums of `values` ([N] or [D, N]; NaN = missing) at points x, y [N] in metres -> PairVariogram.

    edges: [B + 1] for all dates or [D, B + 1], strictly ascending; bin b takes the pairs with edges[b] < h <= edges[b + 1]
    (:644).  None: the reference's default per date, linspace(0, 0.67 * hmax[d], nbins + 1), from the largest pair distance of
    the date (one more pass over the pairs).  float32 values are widened to float64: sums are float64 throughout.  Coordinates must
    be finite.  NumPy arrays in -> NumPy arrays out.  GPU tensors in (x, y, values) -> tensors out, and `values` never visits the
    host; `edges` may then be a tensor or an array."""
    tensors = [_is_tensor(a) for a in (x, y, values)]
    if any(tensors) and not all(tensors):
        raise TypeError('x, y and values must be all NumPy arrays or all GPU tensors')
    on_device = all(tensors)
    if on_device:
        import torch
        if not (x.is_cuda and y.is_cuda and values.is_cuda):
            raise TypeError('tensors must live on the GPU')
        x = x.to(torch.float64).contiguous().reshape(-1); y = y.to(torch.float64).contiguous().reshape(-1)
        v = values.to(torch.float64).contiguous()
    else:
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1); y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        v = np.ascontiguousarray(values, dtype=np.float64)
    if v.ndim == 1:
        v = v[None, :]
    if v.ndim != 2:
        raise ValueError(f'values must be [N] or [D, N] (got {v.ndim} dimensions)')
    nd, n = int(v.shape[0]), int(v.shape[1])
    if x.shape[0] != n or y.shape[0] != n:
        raise ValueError(f'x ({x.shape[0]}), y ({y.shape[0]}) and the last axis of values ({n}) must have the same length')
    if not 2 <= n <= MAX_POINTS:
        raise ValueError(f'2 .. {MAX_POINTS} points (got {n})')
    if not 1 <= nd <= MAX_DATES:
        raise ValueError(f'1 .. {MAX_DATES} dates (got {nd})')
    if edges is None:
        nbins = int(nbins)
        if not 1 <= nbins <= MAX_BINS:
            raise ValueError(f'nbins must be 1 .. {MAX_BINS} (got {nbins})')
    elif not (on_device and _is_tensor(edges)):
        edges = _check_edges_host(edges.detach().cpu().numpy() if _is_tensor(edges) else edges, nd)
    else:                                   # a row on the device: the library reads it back for the ascending check
        if edges.ndim == 1:
            edges = edges[None, :]
        if edges.ndim != 2 or edges.shape[0] not in (1, nd) or not 2 <= edges.shape[1] <= MAX_BINS + 1:
            raise ValueError(f'edges must be [B + 1] or [D, B + 1] with 1 <= B <= {MAX_BINS} and D = {nd} (got {tuple(edges.shape)})')

    ctx = ctx or Context.default()
    loc = L.RDR_DEVICE if on_device else L.RDR_HOST
    hmax = None
    if on_device:
        import torch
        ctx.adopt_torch_stream(v)
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=v.device)
        f64, i64 = torch.float64, torch.int64
    else:
        new = lambda shape, dtype: np.empty(shape, dtype=dtype)
        f64, i64 = np.float64, np.int64
    shown = None
    if edges is None:
        hmax = new((nd,), f64)
        check(ctx.lib.rdr_pair_distance_max(ctx.handle, ptr(x), ptr(y), n, ptr(v), nd, ptr(hmax), loc), ctx.handle)
        shown = default_edges(hmax.cpu().numpy() if on_device else hmax, nbins)      # D numbers come down, D rows go up
        edges = _usable_rows(shown)
    if on_device:
        import torch
        if not _is_tensor(edges):
            edges = torch.from_numpy(np.ascontiguousarray(edges)).to(v.device)
            shown = edges if shown is None else torch.from_numpy(shown).to(v.device)
        else:
            edges = edges.to(device=v.device, dtype=torch.float64).contiguous()
    rows, nb = int(edges.shape[0]), int(edges.shape[1]) - 1
    count = new((nd, nb), i64); lag = new((nd, nb), f64); gam = new((nd, nb), f64)
    check(ctx.lib.rdr_pair_variogram(ctx.handle, ptr(x), ptr(y), n, ptr(v), nd, ptr(edges), rows, nb, ptr(count), ptr(lag), ptr(gam), loc),
          ctx.handle)
    return PairVariogram(count, lag, gam, edges if shown is None else shown, hmax)


def deramp(x, y, values):
    """values ([N] or [D, N], NaN = missing) minus, per date, the plane a x + b y + c fitted to that date's valid points by
    np.linalg.lstsq - the reference's arithmetic (:622-624).  NaNs stay NaN; a date with fewer than three valid points is returned
    as it is.  Host arrays."""
    x = np.asarray(x, dtype=np.float64).reshape(-1); y = np.asarray(y, dtype=np.float64).reshape(-1)
    v = np.asarray(values, dtype=np.float64)
    one = v.ndim == 1
    v2 = np.array(v[None, :] if one else v, dtype=np.float64)
    if v2.ndim != 2 or v2.shape[1] != x.size or y.size != x.size:
        raise ValueError('x, y [N] and values [N] or [D, N] must agree in N')
    for d in range(v2.shape[0]):
        m = ~np.isnan(v2[d])
        if m.sum() < 3:
            continue
        A = np.array([x[m], y[m], np.ones(int(m.sum()))]).T
        ramp = np.linalg.lstsq(A, v2[d][m].T, rcond=None)[0]
        v2[d][m] = v2[d][m] - np.matmul(A, ramp)
    return v2[0] if one else v2


_remove_plane = deramp      # (station_variograms has a keyword of that name)


def utm_zone(lon, lat):
    """(zone 1 .. 60, north?) of a point by the plain 6-degree rule."""
    zone = int((float(lon) + 180.0) // 6.0) % 60 + 1
    return zone, float(lat) >= 0.0


def utm_common_center(lon, lat):
    """(x, y) metres of lon / lat [deg] in ONE UTM zone, that of the median lon and median lat - WGS84_to_UTM(common_center=True),
    utilFcns.py:525-549 - through the device transform (transformPoints to EPSG 326zz north / 327zz south).  The zone comes from the
    plain 6-degree rule: the exceptions around Norway (32V) and Svalbard (31X - 37X) are NOT reproduced."""
    from .delay import transformPoints
    lon = np.asarray(lon, dtype=np.float64); lat = np.asarray(lat, dtype=np.float64)
    if lon.shape != lat.shape or lon.size == 0:
        raise ValueError('lon and lat must have the same, non-empty shape')
    zone, north = utm_zone(np.median(lon), np.median(lat))
    p = transformPoints(lat, lon, np.zeros(lon.shape), 4326, (32600 if north else 32700) + zone)
    return p[..., 1], p[..., 0]


def exponential(parms, h, nugget=False):
    """__exponential__ (:704-713): a = range, b = sill, c = nugget."""
    a, b, c = parms
    with np.errstate(over='ignore', divide='ignore', invalid='ignore'):
        return b * (1 - np.exp(-h / a)) + (c if nugget else 0.0)


def gaussian(parms, h):
    """__gaussian__ (:716-719)."""
    a, b, c = parms
    return b * (1 - np.exp(-np.square(h) / (a ** 2))) + c


VariogramFit = namedtuple('VariogramFit', 'params d_test v_test result')


def fit_variogram(h, gamma, model='exponential', ub=None):
    """`_fit_vario(h, gamma, model, x0=None, Nparm=3)` (:661-701): bounds 0 .. 0.8 * (max h, max gamma, max gamma), start in the
    middle, soft_l1 loss with f_scale 0.1; `ub` replaces the upper bounds, as _fit_vario's argument of that name does.  Under the default
    bounds the sill of a curve without nugget cannot be reached (it lies above every sample, hence above 0.8 * max gamma): the reference
    has this property and it is kept.  -> VariogramFit(params = (range, sill, nugget), d_test, v_test, result)."""
    from scipy.optimize import least_squares
    fn = {'exponential': exponential, 'gaussian': gaussian}.get(model, model)
    if not callable(fn):
        raise ValueError(f"model must be 'exponential', 'gaussian' or a function (got {model!r})")
    dists = np.asarray(h, dtype=np.float64); vario = np.asarray(gamma, dtype=np.float64)
    if dists.shape != vario.shape or dists.ndim != 1:
        raise ValueError('h and gamma must be 1-D and of the same length')
    mask = np.isnan(dists) | np.isnan(vario)
    d = dists[~mask].copy(); v = vario[~mask].copy()
    if d.size == 0:
        raise ValueError('no binned value to fit')
    if ub is None:
        ub = np.array([np.nanmax(dists) * 0.8, np.nanmax(vario) * 0.8, np.nanmax(vario) * 0.8])
    ub = np.asarray(ub, dtype=np.float64)
    if ub.shape != (3,):
        raise ValueError('ub must hold three upper bounds: range, sill, nugget')
    lb = np.zeros(3)
    x0 = (ub - lb) / 2
    res = least_squares(lambda p, dd, vv, m: m(p, dd) - vv, x0, bounds=(lb, ub), loss='soft_l1', f_scale=0.1, args=(d, v, fn))
    d_test = np.linspace(0, np.nanmax(dists), 100)
    return VariogramFit(res.x, d_test, fn(res.x, d_test), res)


StationVariograms = namedtuple('StationVariograms', 'variogram binned fits x y')


def station_variograms(lon, lat, values, deramp=True, edges=None, nbins=19, model='exponential', density_threshold=10, fit=True, ctx=None):
    """_emp_vario + _binned_vario + _fit_vario (:611-701, as _append_variogram chains them) for every date of `values` [D, N] at
    stations lon / lat [deg], over ALL pairs of the stations valid on the date.  One UTM zone serves every date: that of the medians
    over all stations (the reference takes the medians of each date's valid stations).  A date with fewer than `density_threshold` valid
    stations gives empty binned arrays and no fit, as the reference's empty sample does.
    -> StationVariograms(variogram = PairVariogram, binned = [(hExp, expVario)] per date, fits = [VariogramFit or None], x, y)."""
    v = np.asarray(values, dtype=np.float64)
    v = np.array(v[None, :] if v.ndim == 1 else v)
    x, y = utm_common_center(np.asarray(lon, dtype=np.float64).reshape(-1), np.asarray(lat, dtype=np.float64).reshape(-1))
    valid = (~np.isnan(v)).sum(axis=1)
    v[valid < density_threshold] = np.nan
    if deramp:
        v = _remove_plane(x, y, v)
    pv = pair_variogram(x, y, v, edges=edges, nbins=nbins, ctx=ctx)
    binned, fits = [], []
    for d in range(v.shape[0]):
        h, g = pv.binned(d)
        binned.append((h, g))
        fits.append(fit_variogram(h, g, model) if (fit and h.size) else None)
    return StationVariograms(pv, binned, fits, x, y)
