"""Empirical variograms of station delays over ALL pairs (cli/statsPlot.py:573-719, VariogramAnalysis).

The reference lists every station pair, shuffles the list and keeps 1000 (`_get_samples`), because all pairs of a GNSS network
are out of NumPy's reach.  Here the N (N - 1) / 2 pairs are evaluated on the GPU (csrc/variogram_kernels.h: rdr_pair_variogram),
for every date of a [D, N] series in one call, the distance of a pair shared by the dates of a group:

  pair_variogram      - per date and bin: pair count, sum of lags h, sum of semivariances 0.5 (v_i - v_j)^2 (the sums behind
                        `_binned_vario`, :633-659), with the reference's default bins from the largest pair distance of the date
  deramp              - the plane removal of `_emp_vario` (:620-624), per date over its valid points (host, N x 3 least squares)
  utm_common_center   - WGS84_to_UTM(common_center=True) (:621): metres in the UTM zone of the median lon / lat
  fit_variogram       - `_fit_vario` with Nparm=3 (:661-701) through scipy.optimize.least_squares (host)
  fit_variograms      - exponential models of MANY binned variograms in one device call (csrc/variogram_fit_kernels.h: rdr_variogram_fit),
                        each the exact minimum of _fit_vario's own objective over its own bounds; `fitter='device'` of the two drivers
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


# ---- exponential models as exact bounded minima, every row in one device call ---------------------------------------------------------
MAX_FIT_COLUMNS = 65536
MAX_FITS = 1 << 22
AT_FLOOR, AT_UB_A, SILL_ZERO, SILL_UB = 1, 2, 4, 8         # bits of VariogramFits.flags


class VariogramFits(namedtuple('VariogramFits', 'params cost rmse n status flags')):
    """What fit_variograms returns, per row [F] (NumPy arrays or GPU tensors, as the inputs were): params [F, 3] = (range, sill, the
    reference's untouched nugget start ub_c / 2), cost (scipy's soft_l1 cost at the minimum), rmse = sqrt(mean r^2), n (int64: the
    columns present), status (int32: 0 fitted, 1 no column present, 2 unusable bounds or values, 3 no positive lag; NaN in params, cost,
    rmse unless 0) and flags (int32 bits: AT_FLOOR = 1 range at h_pos / 38, AT_UB_A = 2 range at its upper bound, SILL_ZERO = 4,
    SILL_UB = 8).  hmax [F] (an attribute, not a field): the row's largest lag, for curve()."""

    def __new__(cls, params, cost, rmse, n, status, flags, hmax=None):
        self = super().__new__(cls, params, cost, rmse, n, status, flags)
        self.hmax = hmax
        return self

    def curve(self, f, npts=100):
        """(d_test, v_test) of row f as `_fit_vario` returns them: the model on linspace(0, the row's largest lag, npts).  Host arrays."""
        host = lambda a: a.detach().cpu().numpy() if _is_tensor(a) else np.asarray(a)
        d_test = np.linspace(0, float(host(self.hmax[f])), npts)
        return d_test, exponential(host(self.params[f]), d_test)


def fit_variograms(h, gamma, ub=None, f_scale=0.1, k_scan=512, ctx=None):
    """The exponential model b (1 - exp(-h / a)) of every row of h, gamma ([M] or [F, M]; NaN in either = column absent) in ONE device call
    (rdr_variogram_fit) -> VariogramFits over F rows (F = 1 for [M]).  Each fit is the exact minimum of `_fit_vario`'s objective - scipy's
    soft_l1 cost with f_scale - over `_fit_vario`'s box 0 .. ub: ub [3] or [F, 3] (range, sill, nugget), None for the reference's
    0.8 * (max h, max gamma, max gamma) per row.  The range is found by a scan of k_scan (a multiple of 64 in 64 .. 4096) geometrically
    spaced candidates and eight refinement rounds, each candidate at its own best sill; include/raider_hip.h states the contract.
    scipy's trust-region run (fit_variogram) stops short of this minimum on delays in metres: its gradient tolerance is absolute.
    h, gamma (and ub) are all NumPy arrays or all GPU tensors; the outputs are of the same kind.  There is no CPU fallback."""
    tensors = [_is_tensor(a) for a in (h, gamma)]
    if any(tensors) and not all(tensors):
        raise TypeError('h and gamma must be both NumPy arrays or both GPU tensors')
    on_device = all(tensors)
    if on_device:
        import torch
        if not (h.is_cuda and gamma.is_cuda):
            raise TypeError('tensors must live on the GPU')
        h = h.to(torch.float64); g = gamma.to(torch.float64)
        h = (h if h.ndim == 2 else h[None]).contiguous(); g = (g if g.ndim == 2 else g[None]).contiguous()
    else:
        h = np.asarray(h, dtype=np.float64); g = np.asarray(gamma, dtype=np.float64)
        h = np.ascontiguousarray(h if h.ndim == 2 else h[None]); g = np.ascontiguousarray(g if g.ndim == 2 else g[None])
    if h.ndim != 2 or tuple(h.shape) != tuple(g.shape):
        raise ValueError(f'h and gamma must be [M] or [F, M] and of the same shape (got {tuple(h.shape)} and {tuple(g.shape)})')
    nf, m = int(h.shape[0]), int(h.shape[1])
    if not 1 <= nf <= MAX_FITS:
        raise ValueError(f'1 .. {MAX_FITS} rows (got {nf})')
    if not 1 <= m <= MAX_FIT_COLUMNS:
        raise ValueError(f'1 .. {MAX_FIT_COLUMNS} columns (got {m})')
    k_scan = int(k_scan); f_scale = float(f_scale)
    if not 64 <= k_scan <= 4096 or k_scan % 64:
        raise ValueError(f'k_scan must be a multiple of 64 in 64 .. 4096 (got {k_scan})')
    if not (np.isfinite(f_scale) and f_scale > 0):
        raise ValueError(f'f_scale must be finite and > 0 (got {f_scale})')
    if ub is not None:
        shape = tuple(ub.shape) if hasattr(ub, 'shape') else np.shape(ub)
        if shape not in ((3,), (1, 3), (nf, 3)):
            raise ValueError(f'ub must hold three upper bounds (range, sill, nugget), [3] or [F, 3] (got shape {shape})')
        if on_device:
            ub = ub.to(device=h.device, dtype=torch.float64) if _is_tensor(ub) else torch.from_numpy(np.asarray(ub, dtype=np.float64)).to(h.device)
            ub = ub.reshape(-1, 3).expand(nf, 3).contiguous()
        else:
            ub = np.asarray(ub.detach().cpu().numpy() if _is_tensor(ub) else ub, dtype=np.float64)
            ub = np.ascontiguousarray(np.broadcast_to(ub.reshape(-1, 3), (nf, 3)))
    ctx = ctx or Context.default()
    if on_device:
        ctx.adopt_torch_stream(h)
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=h.device)
        f64, i64, i32 = torch.float64, torch.int64, torch.int32
        hmax = torch.where(torch.isnan(h), torch.full_like(h, -np.inf), h).amax(dim=1)
        hmax = torch.where(torch.isinf(hmax) & (hmax < 0), torch.full_like(hmax, np.nan), hmax)
    else:
        new = lambda shape, dtype: np.empty(shape, dtype=dtype)
        f64, i64, i32 = np.float64, np.int64, np.int32
        hmax = np.where(np.isnan(h), -np.inf, h).max(axis=1)
        hmax = np.where(np.isneginf(hmax), np.nan, hmax)
    o = VariogramFits(new((nf, 3), f64), new((nf,), f64), new((nf,), f64), new((nf,), i64), new((nf,), i32), new((nf,), i32), hmax)
    check(ctx.lib.rdr_variogram_fit(ctx.handle, ptr(h), ptr(g), nf, m, ptr(ub), f_scale, k_scan, ptr(o.params), ptr(o.cost), ptr(o.rmse), ptr(o.n),
                                    ptr(o.status), ptr(o.flags), L.RDR_DEVICE if on_device else L.RDR_HOST), ctx.handle)
    return o


def _mean_rows(total, count):
    """total / count per bin, NaN where count is 0 - elementwise where the sums live (NumPy arrays or GPU tensors)"""
    if _is_tensor(total):
        import torch
        return torch.where(count > 0, total / count, torch.full_like(total, np.nan))
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(count > 0, total / count, np.nan)


def _check_fitter(fitter, model):
    if fitter not in ('scipy', 'device'):
        raise ValueError(f"fitter must be 'scipy' or 'device' (got {fitter!r})")
    if fitter == 'device' and model != 'exponential':
        raise ValueError(f"fitter='device' fits the exponential model only (got model={model!r}): the Gaussian model carries a live nugget and stays on the host")


StationVariograms = namedtuple('StationVariograms', 'variogram binned fits x y')


def station_variograms(lon, lat, values, deramp=True, edges=None, nbins=19, model='exponential', density_threshold=10, fit=True, ctx=None,
                       fitter='scipy'):
    """_emp_vario + _binned_vario + _fit_vario (:611-701, as _append_variogram chains them) for every date of `values` [D, N] at
    stations lon / lat [deg], over ALL pairs of the stations valid on the date.  One UTM zone serves every date: that of the medians
    over all stations (the reference takes the medians of each date's valid stations).  A date with fewer than `density_threshold` valid
    stations gives empty binned arrays and no fit, as the reference's empty sample does.
    -> StationVariograms(variogram = PairVariogram, binned = [(hExp, expVario)] per date, fits = [VariogramFit or None], x, y).
    fitter='device': all dates are fitted in one fit_variograms call and `fits` is its VariogramFits over the D dates (status 1 for a date
    without a binned value); the exponential model only."""
    _check_fitter(fitter, model)
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
        if fitter == 'scipy':
            fits.append(fit_variogram(h, g, model) if (fit and h.size) else None)
    if fitter == 'device':
        fits = fit_variograms(_mean_rows(pv.lag_sum, pv.count), _mean_rows(pv.gamma_sum, pv.count), ctx=ctx) if fit else None
    return StationVariograms(pv, binned, fits, x, y)


# ---- per-grid-cell variograms: the gridding of raiderStats and _append_variogram over all cells and dates in one device pass ---------
StationGrid = namedtuple('StationGrid', 'extent spacing grid_dim gridpoints cell order start')


def station_grid(lon, lat, spacing=1.0, bbox=None):
    """The grid of `RaiderStats._get_extent` (cli/statsPlot.py:1291-1368) and the cell of every station -> StationGrid.

    extent [W, E, S, N] = floor / ceil of the stations' bounds, or of `bbox` = [S, N, W, E] (which must overlap the stations' extent
    and stay within +-180 / +-90: the reference's two exceptions, here ValueError with its messages); clamped to +-180 / +-90.  A
    spacing that does not divide both extents is reset to 1 with a warning (:1339).  grid_dim = [nx, ny].  gridpoints [G, 2] (lon, lat
    of the cell centres) in the reference's order: cell g = ix * ny + (ny - 1 - iy), ix counted from the west, iy from the south, so a
    map is a[g].reshape(nx, ny).T with row 0 in the north.

    cell [N]: station i lies in ix = min(floor((lon - W) / spacing), nx - 1), likewise iy - a cell owns its west and south edges, the
    outer east and north borders belong to the last column and row (the reference resolves a station exactly on an interior edge by
    R-tree order, which is not a rule); -1 for a station outside the extent (or NaN), which takes part in nothing.  order: a stable
    argsort of cell without the dropped stations; start [G + 1]: cell g owns order[start[g]:start[g + 1]]."""
    import warnings
    lon = np.asarray(lon, dtype=np.float64).reshape(-1); lat = np.asarray(lat, dtype=np.float64).reshape(-1)
    if lon.size != lat.size or lon.size == 0:
        raise ValueError('lon and lat must have the same, non-empty length')
    extent = [np.floor(np.nanmin(lon)), np.ceil(np.nanmax(lon)), np.floor(np.nanmin(lat)), np.ceil(np.nanmax(lat))]
    if bbox is not None:
        s, n, w, e = (float(b) for b in bbox)
        if e < extent[0] or w > extent[1] or n < extent[2] or s > extent[3]:          # closed rectangles: touching counts as overlap
            raise ValueError('User-specified bounds do not overlap with dataset bounds, adjust bounds and re-run program.')
        extent = [np.floor(w), np.ceil(e), np.floor(s), np.ceil(n)]
        if extent[0] < -180.0 or extent[1] > 180.0 or extent[2] < -90.0 or extent[3] > 90.0:
            raise ValueError('Specified bounds exceed -180/180 lon and/or -90/90 lat, adjust bounds and re-run program.')
    extent = [max(extent[0], -180.0), min(extent[1], 180.0), max(extent[2], -90.0), min(extent[3], 90.0)]
    if (extent[1] - extent[0]) % spacing != 0 or (extent[3] - extent[2]) % spacing:
        warnings.warn(f'spacing {spacing} is not an even multiple of the bounds, reset to 1 degree')
        spacing = 1
    nx, ny = int((extent[1] - extent[0]) / spacing), int((extent[3] - extent[2]) / spacing)
    # centres by the reference's running sums: x from the east edge downwards, y from the south edge upwards, the list then reversed
    xs, x = [], extent[1] - spacing / 2
    while x >= extent[0] + spacing / 2:
        xs.append(x); x -= spacing
    ys, y = [], extent[2] + spacing / 2
    while y <= extent[3] - spacing / 2:
        ys.append(y); y += spacing
    if len(xs) != nx or len(ys) != ny:
        raise ValueError(f'the grid of spacing {spacing} over {extent} has {len(xs)} x {len(ys)} centres, not {nx} x {ny}')
    gridpoints = np.array([[xv, yv] for xv in xs[::-1] for yv in ys[::-1]], dtype=np.float64).reshape(nx * ny, 2)
    with np.errstate(invalid='ignore'):
        inside = (lon >= extent[0]) & (lon <= extent[1]) & (lat >= extent[2]) & (lat <= extent[3])
        ix = np.minimum(np.floor((np.where(inside, lon, extent[0]) - extent[0]) / spacing), nx - 1).astype(np.int64)
        iy = np.minimum(np.floor((np.where(inside, lat, extent[2]) - extent[2]) / spacing), ny - 1).astype(np.int64)
    cell = np.where(inside, ix * ny + (ny - 1 - iy), -1).astype(np.int64)
    order = np.argsort(cell, kind='stable')
    order = order[cell[order] >= 0]
    start = np.concatenate([[0], np.cumsum(np.bincount(cell[order], minlength=nx * ny))]).astype(np.int64)
    return StationGrid(extent, spacing, [nx, ny], gridpoints, cell, order, start)


class GridVariograms:
    """What grid_variograms returns.  grid: the StationGrid; G cells, D dates, B bins.  nvalid, hmax, status [G, D] (status 0 done on
    the device, 1 skipped - fewer than density_threshold valid stations -, 2 done through the host chain: a singular plane); count,
    lag_sum, gamma_sum [G, D, B] and edges [G, D, B + 1] per slice; total_count, total_lag, total_gamma [G, B] in total_edges [G, B + 1]:
    all good dates of a cell binned together; these sums are NumPy arrays or GPU tensors as the inputs were.  Host arrays: params [G, 3]
    (range, sill, nugget of the total fit) and rmse [G], NaN for a cell without a good date; sparse_grids: the cells that hold stations
    but no good date; skipped_slices: (cell, date index) of the slices that hold data but fewer than density_threshold stations;
    grid_range, grid_variance, grid_variogram_rmse [ny, nx]: the maps, row 0 in the north (cli/statsPlot.py:3302-3337);
    date_fits: {(cell, date index): VariogramFit} when per_date_fits was asked for (fitter='device': a VariogramFits over [G * D] rows), else
    None; x, y: the sorted stations' metres."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def binned(self, c, d):
        """(hExp, expVario) of cell c on date d, empty bins dropped (_binned_vario)."""
        n = self.count[c][d]
        keep = n > 0
        return self.lag_sum[c][d][keep] / n[keep], self.gamma_sum[c][d][keep] / n[keep]

    def total_binned(self, c):
        """(hExp, expVario) of all good dates of cell c binned together (:801)."""
        n = self.total_count[c]
        keep = n > 0
        return self.total_lag[c][keep] / n[keep], self.total_gamma[c][keep] / n[keep]

    def map(self, a):
        """[G] -> [ny, nx], row 0 in the north."""
        return np.asarray(a).reshape(self.grid.grid_dim).T


def _cell_call(ctx, x, y, start, v, deramp, min_valid, edges, nbins, residuals, totals, on_device):
    """One rdr_cell_variogram call on sorted stations -> dict of outputs (arrays or tensors, as x is)."""
    nd, n, g = int(v.shape[0]), int(v.shape[1]), int(start.shape[0]) - 1
    if on_device:
        import torch
        new = lambda shape, dtype: torch.empty(shape, dtype=dtype, device=v.device)
        f64, i64, i32 = torch.float64, torch.int64, torch.int32
    else:
        new = lambda shape, dtype: np.empty(shape, dtype=dtype)
        f64, i64, i32 = np.float64, np.int64, np.int32
    o = dict(nvalid=new((g, nd), i64), hmax=new((g, nd), f64), status=new((g, nd), i32), count=new((g, nd, nbins), i64),
             lag_sum=new((g, nd, nbins), f64), gamma_sum=new((g, nd, nbins), f64), edges=new((g, nd, nbins + 1), f64),
             residuals=new((nd, n), f64) if residuals else None)
    for k in ('total_count', 'total_lag', 'total_gamma'):
        o[k] = new((g, nbins), i64 if k == 'total_count' else f64) if totals else None
    check(ctx.lib.rdr_cell_variogram(ctx.handle, ptr(x), ptr(y), n, ptr(start), g, ptr(v), nd, int(bool(deramp)), int(min_valid), ptr(edges), nbins,
                                     ptr(o['nvalid']), ptr(o['hmax']), ptr(o['status']), ptr(o['count']), ptr(o['lag_sum']), ptr(o['gamma_sum']),
                                     ptr(o['edges']), ptr(o['residuals']), ptr(o['total_count']), ptr(o['total_lag']), ptr(o['total_gamma']),
                                     L.RDR_DEVICE if on_device else L.RDR_HOST), ctx.handle)
    return o


def grid_variograms(lon, lat, values, spacing=1.0, bbox=None, density_threshold=10, deramp=True, nbins=19, binned=False, model='exponential',
                    errlimit=np.inf, fit=True, per_date_fits=False, ctx=None, fitter='scipy'):
    """`raiderStats --variogramplot` up to its three maps (VariogramAnalysis.create_variograms / _append_variogram, cli/statsPlot.py:721-883,
    and stats_analyses :3300-3339) for stations lon / lat [N] (degrees) and values [D, N] (NaN = missing), over ALL pairs of every cell
    -> GridVariograms.  lon, lat, values are all NumPy arrays or all GPU tensors (values then never visits the host; lon and lat do, for
    the gridding).

      1. station_grid(lon, lat, spacing, bbox); metres in ONE UTM zone per cell, that of the medians of the cell's stations - the rule of
         station_variograms; the reference takes the medians of each date's valid stations.  Cells are grouped by zone: one transform
         per zone.
      2. one device pass (rdr_cell_variogram): per cell and date the plane removal, the largest pair distance, the default bins
         linspace(0, 0.67 hmax, nbins + 1) and the binned sums.  A slice with fewer than density_threshold valid stations is skipped.
      3. the few slices whose plane is numerically singular (stations on one line; status 2) are redone through the host chain, `deramp`
         (np.linalg.lstsq) + pair_variogram, and patched in.
      4. per cell, one row linspace(0, 0.67 * the largest hmax of its good dates, nbins + 1), and
      5. a second pass over the residuals in those rows, summed over the good dates: _binned_vario of the concatenated raw arrays (:801).
      6. per cell with a good date: fit_variogram (host, scipy.optimize.least_squares, as the reference) of the total binned variogram
         - of the concatenated per-date binned arrays with binned=True (:796-798); rmse = sqrt(nanmean(fun^2)), NaN above errlimit.
         fit=False leaves params and rmse NaN.  per_date_fits=True also fits every good slice: one host scipy fit per slice, G x D of
         them - off by default, the maps do not need them.
         fitter='device' (the exponential model only): the fits are fit_variograms' exact bounded minima instead.  The rows lag_sum / count
         (NaN for an empty bin) are formed where the sums live; ALL total fits are one device call - with binned=True on the rows
         [G, D * nbins] of the per-date bins, NaN for a date that is not good -, and with per_date_fits=True all G x D slices are a second
         one: date_fits is then a VariogramFits over [G * D] rows (row c * D + d; a slice that is not good has status 1), not a dict."""
    _check_fitter(fitter, model)
    tensors = [_is_tensor(a) for a in (lon, lat, values)]
    if any(tensors) and not all(tensors):
        raise TypeError('lon, lat and values must be all NumPy arrays or all GPU tensors')
    on_device = all(tensors)
    nbins = int(nbins)
    if not 1 <= nbins <= MAX_BINS:
        raise ValueError(f'nbins must be 1 .. {MAX_BINS} (got {nbins})')
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
    nd = int(v.shape[0])
    if not 1 <= nd <= MAX_DATES:
        raise ValueError(f'1 .. {MAX_DATES} dates (got {nd})')
    grid = station_grid(lon_h, lat_h, spacing, bbox)
    order, start = grid.order, grid.start
    n, ng = int(order.size), int(start.size) - 1
    if not 2 <= n <= MAX_POINTS:
        raise ValueError(f'2 .. {MAX_POINTS} stations inside the grid (got {n})')
    # 1. metres, one transform per UTM zone
    from .delay import transformPoints
    lo, la = lon_h[order], lat_h[order]
    full = np.flatnonzero(np.diff(start) > 0)
    zones = {}
    for c in full:
        sl = slice(start[c], start[c + 1])
        zones.setdefault(utm_zone(np.median(lo[sl]), np.median(la[sl])), []).append(c)
    x = np.empty(n); y = np.empty(n)
    for (zone, north), cells in zones.items():
        idx = np.concatenate([np.arange(start[c], start[c + 1]) for c in cells])
        p = transformPoints(la[idx], lo[idx], np.zeros(idx.size), 4326, (32600 if north else 32700) + zone)
        x[idx] = p[..., 1]; y[idx] = p[..., 0]
    ctx = ctx or Context.default()
    if on_device:
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(v.device)
        vs = v.to(torch.float64).index_select(1, dev(order)).contiguous()
        ctx.adopt_torch_stream(vs)
        xd, yd, sd = dev(x), dev(y), dev(start)
        host = lambda a: a.cpu().numpy()
    else:
        dev = lambda a: a
        vs = np.ascontiguousarray(v[:, order], dtype=np.float64)
        xd, yd, sd = x, y, start
        host = lambda a: a
    # 2. the slices
    o = _cell_call(ctx, xd, yd, sd, vs, deramp, density_threshold, None, nbins, True if deramp else False, False, on_device)
    status = host(o['status']).copy()
    resid = o['residuals'] if deramp else vs
    # 3. singular planes: the host chain on the slice
    for c, d in zip(*np.nonzero(status == 2)):
        sl = slice(int(start[c]), int(start[c + 1]))
        r = _remove_plane(x[sl], y[sl], host(vs[d, sl]))
        resid[d, sl] = dev(r)
        if sl.stop - sl.start >= 2:
            pv = pair_variogram(x[sl], y[sl], r, nbins=nbins, ctx=ctx)
            for k, a in (('count', pv.count[0]), ('lag_sum', pv.lag_sum[0]), ('gamma_sum', pv.gamma_sum[0]), ('edges', pv.edges[0]), ('hmax', pv.hmax[0:1])):
                o[k][c, d] = dev(a) if k != 'hmax' else dev(a)[0]
    hmax = host(o['hmax'])
    nvalid = host(o['nvalid'])
    good = status != 1
    # 4. one row per cell over its good dates
    with np.errstate(invalid='ignore'):
        top = np.array([np.nanmax(hmax[c][good[c]]) if (good[c] & ~np.isnan(hmax[c])).any() else np.nan for c in range(ng)])
    total_edges = default_edges(top, nbins)
    # 5. the totals
    t = _cell_call(ctx, xd, yd, sd, resid, False, density_threshold, dev(_usable_rows(total_edges)), nbins, False, True, on_device)
    # 6. the fits
    params = np.full((ng, 3), np.nan); rmse = np.full(ng, np.nan)
    has_good = good.any(axis=1)
    sparse = [int(c) for c in full if not has_good[c]]
    skipped = [(int(c), int(d)) for c, d in zip(*np.nonzero((status == 1) & (nvalid > 0)))]
    res = GridVariograms(grid=grid, nvalid=o['nvalid'], hmax=o['hmax'], status=status, count=o['count'], lag_sum=o['lag_sum'], gamma_sum=o['gamma_sum'],
                         edges=o['edges'], total_count=t['total_count'], total_lag=t['total_lag'], total_gamma=t['total_gamma'],
                         total_edges=dev(total_edges), residuals=resid, params=params, rmse=rmse, sparse_grids=sparse, skipped_slices=skipped,
                         date_fits=None, x=x, y=y)
    if fitter == 'device':
        if on_device:
            gd = dev(good)
            mask = lambda a, keep: torch.where(keep, a, torch.full_like(a, np.nan))
        else:
            gd = good
            mask = lambda a, keep: np.where(keep, a, np.nan)
        if fit or per_date_fits:
            ph = mask(_mean_rows(o['lag_sum'], o['count']), gd[:, :, None]); pg = mask(_mean_rows(o['gamma_sum'], o['count']), gd[:, :, None])
        if fit:
            if binned:
                th, tg = ph.reshape(ng, nd * nbins), pg.reshape(ng, nd * nbins)
            else:
                th, tg = _mean_rows(t['total_lag'], t['total_count']), _mean_rows(t['total_gamma'], t['total_count'])
                th = mask(th, dev(has_good)[:, None]); tg = mask(tg, dev(has_good)[:, None])
            f = fit_variograms(th, tg, ctx=ctx)
            params[:] = host(f.params)
            e = host(f.rmse)
            with np.errstate(invalid='ignore'):
                rmse[:] = np.where(e <= errlimit, e, np.nan)
        if per_date_fits:
            res.date_fits = fit_variograms(ph.reshape(ng * nd, nbins), pg.reshape(ng * nd, nbins), ctx=ctx)
        fit = per_date_fits = False            # (done; the maps below)
    if fit or per_date_fits:
        cnt = host(o['count']); lag = host(o['lag_sum']); gam = host(o['gamma_sum'])
        per = lambda c, d: (lag[c, d][cnt[c, d] > 0] / cnt[c, d][cnt[c, d] > 0], gam[c, d][cnt[c, d] > 0] / cnt[c, d][cnt[c, d] > 0])
    if fit:
        tc = host(t['total_count']); tl = host(t['total_lag']); tg = host(t['total_gamma'])
        for c in np.flatnonzero(has_good):
            if binned:
                parts = [per(c, d) for d in np.flatnonzero(good[c])]
                h = np.concatenate([p_[0] for p_ in parts]); g = np.concatenate([p_[1] for p_ in parts])
            else:
                keep = tc[c] > 0
                h = tl[c][keep] / tc[c][keep]; g = tg[c][keep] / tc[c][keep]
            if h.size == 0:
                continue
            f = fit_variogram(h, g, model)
            params[c] = f.params
            e = float(np.sqrt(np.nanmean(f.result.fun ** 2)))
            rmse[c] = e if e <= errlimit else np.nan
    if per_date_fits:
        res.date_fits = {}
        for c, d in zip(*np.nonzero(good)):
            h, g = per(c, d)
            if h.size:
                res.date_fits[(int(c), int(d))] = fit_variogram(h, g, model)
    res.grid_range = res.map(params[:, 0]); res.grid_variance = res.map(params[:, 1]); res.grid_variogram_rmse = res.map(rmse)
    return res
