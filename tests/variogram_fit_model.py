"""A NumPy restatement of rdr_variogram_fit (csrc/variogram_fit_kernels.h), in float64 or np.longdouble - the yardstick of the variogram-fit
tests.  Not a test module.  It restates the contract of include/raider_hip.h, not the kernels' code: one row at a time, the
range candidates of a round as one array, every sum over the row's present columns in column order (np.cumsum).

    fit_row(h, gamma, ub=None, f_scale=0.1, k_scan=512, dtype=np.float64) -> dict(params [3], cost, rmse, n, status, flags)
    fit_rows(h [F, M], gamma [F, M], ub=None or [F, 3], ...)             -> the same, stacked over the rows
    cost_at(h, gamma, a, b, f_scale=0.1, dtype=np.float64)               -> C(a, b) of the contract, for any (a, b)
    golden_rows()                                                        -> the 21 fit inputs that goldens g20 and g21 record
"""
import functools
from pathlib import Path

import numpy as np

ROUNDS = 8                # refinement rounds
FINE = 64                 # candidates of a refinement round
HALVINGS = 64             # bisection steps at most
FLOOR_DIV = 38.0          # exp(-38) < 2^-54: below h_pos / 38 every e of a positive lag is exactly 1
AT_FLOOR, AT_UB_A, SILL_ZERO, SILL_UB = 1, 2, 4, 8
GOLDEN = Path(__file__).resolve().parent / 'golden'


def _sum(x):
    """the sum of x along axis 0, added in that order"""
    return np.cumsum(x, axis=0)[-1]


def _e(h, a):
    """e [n, C] = 1 - exp(-h / a) for lags h [n] and ranges a [C]"""
    return 1 - np.exp(-h[:, None] / a[None, :])


def _cost(e, g, b, s, inv_s):
    """C [C] for e [n, C], gamma g [n], sills b [C]: s^2 sum z / (sqrt(1 + z) + 1)"""
    r = b[None, :] * e - g[:, None]
    z = (r * inv_s) ** 2
    return s * s * _sum(z / (np.sqrt(1 + z) + 1))


def _slope(e, g, b, inv_s):
    """D [C] = sum e r / sqrt(1 + z): dC / db"""
    r = b[None, :] * e - g[:, None]
    z = (r * inv_s) ** 2
    return _sum(e * r / np.sqrt(1 + z))


def _sill(e, g, ub_b, inv_s):
    """the sill of least cost in [0, ub_b] per candidate column of e -> b [C]"""
    dtype = e.dtype.type
    nc = e.shape[1]
    lo = np.zeros(nc, dtype); hi = np.full(nc, ub_b, dtype)
    at0 = _slope(e, g, lo, inv_s) >= 0
    at1 = ~at0 & (_slope(e, g, hi, inv_s) <= 0)
    tol = dtype(2.0 ** -52) * ub_b
    for _ in range(HALVINGS):
        act = ~at0 & ~at1 & ((hi - lo) > tol)
        if not act.any():
            break
        mid = (lo + hi) / 2
        up = _slope(e, g, mid, inv_s) > 0
        hi = np.where(act & up, mid, hi); lo = np.where(act & ~up, mid, lo)
    return np.where(at0, dtype(0), np.where(at1, ub_b, (lo + hi) / 2)), at0, at1


def _geometric(lo, hi, k):
    """k candidates from lo to hi, both included exactly"""
    dtype = type(lo)
    if k == 1:
        return np.array([hi], dtype)
    step = np.log(hi / lo) / dtype(k - 1)
    a = lo * np.exp(np.arange(k).astype(dtype) * step)
    a[0] = lo; a[-1] = hi
    return a


def cost_at(h, gamma, a, b, f_scale=0.1, dtype=np.float64):
    h = np.asarray(h, dtype=np.float64); g = np.asarray(gamma, dtype=np.float64)
    keep = ~(np.isnan(h) | np.isnan(g))
    h = h[keep].astype(dtype); g = g[keep].astype(dtype)
    s = dtype(f_scale)
    with np.errstate(divide='ignore', over='ignore'):
        e = _e(h, np.array([a], dtype))
    return _cost(e, g, np.array([b], dtype), s, 1 / s)[0]


def fit_row(h, gamma, ub=None, f_scale=0.1, k_scan=512, dtype=np.float64):
    h = np.asarray(h, dtype=np.float64).reshape(-1); g = np.asarray(gamma, dtype=np.float64).reshape(-1)
    keep = ~(np.isnan(h) | np.isnan(g))
    h = h[keep]; g = g[keep]
    nan = dtype(np.nan)
    out = dict(params=np.full(3, nan, dtype), cost=nan, rmse=nan, n=int(h.size), status=0, flags=0)
    if h.size == 0:
        out['status'] = 1
        return out
    if ub is None:
        ub = np.array([0.8 * h.max(), 0.8 * g.max(), 0.8 * g.max()])
    ub = np.asarray(ub, dtype=np.float64)
    if np.isinf(h).any() or np.isinf(g).any() or (h < 0).any():
        out['status'] = 2
        return out
    if not (h > 0).any():
        out['status'] = 3
        return out
    if not (np.isfinite(ub[0]) and np.isfinite(ub[1]) and ub[0] > 0 and ub[1] > 0):
        out['status'] = 2
        return out
    ub_a, ub_b = dtype(ub[0]), dtype(ub[1])
    s = dtype(f_scale); inv_s = 1 / s
    a_floor = dtype(h[h > 0].min()) / dtype(FLOOR_DIV)
    h = h.astype(dtype); g = g.astype(dtype)

    def evaluate(cand):
        e = _e(h, cand)
        b, at0, at1 = _sill(e, g, ub_b, inv_s)
        c = _cost(e, g, b, s, inv_s)
        c = np.where(np.isnan(c), dtype(np.inf), c)
        k = int(np.argmin(c))                       # (the first of equal minima)
        return k, c[k], b[k], bool(at0[k]), bool(at1[k])

    cand = _geometric(a_floor, ub_a, k_scan) if ub_a > a_floor else np.array([ub_a], dtype)
    k, best_c, best_b, at0, at1 = evaluate(cand)
    best_a = cand[k]
    if cand.size > 1:
        for _ in range(ROUNDS):
            lo, hi = cand[max(k - 1, 0)], cand[min(k + 1, cand.size - 1)]
            cand = _geometric(lo, hi, FINE)
            k, c, b, z0, z1 = evaluate(cand)
            if c < best_c:
                best_c, best_b, best_a, at0, at1 = c, b, cand[k], z0, z1
    r = best_b * (1 - np.exp(-h / best_a)) - g
    out['params'] = np.array([best_a, best_b, dtype(ub[2]) / 2], dtype)
    out['cost'] = best_c
    out['rmse'] = np.sqrt(_sum(r * r) / dtype(h.size))
    # "at" a bound: within 2^-40 of it - the last round's candidates lie a few ulp apart and their costs are equal to round-off
    near = dtype(2.0 ** -40)
    out['flags'] = ((AT_FLOOR if best_a <= a_floor + near * a_floor else 0) | (AT_UB_A if best_a >= ub_a - near * ub_a else 0) | (SILL_ZERO if at0 else 0)
                    | (SILL_UB if at1 else 0))
    return out


def fit_rows(h, gamma, ub=None, f_scale=0.1, k_scan=512, dtype=np.float64):
    h = np.atleast_2d(np.asarray(h, dtype=np.float64)); g = np.atleast_2d(np.asarray(gamma, dtype=np.float64))
    rows = [fit_row(h[f], g[f], None if ub is None else np.asarray(ub, dtype=np.float64).reshape(-1, 3)[f], f_scale, k_scan, dtype) for f in range(h.shape[0])]
    return dict(params=np.stack([r['params'] for r in rows]), cost=np.array([r['cost'] for r in rows], dtype), rmse=np.array([r['rmse'] for r in rows], dtype),
                n=np.array([r['n'] for r in rows], np.int64), status=np.array([r['status'] for r in rows], np.int32),
                flags=np.array([r['flags'] for r in rows], np.int32))


def golden_rows():
    """(names [21], h [21, 19], gamma [21, 19], recorded fit [21, 3] or NaN): g20's a, b, c; g21's cells with a total fit; g21's slices with a
    binned variogram.  Empty bins are NaN."""
    g20 = np.load(GOLDEN / 'g20_variogram.npz'); g21 = np.load(GOLDEN / 'g21_grid_variogram.npz')
    names, hs, gs, fits = [], [], [], []
    for k in 'abc':
        names.append(f'g20 {k}'); hs.append(g20[f'{k}_hexp']); gs.append(g20[f'{k}_vexp']); fits.append(g20[f'{k}_fit'])
    for c in g21['tot_grids']:
        names.append(f'g21 cell {c}'); hs.append(g21['tot_hexp'][c]); gs.append(g21['tot_vexp'][c]); fits.append(g21['tot_fit'][c])
    for c, d in zip(*np.nonzero(~np.isnan(g21['slice_hexp']).all(axis=2))):
        names.append(f'g21 slice {c}/{d}'); hs.append(g21['slice_hexp'][c, d]); gs.append(g21['slice_vexp'][c, d]); fits.append(np.full(3, np.nan))
    return names, np.array(hs), np.array(gs), np.array(fits)


@functools.lru_cache(maxsize=None)
def golden_fits(dtype=np.float64, k_scan=512):
    """fit_rows on the 21 golden rows, computed once per (dtype, k_scan) and shared by the tests; read only"""
    _, h, g, _ = golden_rows()
    out = fit_rows(h, g, k_scan=k_scan, dtype=dtype)
    for a in out.values():
        a.setflags(write=False)
    return out


def exact_row(a0, b0, n=19, seed=0):
    """gamma = b0 (1 - exp(-h / a0)) on n jittered lags up to about 60 km -> (h, gamma, ub = (2 max h, 2 max gamma, 2 max gamma))"""
    rng = np.random.default_rng(seed)
    h = (np.arange(n) + rng.uniform(0.2, 0.8, n)) * (60000.0 / n)
    g = b0 * (1 - np.exp(-h / a0))
    return h, g, np.array([2 * h.max(), 2 * g.max(), 2 * g.max()])


EXACT = ((5000.0, 3e-4), (30000.0, 1e-3), (900.0, 2e-4), (20000.0, 40.0))
