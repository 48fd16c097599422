"""A NumPy restatement of rdr_seasonal_fit (csrc/seasonal_kernels.h), in float64 or np.longdouble - the yardstick of the seasonal tests and
of tools/gen_golden_seasonal.py.  Not a test module.  It restates the DESIGN, not the kernels' code: the same sums, closed form, grid
argmin, golden-section rule and Jacobian, written with array operations per station; every sum runs in date order (np.cumsum).

    restate(t, v, omega, scan, min_span, min_frac, dtype) -> {row name: [N]} in `dtype`, the rows of the station block
    ref_columns(res, scan)                                 -> the reference's seven columns, with its labels
    cell_means(cols, nobs, fitted, start)                  -> [14, G]
"""
import numpy as np

YEAR = 31556952.0
GOLD = 0.6180339887498949
MAXIT = 64
ROWS = ('nobs', 'span_years', 'fitted', 'at_edge', 'amplitude', 'phase', 'offset', 'omega', 'rss', 'rmse', 'sigma_amplitude', 'sigma_omega',
        'sigma_phase', 'sigma_offset', 'kstar', 'iterations')
REF_COLUMNS = ('phsfit', 'ampfit', 'periodfit', 'phsfit_c', 'ampfit_c', 'periodfit_c', 'seasonalfit_rmse')


def _sum(x):
    """the sum of x along axis 0, added in that order"""
    return np.cumsum(x, axis=0)[-1]


def _pi(dtype):
    return 4 * np.arctan(dtype(1))


def _solve(n, s, c, ss, sc, ys, yc, sy, syy):
    """(a, b, c, R) of the closed form for arrays of sums; R = inf where the system is singular"""
    cc = n - ss
    Sss, Ssc, Scc = ss - s * s / n, sc - s * c / n, cc - c * c / n
    Sys, Syc, Syy = ys - s * sy / n, yc - c * sy / n, syy - sy * sy / n
    det = Sss * Scc - Ssc * Ssc
    ok = det > 0
    det = np.where(ok, det, 1)
    a = (Sys * Scc - Syc * Ssc) / det
    b = (Syc * Sss - Sys * Ssc) / det
    c0 = (sy - a * s - b * c) / n
    R = Syy - a * Sys - b * Syc
    R = np.where(R > 0, R, 0)
    return a, b, c0, np.where(ok, R, np.inf)


def _evaluate(tau, y, w):
    """the fit of one station (its valid rows: tau, y relative to the mean) at the frequencies w [K] -> (a, b, c, R) [K]"""
    ph = tau[:, None] * np.atleast_1d(w)[None, :]
    sn, cs = np.sin(ph), np.cos(ph)
    yy = y[:, None]
    n = type(y[0])(y.size)
    return _solve(n, _sum(sn), _sum(cs), _sum(sn * sn), _sum(sn * cs), _sum(yy * sn), _sum(yy * cs), _sum(y), _sum(y * y))


def _invert(M):
    """the inverse of a symmetric positive definite matrix in its own dtype: unit-diagonal scaling, Gauss-Jordan"""
    P = M.shape[0]
    sc = 1 / np.sqrt(np.diag(M))
    M = M * sc[:, None] * sc[None, :]
    inv = np.eye(P, dtype=M.dtype)
    M = M.copy()
    for p in range(P):
        ip = 1 / M[p, p]
        M[p] = M[p] * ip; inv[p] = inv[p] * ip
        for i in range(P):
            if i != p:
                f = M[i, p]
                M[i] = M[i] - f * M[p]; inv[i] = inv[i] - f * inv[p]
    return inv * sc[:, None] * sc[None, :]


def restate(t, v, omega, scan, min_span, min_frac, dtype=np.float64):
    t = np.asarray(t, dtype=np.float64); v = np.asarray(v, dtype=np.float64)
    v = v if v.ndim == 2 else v[None, :]
    omega = np.asarray(omega, dtype=np.float64)
    nd, N = v.shape
    K = omega.size
    P = 4 if scan else 3
    t_ref = 0.5 * (t.min() + t.max())
    tau_all = (t - t_ref).astype(dtype)
    t_ref = dtype(t_ref)
    wgrid = omega.astype(dtype)
    pi = _pi(dtype)
    out = {k: np.full(N, np.nan, dtype=dtype) for k in ROWS}
    out['fitted'][:] = 0; out['at_edge'][:] = 0
    with np.errstate(all='ignore'):
        for i in range(N):
            ok = ~np.isnan(v[:, i])
            m = int(ok.sum())
            out['nobs'][i] = m
            if m == 0:
                continue
            tau = tau_all[ok]
            span = (tau.max() - tau.min()) / dtype(YEAR)
            out['span_years'][i] = span
            if not (m >= P + 1 and span >= min_span and dtype(m) / (span * dtype(365.25)) >= min_frac):
                continue
            col = v[ok, i].astype(dtype)
            mean = _sum(col) / dtype(m)
            y = col - mean
            iters = 0
            kstar = np.nan; edge = 0
            if scan:
                R = _evaluate(tau, y, wgrid)[3]
                if not np.isfinite(R).any():
                    continue
                ks = int(np.argmin(R))                       # (the first of equal minima)
                kstar = ks; edge = int(ks == 0 or ks == K - 1)
                w = wgrid[ks]
                best = [q[0] for q in _evaluate(tau, y, w)]
                lo, hi = wgrid[max(ks - 1, 0)], wgrid[min(ks + 1, K - 1)]
                tol = dtype(1e-10) * (wgrid[1] - wgrid[0]) if K > 1 else dtype(0)
                g = dtype(GOLD)
                if hi - lo >= tol and hi > lo:
                    x1, x2 = hi - g * (hi - lo), lo + g * (hi - lo)
                    f1 = [q[0] for q in _evaluate(tau, y, x1)]; f2 = [q[0] for q in _evaluate(tau, y, x2)]
                    if f1[3] < best[3]:
                        best, w = f1, x1
                    if f2[3] < best[3]:
                        best, w = f2, x2
                    while iters < MAXIT and hi - lo >= tol and f1[3] != f2[3]:
                        iters += 1
                        if f1[3] < f2[3]:
                            hi = x2; x2 = x1; f2 = f1; x1 = hi - g * (hi - lo)
                            f1 = [q[0] for q in _evaluate(tau, y, x1)]
                            if f1[3] < best[3]:
                                best, w = f1, x1
                        else:
                            lo = x1; x1 = x2; f1 = f2; x2 = lo + g * (hi - lo)
                            f2 = [q[0] for q in _evaluate(tau, y, x2)]
                            if f2[3] < best[3]:
                                best, w = f2, x2
            else:
                w = wgrid[0]
                best = [q[0] for q in _evaluate(tau, y, w)]
            a, b, c0, R = best
            if not np.isfinite(R):
                continue
            amp = np.hypot(a, b); pc = np.arctan2(b, a)
            sn, cs = np.sin(w * tau), np.cos(w * tau)
            u = (a * sn + b * cs) / amp; vv = a * cs - b * sn; ww = (tau / dtype(YEAR)) * vv
            one = np.ones_like(u)
            cols = [u, ww, vv, one] if scan else [u, vv, one]
            M = np.array([[_sum(p * q) for q in cols] for p in cols], dtype=dtype)
            inv = _invert(M)
            s2 = R / dtype(m - P)
            if scan:
                ty = t_ref / dtype(YEAR)
                sA = np.sqrt(s2 * inv[0, 0]); sW = np.sqrt(s2 * inv[1, 1]) / dtype(YEAR)
                sP = np.sqrt(s2 * (inv[2, 2] - 2 * ty * inv[1, 2] + ty * ty * inv[1, 1])); sC = np.sqrt(s2 * inv[3, 3])
            else:
                sA, sW, sP, sC = np.sqrt(s2 * inv[0, 0]), dtype(np.nan), np.sqrt(s2 * inv[1, 1]), np.sqrt(s2 * inv[2, 2])
            x = pc - w * t_ref
            p = x - 2 * pi * np.rint(x / (2 * pi))
            if p <= -pi:
                p += 2 * pi
            if p > pi:
                p -= 2 * pi
            rmse = np.sqrt(R / dtype(m - 2)); off = mean + c0
            vals = [amp, p, off, rmse, sA, sP, sC] + ([sW] if scan else [])
            if not all(np.isfinite(q) for q in vals):
                continue
            for k, q in zip(ROWS[2:], (1, edge, amp, p, off, w, R, rmse, sA, sW, sP, sC, kstar, iters)):
                out[k][i] = q
    return out


def ref_columns(res, scan):
    """the reference's seven columns of a station block (a dict of rows), with the reference's labels for the three *_c"""
    dtype = res['phase'].dtype.type
    two_pi = 2 * _pi(dtype) if dtype is not np.float64 else 2.0 * np.pi
    return dict(phsfit=(dtype(365.25) / 2) * np.sin(res['phase']), ampfit=res['amplitude'], periodfit=1 / ((res['omega'] / two_pi) * dtype(YEAR)),
                phsfit_c=res['sigma_phase'] if scan else res['sigma_offset'], ampfit_c=res['sigma_amplitude'],
                periodfit_c=res['sigma_omega'] if scan else res['sigma_phase'], seasonalfit_rmse=res['rmse'])


def cell_means(cols, nobs, fitted, start):
    """[14, G]: per cell the plain mean of each reference column over its fitted stations, then the mean weighted by their row counts;
    stations sorted by cell (start [G + 1]), added in station order"""
    G = len(start) - 1
    dtype = cols['ampfit'].dtype
    out = np.full((2 * len(REF_COLUMNS), G), np.nan, dtype=dtype)
    for g in range(G):
        idx = [s for s in range(int(start[g]), int(start[g + 1])) if fitted[s] != 0]
        if not idx:
            continue
        rows = nobs[idx].astype(dtype)
        for c, name in enumerate(REF_COLUMNS):
            x = cols[name][idx]
            out[c, g] = np.cumsum(x)[-1] / dtype.type(len(idx))
            out[len(REF_COLUMNS) + c, g] = np.cumsum(rows * x)[-1] / np.cumsum(rows)[-1]
    return out


def angle_gap(a, b):
    """|a - b| of two angles, on the circle"""
    d = np.asarray(a - b, dtype=np.float64)
    return np.abs((d + np.pi) % (2 * np.pi) - np.pi)
