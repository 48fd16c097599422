"""GPU: exponential variogram models as exact bounded minima (rdr_variogram_fit, csrc/variogram_fit_kernels.h; raider_amd/variogram.py:
fit_variograms and fitter='device' of grid_variograms / station_variograms).

The yardstick is tests/variogram_fit_model.py, run on the test's rows in float64 AND in np.longdouble.  For cost, sill and range, `gap` is
the largest relative |float64 - long double| over the rows of the scene; the device may differ from the long-double model by 16 x gap,
with a floor of 32 x 2^-52 (a sum of up to 64 terms, each through an exp, a square root and a division): it differs from the float64
restatement by a few ulp in exp and the division, by fused multiply-adds, and - for rows of more than 64 columns - by the order of the
sums.  The range is compared on the rows where the model's own float64 and long-double ranges agree to 1e-6: a row on the plateau above
a_floor is flat to round-off in a; at most 20 % of the golden rows may be left out (none is).  n, status and the sill's flags are exact; the
range's flags equal the model's where its two precisions agree, else either's.  The figures are printed before they are asserted.

Observed on the MI355X, device against long double as a share of the tolerance: at most 0.076 over the golden, exact, robust, edge, binned
and n <= 64 scenes, 0.18 (the sill of the M = 1000 scene, whose wide rows add in another order); exact exponentials come back to 6.1e-15
in the range and 3.0e-15 in the sill.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import raider_amd as R                                     # noqa: E402
from raider_amd import _lib as L                           # noqa: E402
from raider_amd import variogram as V                      # noqa: E402
from tests import variogram_fit_model as M                 # noqa: E402

EPS = 2.0 ** -52
FLOOR = 32 * EPS
FIELDS = ('params', 'cost', 'rmse', 'n', 'status', 'flags')


def as_bytes(fit):
    return [np.asarray(a.cpu().numpy() if hasattr(a, 'cpu') else a).tobytes() for a in fit]


def rel(a, b):
    a = np.asarray(a, dtype=np.longdouble); b = np.asarray(b, dtype=np.longdouble)
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.asarray(np.where(a == b, 0, np.abs(a - b) / np.abs(b)), dtype=np.float64)


def compare(got, f64, ld, tag, min_range_share=0.8):
    """the device's rows against the long-double model; tolerances from the float64 model's gap over the scene -> worst error in tolerances"""
    assert np.array_equal(got.n, ld['n']) and np.array_equal(got.status, ld['status']), (tag, got.n, got.status, ld['status'])
    assert np.array_equal(f64['status'], ld['status'])
    ok = ld['status'] == 0
    assert np.isnan(got.params[~ok]).all() and np.isnan(got.cost[~ok]).all() and np.isnan(got.rmse[~ok]).all() and not got.flags[~ok].any(), tag
    if not ok.any():
        return 0.0
    # the sill's flags are exact; the range's where the model's two precisions agree on them, else either's (long double has no plateau at
    # h_pos / 38: its exp(-38) is not below its half-ulp of 1, so a row that float64 puts AT a_floor may sit just above it there)
    both = V.SILL_ZERO | V.SILL_UB
    assert np.array_equal(got.flags[ok] & both, ld['flags'][ok] & both) and np.array_equal(f64['flags'][ok] & both, ld['flags'][ok] & both), (tag, got.flags, ld['flags'])
    assert ((got.flags[ok] == ld['flags'][ok]) | (got.flags[ok] == f64['flags'][ok])).all(), (tag, got.flags, f64['flags'], ld['flags'])
    assert np.array_equal(got.params[ok, 2], np.asarray(ld['params'][ok, 2], dtype=np.float64)), tag
    sure = ok & (rel(f64['params'][:, 0], ld['params'][:, 0]) <= 1e-6)
    assert sure.sum() >= min_range_share * ok.sum(), (tag, sure)
    worst = 0.0
    for name, dev, a, b, rows in (('cost', got.cost, f64['cost'], ld['cost'], ok), ('sill', got.params[:, 1], f64['params'][:, 1], ld['params'][:, 1], ok),
                                  ('rmse', got.rmse, f64['rmse'], ld['rmse'], ok), ('range', got.params[:, 0], f64['params'][:, 0], ld['params'][:, 0], sure)):
        if not rows.any():
            continue
        gap = rel(a, b)[rows].max()
        tol = max(16 * gap, FLOOR)
        err = rel(dev, b)[rows].max()
        print(f'{tag} {name}: float64 model gap {gap:.3e}, device {err:.3e} = {err / tol:.3f} of the tolerance {tol:.3e}')
        assert err <= tol, (tag, name, err, tol)
        worst = max(worst, err / tol)
    return worst


def model_pair(h, g, ub=None):
    return M.fit_rows(h, g, ub=ub), M.fit_rows(h, g, ub=ub, dtype=np.longdouble)


# ---- the golden rows -------------------------------------------------------------------------------------------------------------------
def test_golden_rows_reach_the_model_and_beat_scipy():
    names, h, g, _ = M.golden_rows()
    got = R.fit_variograms(h, g)
    assert got.params.shape == (21, 3) and got.status.dtype == np.int32 and got.n.dtype == np.int64
    compare(got, M.golden_fits(), M.golden_fits(np.longdouble), 'golden')
    for i, name in enumerate(names):
        keep = ~np.isnan(h[i])
        res = V.fit_variogram(h[i][keep], g[i][keep]).result
        assert got.cost[i] <= res.cost * (1 + 1e-9), (name, got.cost[i], res.cost)
    flag = dict(zip(names, got.flags))
    assert flag['g20 c'] & V.AT_UB_A and flag['g21 slice 4/2'] & V.AT_FLOOR and flag['g21 slice 4/3'] & V.AT_FLOOR
    assert flag['g20 b'] & V.SILL_UB and flag['g21 cell 5'] & V.SILL_UB
    d_test, v_test = got.curve(0)
    assert d_test.shape == v_test.shape == (100,) and d_test[-1] == np.nanmax(h[0]) and v_test[0] == 0
    assert np.array_equal(v_test, V.exponential(got.params[0], d_test))


# ---- exact data ------------------------------------------------------------------------------------------------------------------------
def test_exact_exponentials_are_recovered():
    rows = [M.exact_row(a0, b0) for a0, b0 in M.EXACT]
    got = R.fit_variograms(np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), ub=np.array([r[2] for r in rows]))
    assert (got.status == 0).all() and not got.flags.any()
    for (a0, b0), p in zip(M.EXACT, got.params):
        print(f'exact ({a0}, {b0}): range off by {abs(p[0] - a0) / a0:.2e}, sill by {abs(p[1] - b0) / b0:.2e}')
        assert abs(p[0] - a0) <= 1e-9 * a0 and abs(p[1] - b0) <= 1e-9 * b0, (a0, b0, p)


# ---- the robust regime -----------------------------------------------------------------------------------------------------------------
def test_the_loss_is_applied_where_residuals_are_large():
    rng = np.random.default_rng(3)
    h = np.stack([M.exact_row(1.0, 1.0, seed=s)[0] for s in range(4)])
    g = np.array([1.0, 5.0, 30.0, 100.0])[:, None] * (1 - np.exp(-h / 15000.0)) * (1 + 0.05 * rng.standard_normal(h.shape))
    g[:, 7] *= 40.0                                          # one gross outlier per row: z >> 1
    got = R.fit_variograms(h, g)
    f64, ld = model_pair(h, g)
    compare(got, f64, ld, 'robust')
    e = 1 - np.exp(-h / got.params[:, :1])
    plain = (e * g).sum(axis=1) / (e * e).sum(axis=1)       # the least-squares sill at the fitted range
    gap = rel(got.params[:, 1], plain)
    print('robust: sill against the plain least-squares sill', gap)
    assert (gap > 0.1).all()


# ---- status and edge rows ----------------------------------------------------------------------------------------------------------------
def edge_rows():
    nan = np.nan
    h0, g0, _ = M.exact_row(8000.0, 2e-4, n=8, seed=5)
    g0 = g0 * (1 + 0.1 * np.random.default_rng(5).standard_normal(8))
    rows = [(np.full(8, nan), g0),                                                  # 0 all NaN: 1
            (np.where(np.arange(8) % 2 == 0, nan, h0), np.where(np.arange(8) % 2 == 1, nan, g0)),      # 1 no column with both: 1
            (h0, -g0),                                                              # 2 all gamma <= 0: 2
            (np.where(np.arange(8) < 3, 0.0, nan), g0),                             # 3 only h = 0: 3
            (np.where(np.arange(8) == 2, -h0, h0), g0),                             # 4 a negative lag: 2
            (h0, np.where(np.arange(8) == 4, np.inf, g0)),                          # 5 an infinity: 2
            (np.where(np.arange(8) == 5, h0, nan), g0),                             # 6 one present column
            (np.where((np.arange(8) == 1) | (np.arange(8) == 6), h0, nan), g0),     # 7 two present columns
            (h0, np.where(np.arange(8) == 0, 1e-5, -g0)),                           # 8 mixed signs, D(0) >= 0: sill 0
            (h0, g0)]                                                               # 9 a plain row
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows])


def test_status_and_edge_rows():
    h, g = edge_rows()
    got = R.fit_variograms(h, g)
    assert got.status.tolist() == [1, 1, 2, 3, 2, 2, 0, 0, 0, 0] and got.n.tolist() == [0, 0, 8, 3, 8, 8, 1, 2, 8, 8]
    f64, ld = model_pair(h, g)
    compare(got, f64, ld, 'edges', min_range_share=0.5)
    assert got.params[8, 1] == 0 and got.flags[8] == V.SILL_ZERO | V.AT_FLOOR
    # bounds per row
    ub = np.array([[20000.0, 3e-4, 1e-4], [5000.0, 1e-4, 7.0], [np.inf, 1e-4, 1.0], [9000.0, 0.0, 1.0], [100.0, 1e-3, 1.0]])
    hh, gg = np.tile(h[9], (5, 1)), np.tile(g[9], (5, 1))
    got = R.fit_variograms(hh, gg, ub=ub)
    assert got.status.tolist() == [0, 0, 2, 2, 0]
    f64, ld = model_pair(hh, gg, ub)
    compare(got, f64, ld, 'given bounds')
    assert got.params[0, 2] == 5e-5 and got.params[1, 2] == 3.5 and (got.params[[0, 1, 4], 0] <= ub[[0, 1, 4], 0]).all()
    assert got.flags[4] & V.AT_UB_A                         # (ub_a = 100 m lies below a_floor: the single candidate)


# ---- shapes ----------------------------------------------------------------------------------------------------------------------------
POOL = 6


@functools.lru_cache(maxsize=None)
def pool(m):
    """six rows of m columns with a different number of present columns each -> (h, gamma, model float64, model long double)"""
    rng = np.random.default_rng(100 + m)
    present = {1: [1, 0, 1, 1, 0, 1], 19: [19, 1, 2, 7, 18, 12], 64: [64, 63, 1, 33, 64, 20], 65: [65, 64, 63, 65, 2, 40], 1000: [300, 64, 65, 19, 0, 130]}[m]
    h = np.full((POOL, m), np.nan); g = np.full((POOL, m), np.nan)
    for r, n in enumerate(present):
        cols = np.sort(rng.choice(m, n, replace=False))
        lag = np.sort(rng.uniform(500.0, 80000.0, n))
        h[r, cols] = lag
        g[r, cols] = rng.uniform(1e-4, 4e-4) * (1 - np.exp(-lag / rng.uniform(3000.0, 30000.0))) * (1 + 0.1 * rng.standard_normal(n))
    h.setflags(write=False); g.setflags(write=False)
    return (h, g) + model_pair(h, g) + (present,)


@pytest.mark.parametrize('m', [1, 19, 64, 65, 1000])
def test_shapes_rows_and_bytes(m):
    import torch
    h, g, f64, ld, present = pool(m)
    base = R.fit_variograms(h, g)
    assert base.n.tolist() == present
    compare(base, f64, ld, f'M = {m}', min_range_share=0.6)
    want = as_bytes(base)
    assert as_bytes(R.fit_variograms(h, g)) == want                                                  # two runs
    dev = R.fit_variograms(torch.from_numpy(np.array(h)).cuda(), torch.from_numpy(np.array(g)).cuda())
    assert all(a.is_cuda for a in dev) and as_bytes(dev) == want                                     # host arrays and device tensors
    one = R.fit_variograms(h[0], g[0])                                                               # F = 1, from [M]
    assert [a.shape[0] for a in one] == [1] * 6 and as_bytes(one) == [np.asarray(a[:1]).tobytes() for a in base]
    for nf in (4, 257):                                                                              # a row's bytes do not depend on the batch
        idx = np.random.default_rng(nf).permutation(np.arange(nf) % POOL)
        got = R.fit_variograms(h[idx], g[idx])
        assert as_bytes(got) == [np.asarray(a[idx]).tobytes() for a in base], (m, nf)


# ---- the drivers -----------------------------------------------------------------------------------------------------------------------
def test_grid_variograms_with_the_device_fitter():
    g = np.load(M.GOLDEN / 'g21_grid_variogram.npz')
    gv = V.grid_variograms(g['lon'], g['lat'], g['values'], fitter='device', per_date_fits=True)
    good = g['slice_state'] == 1
    cells = np.flatnonzero(good.any(axis=1))
    for c in range(6):
        if c in cells:
            one = R.fit_variograms(*gv.total_binned(c))
            assert one.params.tobytes() == gv.params[c].tobytes() and one.rmse.tobytes() == gv.rmse[c].tobytes(), c
        else:
            assert np.isnan(gv.params[c]).all() and np.isnan(gv.rmse[c])
    for got, want in ((gv.grid_range, g['map_range']), (gv.grid_variance, g['map_variance']), (gv.grid_variogram_rmse, g['map_rmse'])):
        assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    assert isinstance(gv.date_fits, V.VariogramFits) and gv.date_fits.status.shape == (30,)
    assert np.array_equal(gv.date_fits.status.reshape(6, 5) == 0, good) and (gv.date_fits.status[~good.reshape(-1)] == 1).all()
    for c, d in zip(*np.nonzero(good)):
        one = R.fit_variograms(*gv.binned(c, d))
        assert one.params.tobytes() == gv.date_fits.params[c * 5 + d].tobytes(), (c, d)
    assert np.isnan(V.grid_variograms(g['lon'], g['lat'], g['values'], fitter='device', errlimit=1e-9).rmse).all()
    # binned=True: the per-date bins side by side, 4 good dates x 19 bins in cells 4 and 5 - more than 64 columns
    gb = V.grid_variograms(g['lon'], g['lat'], g['values'], fitter='device', binned=True)
    keep = good[:, :, None] & (gv.count > 0)
    rows_h = np.where(keep, gv.lag_sum / np.maximum(gv.count, 1), np.nan).reshape(6, 95)
    rows_g = np.where(keep, gv.gamma_sum / np.maximum(gv.count, 1), np.nan).reshape(6, 95)
    f64, ld = model_pair(rows_h, rows_g)
    assert (ld['n'] > 64).sum() >= 2
    got = R.fit_variograms(rows_h, rows_g)
    assert got.params.tobytes() == gb.params.tobytes()
    compare(got, f64, ld, 'binned', min_range_share=0.5)      # (four fitted rows; cell 4 lies on the plateau, as its slices 4/2 and 4/3 do)


def test_station_variograms_with_the_device_fitter():
    g = np.load(M.GOLDEN / 'g20_variogram.npz')
    rng = np.random.default_rng(11)
    lon = rng.uniform(-118.9, -118.1, 40); lat = rng.uniform(33.1, 33.9, 40)
    v = np.stack([g['a_values'], g['b_values'], g['c_values'], np.where(np.arange(40) < 9, g['a_values'], np.nan)])
    sv = V.station_variograms(lon, lat, v, fitter='device')
    assert isinstance(sv.fits, V.VariogramFits) and sv.fits.status.tolist() == [0, 0, 0, 1]
    for d in range(3):
        one = R.fit_variograms(*sv.binned[d])
        assert one.params.tobytes() == sv.fits.params[d].tobytes() and one.cost.tobytes() == sv.fits.cost[d].tobytes()
        res = V.fit_variogram(*sv.binned[d]).result
        assert sv.fits.cost[d] <= res.cost * (1 + 1e-9)
    assert V.station_variograms(lon, lat, v, fitter='device', fit=False).fits is None


def test_the_device_fitter_refuses_other_models():
    g = np.load(M.GOLDEN / 'g21_grid_variogram.npz')
    with pytest.raises(ValueError, match='exponential model only'):
        V.grid_variograms(g['lon'], g['lat'], g['values'], fitter='device', model='gaussian')
    with pytest.raises(ValueError, match='exponential model only'):
        V.station_variograms(g['lon'], g['lat'], g['values'], fitter='device', model='gaussian')
    with pytest.raises(ValueError, match="fitter must be 'scipy' or 'device'"):
        V.grid_variograms(g['lon'], g['lat'], g['values'], fitter='host')


# ---- argument errors -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loc', [L.RDR_HOST, L.RDR_DEVICE])
def test_refusals_leave_the_outputs_untouched(loc):
    import torch
    ctx = R.Context.default()
    nf, m = 3, 19
    _, h, g, _ = M.golden_rows()
    arrays = dict(h=np.array(h[:nf]), g=np.array(g[:nf]), ub=np.tile([3e4, 1e-3, 1e-3], (nf, 1)), params=np.full((nf, 3), -7.0), cost=np.full(nf, -7.0),
                  rmse=np.full(nf, -7.0), n=np.full(nf, -7, np.int64), status=np.full(nf, -7, np.int32), flags=np.full(nf, -7, np.int32))
    if loc == L.RDR_DEVICE:
        bufs = {k: torch.from_numpy(a).cuda() for k, a in arrays.items()}
        torch.cuda.synchronize()
        read = lambda k: bufs[k].cpu().numpy()
    else:
        bufs = {k: a.copy() for k, a in arrays.items()}
        read = lambda k: bufs[k]

    def vf(h_='h', g_='g', nf_=nf, m_=m, ub_='ub', s_=0.1, k_=512, params_='params', cost_='cost', rmse_='rmse', n_='n', status_='status', flags_='flags', loc_=loc):
        p = lambda k: None if k is None else L.ptr(bufs[k])
        return ctx.lib.rdr_variogram_fit(ctx.handle, p(h_), p(g_), nf_, m_, p(ub_), s_, k_, p(params_), p(cost_), p(rmse_), p(n_), p(status_), p(flags_), loc_)
    for kw, text in ((dict(h_=None), 'NULL argument'), (dict(g_=None), 'NULL argument'), (dict(params_=None), 'NULL argument'), (dict(cost_=None), 'NULL argument'),
                     (dict(rmse_=None), 'NULL argument'), (dict(n_=None), 'NULL argument'), (dict(status_=None), 'NULL argument'), (dict(flags_=None), 'NULL argument'),
                     (dict(loc_=2), 'loc must be RDR_HOST or RDR_DEVICE'), (dict(loc_=-1), 'loc must be RDR_HOST or RDR_DEVICE'),
                     (dict(nf_=0), 'nfits must be 1 .. 2^22 rows (got 0)'), (dict(nf_=-1), 'nfits must be 1 .. 2^22 rows (got -1)'),
                     (dict(nf_=(1 << 22) + 1), 'nfits must be 1 .. 2^22 rows'), (dict(m_=0), 'm must be 1 .. 65536 columns (got 0)'),
                     (dict(m_=65537), 'm must be 1 .. 65536 columns (got 65537)'), (dict(nf_=1 << 22, m_=65536), 'nfits x m must not exceed 2^30 values'),
                     (dict(s_=0.0), 'f_scale must be finite and > 0'), (dict(s_=-0.1), 'f_scale must be finite and > 0'),
                     (dict(s_=float('nan')), 'f_scale must be finite and > 0'), (dict(s_=float('inf')), 'f_scale must be finite and > 0'),
                     (dict(k_=0), 'k_scan must be a multiple of 64 in 64 .. 4096 (got 0)'), (dict(k_=100), 'k_scan must be a multiple of 64 in 64 .. 4096 (got 100)'),
                     (dict(k_=4160), 'k_scan must be a multiple of 64 in 64 .. 4096 (got 4160)')):
        assert vf(**kw) == L.RDR_ERR_INVALID, kw
        assert text in L.last_error(ctx.handle), (text, L.last_error(ctx.handle))
    ctx.synchronize()
    for k in ('params', 'cost', 'rmse', 'n', 'status', 'flags'):          # the sentinels are still there
        assert (read(k) == -7).all(), k
    assert vf() == L.RDR_OK and vf(ub_=None, k_=64) == L.RDR_OK
    ctx.synchronize()
    assert (read('status') == 0).all() and (read('n') == 19).all()
    with pytest.raises(ValueError, match='k_scan'):
        R.fit_variograms(arrays['h'], arrays['g'], k_scan=100)
    with pytest.raises(ValueError, match='same shape'):
        R.fit_variograms(arrays['h'], arrays['g'][:, :5])
    with pytest.raises(TypeError):
        R.fit_variograms(torch.from_numpy(arrays['h']).cuda(), arrays['g'])
