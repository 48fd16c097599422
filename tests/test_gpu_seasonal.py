"""GPU: the seasonal fits (rdr_seasonal_fit, csrc/seasonal_kernels.h; raider_amd/seasonal.py: seasonal_fits, grid_seasonal).

The yardstick is tests/seasonal_model.py, run on the test's inputs in float64 AND in np.longdouble.  Per column, `gap` is the largest
|float64 - long double| over the stations; the device may differ from the long-double column by 16 x gap: it differs from the float64
restatement only in the order of a few sums and a few ulp in sin / cos.  Counts, the fitted flags and the NaN masks are exact.  (A
scanned frequency is determined to about sqrt(eps) of a grid step only - R(w) is flat to round-off at its minimum -, which the gap of
the omega column measures.)  The figures are printed before they are asserted.

Golden g23 (tools/gen_golden_seasonal.py: the reference's own RaiderStats run):
  fixed period   the seven station columns and the fourteen maps within 2 x (the recorded largest |reference - restatement| of the column)
                 + the device allowance above; a map, a mean of at most 3 stations weighted by at most 2280 rows, gets 8 * 2^-53 relative
                 on top for the roundings of the mean itself (k + 2 for k terms, the products, the division).
  free period    the stations where the reference reached the least-squares minimum agree in the same way; at EVERY fitted station the
                 device's residual sum is at most the reference's times (1 + 1e-9).

Shapes (one scene of 130 stations per D; a smaller N takes its first columns): N = 1, 64, 65, 130 (one lane, a full wave, one lane of a second workgroup, three workgroups), D = 1, 2 (nobody is fitted), 40, 77
(the tail of the four-date unrolling); K = 1, 7, 9 (SF_KT = 8: one frequency, a tile less one, a tile and one) and 41; columns with holes
only at the start, only at the end, alternating, an all-NaN column between fitted ones; a line below the band (k* = 0: at_edge) and a line
exactly between two grid frequencies; cells with zero, one and several fitted stations; 131072 stations (2048 workgroups: the scan's
frequency tiles are then cut into segments of two) as 1024 copies of 128 columns, which must repeat the small call's bytes.
"""
import functools
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import raider_amd as R                                     # noqa: E402
from raider_amd import _lib as L                           # noqa: E402
from raider_amd import seasonal as S                       # noqa: E402
from tests import seasonal_model as M                      # noqa: E402

GOLDEN = Path(__file__).resolve().parent / 'golden' / 'g23_seasonal.npz'
DAY = 86400.0
U = 2.0 ** -53
KT = 8                                                     # SF_KT of csrc/seasonal_kernels.h
ELIG = dict(min_span=0.05, min_frac=0.3)
COLUMNS = ('span_years', 'amplitude', 'phase', 'offset', 'omega', 'rss', 'rmse', 'sigma_amplitude', 'sigma_omega', 'sigma_phase', 'sigma_offset')
BYTES = ('nobs', 'span_years', 'fitted', 'at_edge', 'amplitude', 'phase', 'offset', 'omega', 'period', 'frequency', 'rss', 'rmse', 'sigma_amplitude',
         'sigma_phase', 'sigma_offset', 'sigma_omega', 'sigma_frequency', 'kstar', 'iterations')


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------
def band(t, k, first=3.0):
    """(lo, hi) years such that the scan over the axis t has exactly k frequencies, the first `first` cycles per span"""
    span = max(t.max() - t.min(), DAY)
    delta = 2 * np.pi / (8 * span)
    w_lo = 2 * np.pi * first / span
    return 2 * np.pi / ((w_lo + (k - 0.5) * delta) * S.YEAR), 2 * np.pi / (w_lo * S.YEAR)


NFULL = 130


def scene(n, nd):
    """the first n columns of full_scene(nd)"""
    t, v = full_scene(nd)
    return t, v[:, :n]


@functools.lru_cache(maxsize=None)
def full_scene(nd, n=NFULL, seed=1):
    """t [nd] daily, v [nd, n]: a line of 3.5375 cycles per span (grid index 4.3 of band(t, k)) of amplitude 0.5 on 2.0 with noise 0.05;
    column 0 lacks its first dates, 1 its last, 2 every other date, 3 is all NaN, 5's line lies two grid steps BELOW the band, 6's exactly
    between grid frequencies 3 and 4; the others have 20 % holes"""
    rng = np.random.default_rng(seed)
    t = 1.6e9 + DAY * np.arange(nd, dtype=np.float64)
    span = max(t.max() - t.min(), DAY)
    cyc = np.full(n, 3.0 + 4.3 / 8)
    if n > 6:
        cyc[5] = 3.0 - 2.0 / 8; cyc[6] = 3.0 + 3.5 / 8
    ph = rng.uniform(-np.pi, np.pi, n)
    v = 2.0 + 0.5 * np.sin(2 * np.pi * cyc[None, :] * (t[:, None] - t[0]) / span + ph[None, :]) + 0.05 * rng.standard_normal((nd, n))
    v[rng.uniform(size=(nd, n)) < 0.2] = np.nan
    if n > 3:
        v[:, :3] = 2.0 + 0.5 * np.sin(2 * np.pi * cyc[None, :3] * (t[:, None] - t[0]) / span + ph[None, :3]) + 0.05 * rng.standard_normal((nd, 3))
        v[:nd // 4, 0] = np.nan; v[nd - nd // 4:, 1] = np.nan; v[1::2, 2] = np.nan; v[:, 3] = np.nan
    t.setflags(write=False); v.setflags(write=False)
    return t, v


@functools.lru_cache(maxsize=None)
def model(nd, k, dtype):
    """the yardstick on full_scene(nd), computed once: k = 0 is the fixed period of 3.5375 cycles per span, k > 0 the scan of band(t, k)"""
    t, v = full_scene(nd)
    omega, scan = grid_of(t, k)
    return M.restate(t, v, omega, scan, ELIG['min_span'], ELIG['min_frac'], dtype=dtype)


def period_args(t, k):
    if k == 0:
        return dict(period_limit=max(t.max() - t.min(), DAY) / (3.0 + 4.3 / 8) / S.YEAR)
    return dict(period_range=band(t, k))


def grid_of(t, k):
    return S.frequency_grid(t, **period_args(t, k))


def rows_of(fits):
    f64 = lambda a: np.asarray(a, dtype=np.float64)
    return {c: f64(getattr(fits, c)) for c in COLUMNS + ('nobs', 'fitted', 'at_edge', 'kstar')}


def compare(got, f64, ld, tag, ambiguous=()):
    """the device's rows for the first n stations against the long-double yardstick; per column, 16 x the float64 yardstick's own gap over
    ALL stations of the scene is allowed (one station's gap is one draw of a round-off: the column's bound is the scene's)"""
    n = got['nobs'].size
    gaps = {}
    for c in COLUMNS:
        dist = M.angle_gap if c == 'phase' else (lambda a, b: np.abs(np.asarray(a - b, dtype=np.float64)))
        d = dist(np.asarray(f64[c], dtype=np.longdouble), np.asarray(ld[c], dtype=np.longdouble))
        gaps[c] = float(np.nanmax(d)) if not np.isnan(d).all() else 0.0
    f64 = {c: a[:n] for c, a in f64.items()}; ld = {c: a[:n] for c, a in ld.items()}
    fitted = ld['fitted'] != 0
    assert np.array_equal(got['nobs'], np.asarray(ld['nobs'], dtype=np.float64)), tag
    assert np.array_equal(got['fitted'] != 0, fitted) and np.array_equal(f64['fitted'] != 0, fitted), (tag, got['fitted'], ld['fitted'])
    clear = np.ones(fitted.size, bool); clear[list(ambiguous)] = False
    assert np.array_equal(got['at_edge'][clear] != 0, ld['at_edge'][clear] != 0), (tag, got['at_edge'], ld['at_edge'])
    if fitted.any() and not np.isnan(ld['kstar'][fitted]).all():
        assert (np.abs(got['kstar'] - np.asarray(ld['kstar'], dtype=np.float64))[fitted] <= np.where(clear, 0, 1)[fitted]).all(), (tag, got['kstar'], ld['kstar'])
    worst = 0.0
    for c in COLUMNS:
        want = np.asarray(ld[c], dtype=np.longdouble)
        assert np.array_equal(np.isnan(got[c]), np.isnan(np.asarray(want, dtype=np.float64))), (tag, c, got[c], want)
        ok = ~np.isnan(got[c])
        if not ok.any():
            continue
        dist = M.angle_gap if c == 'phase' else (lambda a, b: np.abs(np.asarray(a - b, dtype=np.float64)))
        gap = gaps[c]
        err = dist(got[c].astype(np.longdouble)[ok], want[ok]).max()
        print(f'{tag} {c}: float64 yardstick gap {gap:.3e}, device {err:.3e}' + (f' = {err / gap:.2f} gaps' if gap else ''))
        worst = max(worst, err / gap if gap else (0.0 if err == 0 else np.inf))
        assert err <= 16 * gap, (tag, c, err, gap)
    return worst


# ---- against the yardstick -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n,nd,k', [(1, 40, 0), (64, 77, 0), (65, 40, 0), (130, 77, 0), (7, 1, 0), (7, 2, 0),
                                    (1, 40, 9), (64, 77, 7), (65, 40, 9), (130, 77, 41), (64, 40, 1), (7, 1, 9), (7, 2, 9)])
def test_against_the_yardstick(n, nd, k):
    t, v = scene(n, nd)
    omega, scan = grid_of(t, k)
    assert omega.size == (1 if nd == 1 else max(k, 1)) and scan == (k > 0)              # (one date has no span: one frequency)
    fits = R.seasonal_fits(t, v, **period_args(t, k), **ELIG)
    assert fits.scan == scan and np.array_equal(fits.omega_grid, omega)
    f64, ld = model(nd, k, np.float64), model(nd, k, np.longdouble)
    got = rows_of(fits)
    compare(got, f64, ld, f'N={n} D={nd} K={k}', ambiguous=(6,) if n > 6 else ())
    fitted = got['fitted'] != 0
    if nd <= 2:
        assert not fitted.any()
    elif n > 6:
        assert fitted[[0, 1, 2, 4, 5, 6]].all() and not fitted[3] and np.isnan(got['amplitude'][3]) and got['nobs'][3] == 0
        assert (got['amplitude'][fitted] > 0).all() and (np.abs(got['phase'][fitted]) <= np.pi).all()
        if k >= 7:
            assert got['at_edge'][5] == 1 and got['kstar'][5] == 0 and got['at_edge'][4] == 0 and got['kstar'][4] == 4
            assert got['kstar'][6] in (3, 4) and abs(got['omega'][6] - 0.5 * (omega[3] + omega[4])) < 0.25 * (omega[1] - omega[0])
            assert abs(got['omega'][4] - (omega[4] + 0.3 * (omega[1] - omega[0]))) < 0.25 * (omega[1] - omega[0])
    if k == 1 and nd > 2:
        assert (got['at_edge'][fitted] == 1).all() and (got['omega'][fitted] == omega[0]).all()
    if k == 0 and nd > 2:
        assert np.isnan(got['sigma_omega']).all() and np.isnan(got['kstar']).all() and (got['at_edge'] == 0).all()
    # the derived columns
    ok = fitted
    assert np.array_equal(np.asarray(fits.period)[ok], 1 / ((got['omega'][ok] / (2.0 * np.pi)) * S.YEAR))
    assert np.array_equal(np.asarray(fits.frequency)[ok] * np.asarray(fits.period)[ok] > 0, np.ones(ok.sum(), bool))
    assert np.asarray(fits.nobs).dtype == np.int64 and np.asarray(fits.fitted).dtype == bool


def _network():
    """130 stations of scene(130, 77) on a 4 x 2 one-degree grid (cell = ix * ny + (ny - 1 - iy): the north row comes first): cell 0 holds
    one fitted station, cell 1 only the all-NaN column, the others several"""
    rng = np.random.default_rng(5)
    n = 130
    lon = -118.0 + rng.uniform(0.05, 0.95, n) + rng.integers(1, 4, n)
    lat = 33.0 + rng.uniform(0.05, 0.95, n) + rng.integers(0, 2, n)
    lon[3], lat[3] = -117.5, 33.5                            # (ix 0, iy 0) -> cell 1
    lon[4], lat[4] = -117.4, 34.6                            # (ix 0, iy 1) -> cell 0
    return lon, lat


@pytest.mark.parametrize('k', [0, 9])
def test_cell_means_and_maps(k):
    t, v = scene(130, 77)
    lon, lat = _network()
    res = R.grid_seasonal(lon, lat, t, v, **period_args(t, k), **ELIG)
    grid = res.grid
    assert list(grid.grid_dim) == [4, 2]
    order, start = grid.order, grid.start
    scan = k > 0
    out = {}
    for dtype in (np.float64, np.longdouble):
        m = model(77, k, dtype)
        cols = {c: a[order] for c, a in M.ref_columns(m, scan).items()}
        out[dtype] = M.cell_means(cols, m['nobs'][order], m['fitted'][order], start)
    f64, ld = out[np.float64], out[np.longdouble]
    got = np.asarray(res.cell_means)
    nfit = np.array([int((model(77, k, np.float64)['fitted'][order][start[g]:start[g + 1]] != 0).sum()) for g in range(8)])
    assert nfit[0] == 1 and nfit[1] == 0 and (nfit[2:] > 1).all(), nfit
    assert np.array_equal(np.isnan(got), np.isnan(np.asarray(ld, dtype=np.float64))) and np.isnan(got[:, 1]).all() and not np.isnan(got[:, 0]).any()
    for r in range(14):
        name = ('', 'absolute ')[r // 7] + M.REF_COLUMNS[r % 7]
        okc = ~np.isnan(got[r])
        gap = np.abs(np.asarray(f64[r].astype(np.longdouble) - ld[r], dtype=np.float64))[okc].max()
        err = np.abs(np.asarray(got[r].astype(np.longdouble) - ld[r], dtype=np.float64))[okc].max()
        print(f'K={k} cell mean of {name}: float64 yardstick gap {gap:.3e}, device {err:.3e}')
        assert err <= 16 * gap, (name, err, gap)
    # a cell with one fitted station: the plain mean is that station's column
    one = order[start[0]:start[1]]
    ref = res.fits.as_reference()
    assert one.tolist() == [4] and got[1, 0] == ref['ampfit'][4] and got[6, 0] == ref['seasonalfit_rmse'][4]
    # the maps are the cell means, row 0 in the north
    for i, name in enumerate(S.MAPS):
        assert np.array_equal(getattr(res, name), got[i].reshape(4, 2).T, equal_nan=True), name
    # the fits ride along in the caller's order and equal a plain call's bit for bit
    plain = R.seasonal_fits(t, v, **period_args(t, k), **ELIG)
    for c in BYTES:
        assert np.asarray(getattr(res.fits, c)).tobytes() == np.asarray(getattr(plain, c)).tobytes(), c


def test_no_fitted_station_raises_the_reference_exception():
    t, v = scene(7, 2)
    lon, lat = np.linspace(-117.9, -115.1, 7), np.linspace(33.1, 34.9, 7)
    with pytest.raises(Exception, match=r'No valid data values, adjust --min_span inputs for time span in years 0\.05 and/or fractional obs\. 0\.3'):
        R.grid_seasonal(lon, lat, t, v, period_limit=0.05, **ELIG)


# ---- the same bytes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [0, 9])
def test_same_bytes_host_device_twice_and_permuted(k):
    import torch
    t, v = scene(130, 77)
    kw = dict(period_args(t, k), **ELIG)
    a = R.seasonal_fits(t, v, **kw)
    b = R.seasonal_fits(t, v, **kw)
    d = R.seasonal_fits(t, torch.from_numpy(np.array(v)).cuda(), **kw)
    perm = np.random.default_rng(3).permutation(130)
    p = R.seasonal_fits(t, v[:, perm], **kw)
    assert torch.is_tensor(d.amplitude) and d.amplitude.is_cuda and d.nobs.dtype == torch.int64 and d.fitted.dtype == torch.bool
    for c in BYTES:
        x = np.asarray(getattr(a, c))
        assert x.tobytes() == np.asarray(getattr(b, c)).tobytes(), ('twice', c)
        assert x.tobytes() == getattr(d, c).cpu().numpy().tobytes(), ('device tensors', c)
        assert x[perm].tobytes() == np.asarray(getattr(p, c)).tobytes(), ('permuted', c)
    lon, lat = _network()
    g = R.grid_seasonal(lon, lat, t, v, **kw)
    gd = R.grid_seasonal(torch.from_numpy(lon).cuda(), torch.from_numpy(lat).cuda(), t, torch.from_numpy(np.array(v)).cuda(), **kw)
    assert np.asarray(g.cell_means).tobytes() == gd.cell_means.cpu().numpy().tobytes()
    assert torch.is_tensor(gd.grid_seasonal_phase) and np.array_equal(gd.grid_seasonal_absolute_fit_rmse.cpu().numpy(), g.grid_seasonal_absolute_fit_rmse, equal_nan=True)


def test_many_workgroups_cut_the_scan_into_segments_and_change_no_byte():
    import torch
    t, v = scene(130, 40)
    v = v[:, :128]
    kw = dict(period_args(t, 41), **ELIG)
    small = R.seasonal_fits(t, v, **kw)
    assert small.omega_grid.size == 41 and np.asarray(small.fitted).sum() > 100
    big = R.seasonal_fits(t, torch.from_numpy(np.array(v)).cuda().repeat(1, 1024), **kw)          # 131072 stations
    for c in BYTES:
        x = getattr(big, c).cpu().numpy().reshape(1024, 128)
        assert x[0].tobytes() == np.asarray(getattr(small, c)).tobytes(), c
        assert (x.view(np.uint8).reshape(1024, -1) == x[0].view(np.uint8).reshape(1, -1)).all(), c


# ---- golden g23: the reference's own run ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def g23():
    g = dict(np.load(GOLDEN))
    g['yard'] = {}
    for tag, kw in (('fixed', dict(period_limit=1.0)), ('free', dict(period_range=(0.5, 2.0)))):
        omega, scan = S.frequency_grid(g['t'], **kw)
        f64, ld = (M.restate(g['t'], g['values'], omega, scan, 2.0, 0.6, dtype=d) for d in (np.float64, np.longdouble))
        c64, cld = M.ref_columns(f64, scan), M.ref_columns(ld, scan)
        g['yard'][tag] = {c: float(np.nanmax(np.abs(np.asarray(c64[c].astype(np.longdouble) - cld[c], dtype=np.float64)))) for c in M.REF_COLUMNS}
    return g


def _tolerance(g, tag, c, over):
    """2 x the recorded |reference - restatement| of column c (its largest over the stations `over`) + 16 x the float64 yardstick's gap"""
    return 2 * float(g[f'gap_{tag}_{c}'][over].max()) + 16 * g['yard'][tag][c]


def test_golden_g23_fixed_period(g23):
    g = g23
    when = (g['t'] * 1e9).astype(np.int64).view('datetime64[ns]')                  # datetime64, as station_table returns it
    res = R.grid_seasonal(g['lon'], g['lat'], when, g['values'], spacing=1.0, period_limit=1.0)
    assert res.plotbbox == g['plotbbox'].tolist() and list(res.grid.grid_dim) == g['grid_dim'].tolist()
    fitted = ~np.isnan(g['fixed_ampfit'])
    assert np.array_equal(np.asarray(res.fits.fitted), fitted) and fitted.sum() == 6
    assert np.array_equal(np.asarray(res.fits.nobs), (~np.isnan(g['values'])).sum(axis=0))
    cols = res.fits.as_reference()
    tol = {}
    for c in M.REF_COLUMNS:
        want = g[f'fixed_{c}']
        assert np.array_equal(np.isnan(cols[c]), np.isnan(want)), c
        err = np.abs(cols[c] - want)[fitted].max(); tol[c] = _tolerance(g, 'fixed', c, fitted)
        print(f'g23 fixed {c}: device - reference {err:.3e}, allowed {tol[c]:.3e}')
        assert err <= tol[c], (c, err, tol[c])
    for name in S.MAPS:
        got, want = getattr(res, name), g[f'fixed_{name}']
        c = S.MAP_COLUMNS[name]
        assert got.shape == want.shape == (2, 3) and np.array_equal(np.isnan(got), np.isnan(want)), name
        ok = ~np.isnan(want)
        err = np.abs(got - want)[ok]; allowed = tol[c] + 8 * U * np.abs(want[ok])
        print(f'g23 fixed {name}: device - reference {err.max():.3e}, allowed {allowed.min():.3e}')
        assert (err <= allowed).all(), (name, err, allowed)
    assert (np.abs(res.grid_seasonal_absolute_amplitude - res.grid_seasonal_amplitude) > 1e-9).sum() == 2


def test_golden_g23_free_period(g23):
    g = g23
    fits = R.seasonal_fits(g['t'], g['values'], period_range=(0.5, 2.0))
    assert np.array_equal(fits.omega_grid, g['scan_omega'])
    fitted = ~np.isnan(g['free_ampfit'])
    reached = g['ref_reached_minimum']
    assert np.array_equal(np.asarray(fits.fitted), fitted) and reached.sum() >= 4 and not np.asarray(fits.at_edge).any()
    cols = fits.as_reference()
    for c in M.REF_COLUMNS:
        err = np.abs(cols[c] - g[f'free_{c}'])[reached].max(); tol = _tolerance(g, 'free', c, reached)
        print(f'g23 free {c}: device - reference {err:.3e} over the {int(reached.sum())} stations where the reference reached the minimum, allowed {tol:.3e}')
        assert err <= tol, (c, err, tol)
    ratio = np.asarray(fits.rss)[fitted] / g['free_ref_rss'][fitted]
    print('g23 free: device residual sum / reference residual sum', ratio)
    assert (np.asarray(fits.rss)[fitted] <= g['free_ref_rss'][fitted] * (1 + 1e-9)).all(), ratio


# ---- the C ABI: refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loc', [L.RDR_HOST, L.RDR_DEVICE], ids=['host', 'device'])
def test_refusals_leave_the_outputs_untouched(loc):
    import torch
    ctx = R.Context.default()
    n, nd, nc = 7, 40, 3
    t, v = scene(7, 40)
    i64 = lambda a: np.array(a, dtype=np.int64)
    dev = dict(v=np.array(v), cs=i64([0, 4, 4, 7]), cs_first=i64([1, 4, 4, 7]), cs_last=i64([0, 4, 4, 6]), cs_down=i64([0, 5, 4, 7]),
               st=np.full((16, n), -7.0), ce=np.full((14, nc), -7.0))
    w = grid_of(t, 9)[0]
    host = dict(t=np.array(t), w=w, w1=w[:1].copy(), w_nan=np.where(np.arange(9) == 2, np.nan, w), w_zero=np.where(np.arange(9) == 0, 0.0, w),
                w_down=w[::-1].copy(), t_inf=np.where(np.arange(nd) == 5, np.inf, t))
    if loc == L.RDR_DEVICE:
        bufs = {k: torch.from_numpy(a).cuda() for k, a in dev.items()}
        torch.cuda.synchronize()
        read = lambda k: bufs[k].cpu().numpy()
    else:
        bufs = {k: a.copy() for k, a in dev.items()}
        read = lambda k: bufs[k]
    bufs.update(host)

    def sf(t_='t', v_='v', n_=n, nd_=nd, w_='w', k_=9, scan_=1, span_=0.05, frac_=0.3, cs_='cs', nc_=nc, st_='st', ce_='ce', loc_=loc):
        p = lambda k: None if k is None else L.ptr(bufs[k])
        return ctx.lib.rdr_seasonal_fit(ctx.handle, p(t_), p(v_), n_, nd_, p(w_), k_, scan_, span_, frac_, p(cs_), nc_, p(st_), p(ce_), loc_)
    for kw, text in ((dict(t_=None), 'NULL argument'), (dict(v_=None), 'NULL argument'), (dict(w_=None), 'NULL argument'), (dict(st_=None), 'NULL argument'),
                     (dict(loc_=2), 'loc must be RDR_HOST or RDR_DEVICE'), (dict(loc_=-1), 'loc must be RDR_HOST or RDR_DEVICE'),
                     (dict(n_=0), 'n must be 1 .. 2^20 stations (got 0)'), (dict(n_=(1 << 20) + 1), 'n must be 1 .. 2^20 stations'),
                     (dict(nd_=0), 'nd must be 1 .. 4096 dates (got 0)'), (dict(nd_=4097), 'nd must be 1 .. 4096 dates (got 4097)'),
                     (dict(k_=0), 'k must be 1 .. 4096 frequencies (got 0)'), (dict(k_=4097), 'k must be 1 .. 4096 frequencies (got 4097)'),
                     (dict(scan_=2), 'scan must be 0 or 1'), (dict(scan_=0), 'takes one frequency (got k = 9)'),
                     (dict(span_=-0.5), 'min_span must be finite and >= 0'), (dict(span_=float('nan')), 'min_span must be finite and >= 0'),
                     (dict(frac_=float('inf')), 'min_frac must be finite'),
                     (dict(w_='w_nan'), 'omega[2] must be finite and > 0'), (dict(w_='w_zero'), 'omega[0] must be finite and > 0'),
                     (dict(w_='w_down'), 'omega must ascend (index 1)'), (dict(t_='t_inf'), 't[5] is not finite'),
                     (dict(cs_=None), 'cell_start and cells come together'), (dict(ce_=None), 'cell_start and cells come together'),
                     (dict(nc_=0), 'ncells must be 1 .. 2^20 cells (got 0)'),
                     (dict(cs_='cs_first'), 'cell_start[0] must be 0 (got 1)'), (dict(cs_='cs_last'), 'cell_start[ncells] must be n = 7 (got 6)'),
                     (dict(cs_='cs_down'), 'cell_start is not ascending at index 2')):
        assert sf(**kw) == L.RDR_ERR_INVALID, kw
        assert text in L.last_error(ctx.handle), (text, L.last_error(ctx.handle))
    ctx.synchronize()
    for k in ('st', 'ce'):                                  # the sentinels are still there
        assert np.array_equal(read(k), dev[k]), k
    assert sf() == L.RDR_OK                                 # and the same buffers make a valid call
    assert sf(w_='w1', k_=1, scan_=0, cs_=None, ce_=None) == L.RDR_OK          # fixed mode, no cells
    ctx.synchronize()
    assert not (read('st') == -7.0).any() and not (read('ce') == -7.0).any()
