"""GPU: a date series at query points in one pass (rdr_interp3_project_epochs, rdr_point_delays_epochs) - bit for bit what one
rdr_interp3_project / rdr_point_delays call per date gives.  Every comparison is on the bytes (NaNs included): no tolerances."""
import ctypes as C
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NY, NX, NZ = 5, 6, 4
ZS = np.array([0.0, 300.0, 1200.0, 4000.0])                            # non-uniform
DMAX = 7
MODES = ('none', 'inc0', 'inc', 'div', 'div_per_date')


def _same(a, b):
    a = a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)
    b = b.cpu().numpy() if hasattr(b, 'cpu') else np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _fields(seed):
    from raider_amd.synthetic import synthetic_cube
    return synthetic_cube(NY, NX, NZ, seed=seed, zs=ZS)


@functools.lru_cache(maxsize=None)
def _cubes(dtype):
    """DMAX cubes of 5 x 6 x 4 nodes on one grid - descending y axis, non-uniform z axis - with a different seed per date"""
    import raider_amd as R
    out = []
    for e in range(DMAX):
        c = _fields(100 + e)
        out.append(R.Cube(c['ys'][::-1].copy(), c['xs'], c['zs'], c['wet'].astype(dtype), c['hydro'].astype(dtype), order='zyx'))
    return out


@functools.lru_cache(maxsize=None)
def _points():
    """n = 1000 = 15 full waves and a partial one: every node exactly (the last node of each axis = the closed upper cell among them), a
    point in every cell, 5 % outside each axis, three NaN coordinates, random interior points for the rest"""
    c = _fields(0)
    ys, xs, zs = c['ys'], c['xs'], c['zs']
    rng = np.random.default_rng(7)
    P = [np.stack([g.ravel() for g in np.meshgrid(ys, xs, zs, indexing='ij')], axis=-1)]                      # 120 nodes
    iy, ix, iz = (g.ravel() for g in np.meshgrid(np.arange(NY - 1), np.arange(NX - 1), np.arange(NZ - 1), indexing='ij'))
    t = rng.uniform(0.05, 0.95, (iy.size, 3))
    P.append(np.stack([ys[iy] + t[:, 0] * (ys[iy + 1] - ys[iy]), xs[ix] + t[:, 1] * (xs[ix + 1] - xs[ix]), zs[iz] + t[:, 2] * (zs[iz + 1] - zs[iz])], axis=-1))   # 60 cells
    lo, hi = np.array([ys[0], xs[0], zs[0]]), np.array([ys[-1], xs[-1], zs[-1]])
    for ax in range(3):                                                # 50 outside each axis, both sides
        q = rng.uniform(lo, hi, (50, 3))
        q[:25, ax] = lo[ax] - rng.uniform(1e-9, 1.0, 25) * (hi[ax] - lo[ax])
        q[25:, ax] = hi[ax] + rng.uniform(1e-9, 1.0, 25) * (hi[ax] - lo[ax])
        P.append(q)
    q = rng.uniform(lo, hi, (3, 3))
    q[0, 0] = q[1, 1] = q[2, 2] = np.nan
    P.append(q)
    P.append(rng.uniform(lo, hi, (1000 - sum(p.shape[0] for p in P), 3)))
    pts = np.concatenate(P)
    pts = pts[rng.permutation(pts.shape[0])]
    assert pts.shape == (1000, 3)
    inc = rng.uniform(20.0, 46.0, 1000)
    div = rng.uniform(0.6, 0.95, (DMAX, 1000))
    return pts, inc, div


def _kw(mode, inc, div, e=None, D=None):
    """the projection arguments of one mode: for date e of the per-date reference, or (e None) for the series call on D dates"""
    if mode == 'none':
        return {}
    if mode == 'inc0':
        return dict(inc=33.5)
    if mode == 'inc':
        return dict(inc=inc)
    if mode == 'div':
        return dict(divisor=div[0])
    return dict(divisor=div[e] if e is not None else div[:D])


@functools.lru_cache(maxsize=None)
def _reference(dtype):
    """{mode: (wet[DMAX, n], hydro[DMAX, n])} from one Cube.interp_project per date: made once, shared by every case"""
    pts, inc, div = _points()
    y, x, z = (np.ascontiguousarray(pts[:, k]) for k in range(3))
    ref = {}
    for mode in MODES:
        res = [cb.interp_project(y, x, z, **_kw(mode, inc, div, e=e)) for e, cb in enumerate(_cubes(dtype))]
        w, h = np.stack([np.array(r[0]) for r in res]), np.stack([np.array(r[1]) for r in res])
        w.setflags(write=False); h.setflags(write=False)
        ref[mode] = (w, h)
    w = ref['none'][0]
    inside_all = np.isfinite(pts).all(axis=1)
    assert 140 <= np.isnan(w[0]).sum() <= 160 and np.isfinite(w[0][inside_all]).sum() > 800 and not _same(w[0], w[1])
    return ref


@pytest.mark.parametrize('D', [1, 2, 3, 4, 7])               # launch groups 1, 2, 2 + 1, 4, 4 + 2 + 1
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_gather_equals_the_per_date_call_bit_for_bit(dtype, D):
    import torch
    import raider_amd as R
    pts, inc, div = _points()
    cubes = _cubes(dtype)[:D]
    ref = _reference(dtype)
    y, x, z = (np.ascontiguousarray(pts[:, k]) for k in range(3))
    dev = torch.device('cuda:0')
    ty, tx, tz, tp = (torch.from_numpy(a).to(dev) for a in (y, x, z, pts))
    for mode in MODES:
        rw, rh = ref[mode][0][:D], ref[mode][1][:D]
        kw = _kw(mode, inc, div, D=D)
        w, h = R.interp_project_epochs(cubes, y, x, z, **kw)                                   # host, three arrays
        assert w.shape == (D, 1000) and _same(w, rw) and _same(h, rh), (mode, 'host xyz')
        w, h = R.interp_project_epochs(cubes, pts, **kw)                                       # host, packed (n, 3)
        assert _same(w, rw) and _same(h, rh), (mode, 'host packed')
        w, h = R.interp_project_epochs(cubes, ty, tx, tz, **kw)                                # device tensors, host projection arrays
        assert w.is_cuda and _same(w, rw) and _same(h, rh), (mode, 'device xyz')
        kd = {k: (torch.from_numpy(np.ascontiguousarray(v)).to(dev) if np.ndim(v) else v) for k, v in kw.items()}
        w, h = R.interp_project_epochs(cubes, tp, **kd)                                        # device tensors throughout, packed
        assert _same(w, rw) and _same(h, rh), (mode, 'device packed')
    # a 2-D point set keeps its shape behind the date axis
    w, h = R.interp_project_epochs(cubes, y.reshape(40, 25), x.reshape(40, 25), z.reshape(40, 25), divisor=div[:D].reshape(D, 40, 25))
    assert w.shape == (D, 40, 25) and _same(w.reshape(D, -1), ref['div_per_date'][0][:D]) and _same(h.reshape(D, -1), ref['div_per_date'][1][:D])


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_one_point_and_no_point(dtype):
    import raider_amd as R
    pts, inc, div = _points()
    cubes = _cubes(dtype)[:3]
    ref = _reference(dtype)
    k = int(np.flatnonzero(np.isfinite(ref['inc'][0][0]))[0])
    w, h = R.interp_project_epochs(cubes, pts[k:k + 1, 0], pts[k:k + 1, 1], pts[k:k + 1, 2], inc=inc[k:k + 1])
    assert w.shape == (3, 1) and _same(w[:, 0], ref['inc'][0][:3, k]) and _same(h[:, 0], ref['inc'][1][:3, k])
    w, h = R.interp_project_epochs(cubes, pts[k:k + 1], divisor=div[:3, k:k + 1])
    assert _same(w[:, 0], ref['div_per_date'][0][:3, k]) and _same(h[:, 0], ref['div_per_date'][1][:3, k])
    w, h = R.interp_project_epochs(cubes, np.empty((0, 3)))
    assert w.shape == (3, 0) and h.shape == (3, 0)
    w, h = R.interp_project_epochs(cubes, np.empty(0), np.empty(0), np.empty(0), inc=np.empty(0))
    assert w.shape == (3, 0) and h.shape == (3, 0)


def test_epochs_do_not_mix():
    import raider_amd as R
    pts, inc, div = _points()
    cubes = _cubes(np.float32)
    ref = _reference(np.float32)['inc']
    perm = [4, 0, 6, 2, 1, 5, 3]
    w, h = R.interp_project_epochs([cubes[i] for i in perm], pts, inc=inc)
    assert _same(w, ref[0][perm]) and _same(h, ref[1][perm])
    # one date's cube carries an interior NaN block: only that date's points in the cells around it turn NaN
    c = _fields(100 + 2)
    wet, hyd = c['wet'].copy(), c['hydro'].copy()
    wet[1:3, 2:3, 2:4] = np.nan; hyd[1:3, 2:3, 2:4] = np.nan                                    # (z, y, x)
    holed = R.Cube(c['ys'][::-1].copy(), c['xs'], c['zs'], wet, hyd, order='zyx')
    series = cubes[:2] + [holed] + cubes[3:5]
    w, h = R.interp_project_epochs(series, pts, inc=inc)
    for e in (0, 1, 3, 4):
        assert _same(w[e], ref[0][e]) and _same(h[e], ref[1][e]), e
    w1, h1 = holed.interp_project(pts, inc=inc)
    assert _same(w[2], np.array(w1)) and _same(h[2], np.array(h1))
    hit = np.isnan(w[2]) & ~np.isnan(ref[0][2])
    assert 20 < hit.sum() < 500 and _same(w[2][~hit], ref[0][2][~hit]) and np.array_equal(np.isnan(h[2]), np.isnan(w[2]))


def test_pipelined_upload_sends_the_points_once():
    """2^20 + 37 host points take the chunked three-stream pipeline: the same bits as one call per date, and the points (and a shared
    incidence array) cross the link once - 24 (+ 8) B per point - whatever the number of dates"""
    import raider_amd as R
    cubes = _cubes(np.float64)[:3]
    ctx = cubes[0].ctx
    c = _fields(0)
    n = (1 << 20) + 37
    rng = np.random.default_rng(11)
    lo, hi = np.array([c['ys'][0], c['xs'][0], c['zs'][0]]), np.array([c['ys'][-1], c['xs'][-1], c['zs'][-1]])
    span = hi - lo
    y, x, z = (np.ascontiguousarray(rng.uniform(lo[k] - 0.02 * span[k], hi[k] + 0.02 * span[k], n)) for k in range(3))
    inc = rng.uniform(20.0, 46.0, n)
    w, h = R.interp_project_epochs(cubes, y, x, z, inc=inc)
    assert ctx.point_upload_bytes() == 32 * n
    for e, cb in enumerate(cubes):
        w1, h1 = cb.interp_project(y, x, z, inc=inc)
        assert _same(w[e], np.asarray(w1)) and _same(h[e], np.asarray(h1)), e
    assert 0.8 < np.isfinite(w[0]).mean() < 0.95
    # per-date divisors are the one thing that goes up per date
    div = rng.uniform(0.6, 0.95, (3, n))
    w, h = R.interp_project_epochs(cubes, y, x, z, divisor=div)
    assert ctx.point_upload_bytes() == (24 + 3 * 8) * n
    w1, h1 = cubes[2].interp_project(y, x, z, divisor=div[2])
    assert _same(w[2], np.asarray(w1)) and _same(h[2], np.asarray(h1))
    # below the pipeline's threshold the staging is a single copy as well
    R.interp_project_epochs(cubes, y[:1000], x[:1000], z[:1000])
    assert ctx.point_upload_bytes() == 24 * 1000


def _model_cubes(holed=1, **kw):
    """three float32 total-delay cubes of 12 x 14 x 10 nodes; date `holed` has a NaN block over the middle of the grid"""
    import raider_amd as R
    from raider_amd.synthetic import synthetic_cube
    out = []
    for e in range(3):
        c = synthetic_cube(12, 14, 10, seed=40 + e, **kw)
        wet, hyd = c['wet_total'].astype(np.float32), c['hydro_total'].astype(np.float32)
        if e == holed:
            wet[:, 5:8, 6:9] = np.nan; hyd[:, 5:8, 6:9] = np.nan
        out.append(R.Cube(c['ys'], c['xs'], c['zs'], wet, hyd, order='zyx'))
    return out


def _check_point_delays(cubes, xpts, ypts, zpts, pts, grid=None):
    import raider_amd as R
    rng = np.random.default_rng(5)
    inc = rng.uniform(25.0, 45.0, pts.shape[0])
    div = rng.uniform(0.6, 0.95, (3, pts.shape[0]))
    for kw_series, kw_date in (({}, lambda e: {}), (dict(inc=inc), lambda e: dict(inc=inc)), (dict(divisor=div), lambda e: dict(divisor=div[e]))):
        w, h, nan = R.point_delays_epochs(cubes, xpts, ypts, zpts, pts, grid=grid, **kw_series)
        assert w.shape == (3, pts.shape[0]) and nan.shape == (3,) and nan.dtype == bool
        for e, cb in enumerate(cubes):
            w1, h1, nan1 = cb.point_delays(xpts, ypts, zpts, pts, grid=grid, **kw_date(e))
            assert _same(w[e], np.asarray(w1)) and _same(h[e], np.asarray(h1)) and bool(nan[e]) == nan1, e
        assert list(nan) == [False, True, False]
        assert np.isfinite(w[0]).mean() > 0.7 and np.isnan(w[1]).sum() > np.isnan(w[0]).sum()
    # three arrays instead of the packed one
    w3, h3, _ = R.point_delays_epochs(cubes, xpts, ypts, zpts, *(np.ascontiguousarray(pts[:, k]) for k in range(3)), grid=grid, divisor=div)
    assert _same(w3, w) and _same(h3, h)
    return w


def test_point_delays_epochs_lonlat_lcc_and_utm():
    from raider_amd.delay import grid_projection, transformPoints
    rng = np.random.default_rng(9)
    xpts = np.linspace(-118.6, -115.4, 6); ypts = np.linspace(34.4, 31.6, 5); zpts = np.array([0.0, 400.0, 1500.0, 3500.0])
    la = rng.uniform(31.5, 34.5, 500); lo = rng.uniform(-118.7, -115.3, 500); hg = rng.uniform(-50.0, 3600.0, 500)
    pts = np.stack([la, lo, hg], axis=-1)
    cubes = _model_cubes()
    _check_point_delays(cubes, xpts, ypts, zpts, pts)
    # the same model as an LCC grid (HRRR's cone), seen through views that carry the projection
    H = dict(proj='lcc', lat_1=38.5, lat_2=38.5, lat_0=38.5, lon_0=262.5, a=6371229.0, es=0.0)
    lcc = [cb.view(projection=H) for cb in _model_cubes(y0=-9.0e5, y1=1.0e5, x0=-2.2e6, x1=-1.3e6)]
    xl = np.linspace(-117.5, -114.0, 6); yl = np.linspace(36.0, 33.5, 5)
    pl = np.stack([rng.uniform(33.4, 36.1, 500), rng.uniform(-117.6, -113.9, 500), hg], axis=-1)
    _check_point_delays(lcc, xl, yl, zpts, pl)
    # a UTM output grid (zone 11 N) over the lon/lat model: rdr_point_delays_grid per date
    grid = grid_projection(32611)
    xu = np.linspace(330000.0, 670000.0, 6); yu = np.linspace(3790000.0, 3510000.0, 5)
    pu = np.ascontiguousarray(transformPoints(la, lo, hg, 4326, 32611))            # stacked (northing, easting, height)
    assert pu.shape == (500, 3)
    _check_point_delays(cubes, xu, yu, zpts, pu, grid=grid)
    # one date is rdr_point_delays itself
    import raider_amd as R
    w, h, nan = R.point_delays_epochs(cubes[1:2], xpts, ypts, zpts, pts, inc=31.0)
    w1, h1, nan1 = cubes[1].point_delays(xpts, ypts, zpts, pts, inc=31.0)
    assert _same(w[0], np.asarray(w1)) and _same(h[0], np.asarray(h1)) and list(nan) == [True] and nan1


def test_refusals_by_name():
    import raider_amd as R
    from raider_amd import _lib as L
    pts, inc, div = _points()
    cubes = _cubes(np.float32)
    c = _fields(102)
    ys = c['ys'][::-1].copy()
    bad = {
        'z axis': R.Cube(ys, c['xs'], c['zs'] + 1.0, c['wet'], c['hydro'], order='zyx'),
        'dtype': R.Cube(ys, c['xs'], c['zs'], c['wet'].astype(np.float64), c['hydro'].astype(np.float64), order='zyx'),
        'projection': R.Cube(ys, c['xs'], c['zs'], c['wet'], c['hydro'], order='zyx').set_projection_lcc(38.5, 38.5, 38.5, 262.5),
    }
    xpts = np.linspace(-120.0, -114.0, 6); ypts = np.linspace(35.0, 31.0, 5); zpts = np.array([0.0, 400.0, 1500.0, 3500.0])
    for what, cb in bad.items():
        with pytest.raises(ValueError, match='rdr_interp3_project_epochs: epoch 2'):
            R.interp_project_epochs([cubes[0], cubes[1], cb], pts)
        with pytest.raises(ValueError, match='rdr_point_delays_epochs: epoch 2'):
            R.point_delays_epochs([cubes[0], cubes[1], cb], xpts, ypts, zpts, pts)
    with pytest.raises(ValueError, match='leading axis of 2'):
        R.interp_project_epochs(cubes[:3], pts, divisor=div[:2])
    with pytest.raises(ValueError, match='leading axis of 4'):
        R.point_delays_epochs(cubes[:3], xpts, ypts, zpts, pts, inc=np.broadcast_to(inc, (4, 1000)))
    with pytest.raises(ValueError, match='at least one epoch'):
        R.interp_project_epochs([], pts)
    # the C entries refuse a divisor stride that is neither 0 nor n
    ctx = cubes[0].ctx
    handles = (C.c_void_p * 3)(*[cb.handle for cb in cubes[:3]])
    p = np.ascontiguousarray(pts); d = np.ascontiguousarray(div[:3])
    w = np.empty((3, 1000)); h = np.empty((3, 1000)); flags = np.zeros(3, dtype=np.int32)
    with pytest.raises(ValueError, match='proj_stride'):
        L.check(ctx.lib.rdr_interp3_project_epochs(ctx.handle, handles, 3, L.ptr(p), None, None, 1000, 3, L.ptr(d), 7, 0.0, L.ptr(w), L.ptr(h), L.RDR_HOST), ctx.handle)
    gx, gy = np.ascontiguousarray(xpts), np.ascontiguousarray(ypts)
    with pytest.raises(ValueError, match='proj_stride'):
        L.check(ctx.lib.rdr_point_delays_epochs(ctx.handle, handles, 3, 0, None, 0, L.ptr(gx), 6, L.ptr(gy), 5, L.ptr(zpts), 4, L.ptr(p), None, None, 1000, 3,
                                                L.ptr(d), 999, 0.0, L.ptr(w), L.ptr(h), flags.ctypes.data_as(L.c_ip)), ctx.handle)
    # the refusals left nothing behind: the same context still answers
    w2, _ = R.interp_project_epochs(cubes[:3], pts)
    assert _same(w2, _reference(np.float32)['none'][0][:3])
