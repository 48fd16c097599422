"""GPU: gridded station statistics (rdr_grid_stats, csrc/grid_stats_kernels.h; raider_amd/station_stats.py: grid_statistics).

The yardstick is NumPy with math.fsum and np.longdouble, in this file, on the valid values m of a station or of a cell:
  median   (s[(m - 1) // 2] + s[m // 2]) / 2 of the sorted values - compared with == and the NaN mask (the sign of a zero is not pinned);
  mean     fsum(v) / m; the device within (m + 2) * 2^-53 * sum|v| / m;
  stdev    sqrt(sum (v - mean)^2 / (m - 1)) in long double; the device within ((m + 8) sigma + 2 m |mean|) * 2^-53 - the relative
           ((m + 8) + 2 m |mean| / sigma) * 2^-53 of two-pass rounding plus the first-order effect of the mean's own error, written as
           an absolute bound so that it also speaks for sigma = 0;
  the means over a cell's k stations of a station statistic: the yardstick's own station values, fsum / k; the device within the mean of
           the stations' bounds plus (k + 2) * 2^-53 * sum|statistic| / k.
Golden g22 (tools/gen_golden_grid_stats.py: the reference's RaiderStats.create_DF whole): heatmap and NaN masks exact, the absolute
median bit for bit, the other maps within TWICE those bounds (pandas sums in another order).

Shapes: nd = 1, 2, 3, 64, 65, 257 (the four waves of the station kernel split the dates: 0, 1 or many per wave, the unrolled loop's
tail) and 4096 with n = 3; n = 1, 63, 64, 65, 130 (one workgroup, its last lane, two, three); cells that are empty, hold one station,
hold stations without a row, hold one single-row station; cells of 255, 256 and 257 stations (the slab walk of the cell kernel steps
by 256 / m dates and 256 % m stations: m below, at and above the workgroup's width).
"""
import functools
import math
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import raider_amd as R                                     # noqa: E402
from raider_amd import _lib as L                           # noqa: E402
from raider_amd import variogram as V                      # noqa: E402

GOLDEN = Path(__file__).resolve().parent / 'golden' / 'g22_grid_stats.npz'
U = 2.0 ** -53
ST = ('st_nobs', 'st_mean', 'st_median', 'st_stdev')
OF = ('nstations', 'mean_of_means', 'mean_of_medians', 'mean_of_stdevs')
AB = ('cell_nobs', 'abs_mean', 'abs_median', 'abs_stdev')
MAPS = {'grid_delay_mean': 'mean_of_means', 'grid_delay_median': 'mean_of_medians', 'grid_delay_stdev': 'mean_of_stdevs',
        'grid_delay_absolute_mean': 'abs_mean', 'grid_delay_absolute_median': 'abs_median', 'grid_delay_absolute_stdev': 'abs_stdev'}


# ---- the yardstick -------------------------------------------------------------------------------------------------------------------
def plain(v):
    """no infinity, and nothing whose sum or square leaves the range the bounds speak for (overflow, underflow to a subnormal)"""
    a = np.abs(v[~np.isnan(v)])
    return bool(np.isfinite(a).all() and (a < 1e150).all() and (a[a > 0] > 1e-150).all())


def segment(v):
    """(count, mean, median, stdev, mean bound, stdev bound) of the values of v that are not NaN"""
    v = np.asarray(v, dtype=np.float64).ravel()
    v = v[~np.isnan(v)]
    m = v.size
    if m == 0:
        return 0, np.nan, np.nan, np.nan, 0.0, 0.0
    with np.errstate(all='ignore'):
        s = np.sort(v)
        med = (s[(m - 1) // 2] + s[m // 2]) / 2
        if not plain(v):
            return m, np.nan, med, np.nan, np.nan, np.nan                # (only the count and the median are pinned there)
        mean = math.fsum(v) / m
        tmean = (m + 2) * U * math.fsum(np.abs(v)) / m
        if m < 2:
            return m, mean, med, np.nan, tmean, 0.0
        ld = v.astype(np.longdouble)
        mu = ld.sum() / m
        sd = float(np.sqrt(((ld - mu) ** 2).sum() / (m - 1)))
        return m, mean, med, sd, tmean, ((m + 8) * sd + 2 * m * abs(mean)) * U


def yardstick(vs, start):
    """every output of rdr_grid_stats for sorted values vs [D, n] and cell_start, with its bound: {name: (value, bound)}"""
    n, g = vs.shape[1], start.size - 1
    st = np.array([segment(vs[:, i]) for i in range(n)], dtype=np.float64).reshape(n, 6)
    ab = np.array([segment(vs[:, start[c]:start[c + 1]]) for c in range(g)], dtype=np.float64).reshape(g, 6)
    of = np.full((g, 4), np.nan); oft = np.zeros((g, 4))
    for c in range(g):
        sl = slice(start[c], start[c + 1])
        of[c, 0] = (st[sl, 0] > 0).sum()
        for k, (col, tol) in enumerate(((1, 4), (2, None), (3, 5)), start=1):
            a = st[sl, col]
            ok = ~np.isnan(a)
            if ok.any() and plain(a):                     # (station statistics that are not plain: their mean is not pinned)
                kk = int(ok.sum())
                of[c, k] = math.fsum(a[ok]) / kk
                oft[c, k] = (math.fsum(st[sl, tol][ok]) / kk if tol is not None else 0.0) + (kk + 2) * U * math.fsum(np.abs(a[ok])) / kk
    z = np.zeros
    return {'st_nobs': (st[:, 0], z(n)), 'st_mean': (st[:, 1], st[:, 4]), 'st_median': (st[:, 2], z(n)), 'st_stdev': (st[:, 3], st[:, 5]),
            'nstations': (of[:, 0], z(g)), 'mean_of_means': (of[:, 1], oft[:, 1]), 'mean_of_medians': (of[:, 2], oft[:, 2]),
            'mean_of_stdevs': (of[:, 3], oft[:, 3]), 'cell_nobs': (ab[:, 0], z(g)), 'abs_mean': (ab[:, 1], ab[:, 4]), 'abs_median': (ab[:, 2], z(g)),
            'abs_stdev': (ab[:, 3], ab[:, 5])}


def compare(out, yard, names=ST + OF + AB, factor=1.0, tag=''):
    for k in names:
        got = np.asarray(out[k], dtype=np.float64); want, tol = yard[k]
        assert np.array_equal(np.isnan(got), np.isnan(want)), (tag, k, 'NaN mask', got, want)
        ok = ~np.isnan(want)
        if k in ('st_nobs', 'nstations', 'cell_nobs', 'st_median', 'abs_median'):
            assert np.array_equal(got[ok], want[ok]), (tag, k, got, want)
            continue
        err = np.abs(got[ok] - want[ok])
        worst = (err / np.where(tol[ok] > 0, tol[ok], 1.0)).max() if ok.any() else 0.0
        print(f'{tag} {k}: max |d| {err.max() if ok.any() else 0.0:.3e}, largest share of its bound {worst:.3f}')
        assert (err <= factor * tol[ok]).all(), (tag, k, err, tol[ok])


# ---- calls ---------------------------------------------------------------------------------------------------------------------------
def call(vs, start, medians=True, groups=('st', 'of', 'ab')):
    """rdr_grid_stats on host arrays -> {name: array}; -7 sentinels where a group or the medians are not asked for"""
    ctx = R.Context.default()
    vs = np.ascontiguousarray(vs, dtype=np.float64); start = np.ascontiguousarray(start, dtype=np.int64)
    nd, n = vs.shape; g = start.size - 1
    o = {k: np.full(n if k in ST else g, -7, dtype=np.int64 if k in ('st_nobs', 'nstations', 'cell_nobs') else np.float64) for k in ST + OF + AB}
    on = {'st': ST, 'of': OF, 'ab': AB}
    p = lambda k: L.ptr(o[k]) if any(k in on[q] for q in groups) and (medians or 'median' not in k) else None
    L.check(ctx.lib.rdr_grid_stats(ctx.handle, L.ptr(vs), n, nd, L.ptr(start), g, *[p(k) for k in ST + OF + AB], L.RDR_HOST), ctx.handle)
    return o


def series(nd, n, seed, holes=0.3):
    rng = np.random.default_rng(seed)
    v = 2.4 + 0.3 * rng.standard_normal((nd, n)) * rng.uniform(0.01, 1.0, n)[None, :] - 5.0 * (rng.uniform(size=n) < 0.2)[None, :]
    v[rng.uniform(size=(nd, n)) < holes] = np.nan
    return v


def cells_for(nd, n, seed):
    """values [nd, n] and cell_start: an empty cell, a cell of one single-row station, a cell of two stations without a row, a cell of
    one station, and the rest in two cells (n < 8: an empty cell and one cell)"""
    v = series(nd, n, seed)
    if n < 8:
        return v, np.array([0, 0, n], dtype=np.int64)
    v[:, 0] = np.nan; v[nd // 2, 0] = 2.375
    v[:, 1:3] = np.nan
    return v, np.array([0, 0, 1, 3, 4, 4 + (n - 4) // 2, n, n], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def scene(nd, n, seed):
    v, start = cells_for(nd, n, seed)
    v.setflags(write=False)
    return v, start, yardstick(v, start)


# ---- shapes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nd,n', [(1, 130), (2, 130), (3, 130), (64, 130), (65, 130), (257, 130), (4096, 3), (9, 1), (9, 63), (9, 64), (9, 65)])
def test_shapes_against_the_yardstick(nd, n):
    v, start, yard = scene(nd, n, 100 + nd + n)
    compare(call(v, start), yard, tag=f'nd={nd} n={n}')


def test_cells_below_at_and_above_the_workgroup_width():
    nd = 3
    v = series(nd, 255 + 256 + 257, 7)
    start = np.array([0, 255, 511, 768], dtype=np.int64)
    compare(call(v, start), yardstick(v, start), tag='cells 255 256 257')


# ---- keys ----------------------------------------------------------------------------------------------------------------------------
def _bits(b):
    return np.array([b], dtype=np.uint64).view(np.float64)[0]


def key_series():
    inf = np.inf
    cols = [[2.5] * 7, [2.5] * 8, [-0.75] * 6, [1.0, 2.0, 3.0, 3.0, 4.0, 5.0], [5.0, 3.0, 1.0, 3.0, 3.0, 2.0, 3.0, 4.0],
            [-inf, -1e-310, -0.0, 0.0, 5e-324, 1.0, inf, -2.0, 3.0], [-inf, inf], [inf, inf, -inf, 1.0], [-0.0, 0.0], [0.0, -0.0, -5e-324, 5e-324],
            [-1e-310, 1e-310, -2e-310, 3e-310, -5e-324], [inf], [-inf, -inf, -inf, 7.0, inf, inf], [1.7e308, 1.7e308], [-3.0, -1.0, -2.0, -4.0]]
    a = 0x3ff0000000000000                                  # 1.0
    for p in range(8):                                      # the two middle keys part ways in byte p, counted from the lowest
        b = a + (1 << (8 * p))
        col = [-1.0, _bits(a - 2), _bits(a - 1), _bits(a), _bits(b), _bits(b + 1), _bits(b + 2), 5e30]
        ka, kb = a | (1 << 63), b | (1 << 63)
        assert ka >> (8 * p + 8) == kb >> (8 * p + 8) and (ka >> (8 * p)) & 255 != (kb >> (8 * p)) & 255
        cols.append(col[::-1])
        cols.append([-x for x in col[::2] + col[1::2]])     # the same among the negative keys
    nd = max(len(c) for c in cols)
    v = np.full((nd, len(cols)), np.nan)
    rng = np.random.default_rng(5)
    for i, c in enumerate(cols):
        v[rng.permutation(nd)[:len(c)], i] = c
    return v


@pytest.mark.parametrize('ncells', [1, 5])
def test_keys(ncells):
    v = key_series()
    n = v.shape[1]
    start = np.array([0, n], dtype=np.int64) if ncells == 1 else np.array([0, 5, 11, 15, 23, n], dtype=np.int64)
    out = call(v, start)
    yard = yardstick(v, start)
    for k in ('st_nobs', 'st_median', 'nstations', 'cell_nobs', 'abs_median'):
        got = np.asarray(out[k], dtype=np.float64); want = yard[k][0]
        assert np.array_equal(got, want, equal_nan=True), (k, got, want)
    keep = np.array([plain(v[:, i]) for i in range(n)])                            # there everything holds
    assert 8 <= keep.sum() < n
    sub = np.ascontiguousarray(v[:, keep]); s2 = np.array([0, sub.shape[1]], dtype=np.int64)
    compare(call(sub, s2), yardstick(sub, s2), tag='keys, plain series')


# ---- other checks --------------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes_and_medians_off_changes_nothing_else():
    v, start, yard = scene(65, 130, 100 + 65 + 130)
    a, b = call(v, start), call(v, start)
    for k in ST + OF + AB:
        assert a[k].tobytes() == b[k].tobytes(), k
    c = call(v, start, medians=False)
    for k in ST + OF + AB:
        if 'median' in k:
            assert (c[k] == -7).all(), k                    # not written
        else:
            assert a[k].tobytes() == c[k].tobytes(), k


@pytest.mark.parametrize('groups', [('st',), ('of',), ('ab',), ('of', 'ab'), ('st', 'ab')])
def test_groups_alone_give_the_same_bytes(groups):
    v, start, yard = scene(65, 130, 100 + 65 + 130)
    full = call(v, start)
    for medians in (True, False):
        part = call(v, start, medians=medians, groups=groups)
        on = sum(({'st': ST, 'of': OF, 'ab': AB}[q] for q in groups), ())
        for k in ST + OF + AB:
            if k in on and (medians or 'median' not in k):
                assert part[k].tobytes() == full[k].tobytes(), (groups, medians, k)
            else:
                assert (part[k] == -7).all(), (groups, medians, k)


def _network(seed=3, n=150, nd=12):
    rng = np.random.default_rng(seed)
    lon = rng.uniform(-117.95, -115.05, n); lat = rng.uniform(33.05, 34.95, n)
    lon[:2] = (-117.95, -115.05); lat[:2] = (33.05, 34.95)  # the extent does not hang on the draw
    v = series(nd, n, seed + 1)
    v[:, 5] = np.nan
    return lon, lat, v


def test_host_arrays_and_device_tensors_give_identical_bytes():
    import torch
    lon, lat, v = _network()
    h = R.grid_statistics(lon, lat, v, spacing=0.5)
    d = R.grid_statistics(torch.from_numpy(lon).cuda(), torch.from_numpy(lat).cuda(), torch.from_numpy(v).cuda(), spacing=0.5)
    for k in ST + OF + AB + ('grid_heatmap',) + tuple(MAPS):
        a, b = getattr(h, k), getattr(d, k)
        assert hasattr(b, 'data_ptr') and b.is_cuda and isinstance(a, np.ndarray), k
        assert a.shape == tuple(b.shape) and np.ascontiguousarray(a).tobytes() == b.contiguous().cpu().numpy().tobytes(), k
    assert h.grid_heatmap.shape == (4, 6) and h.grid_heatmap.dtype == np.float64
    # medians=False: NaN arrays and maps for them, the rest unchanged
    m = R.grid_statistics(lon, lat, v, spacing=0.5, medians=False)
    for k in ST + OF + AB + ('grid_heatmap',) + tuple(MAPS):
        if 'median' in k:
            assert np.isnan(getattr(m, k)).all(), k
        else:
            assert np.ascontiguousarray(getattr(m, k)).tobytes() == np.ascontiguousarray(getattr(h, k)).tobytes(), k
    assert sorted(m.maps()) == sorted(set(('grid_heatmap',) + tuple(MAPS)) - {'grid_delay_median', 'grid_delay_absolute_median'})


def test_station_order_is_restored_and_stations_outside_the_grid_get_nan():
    lon, lat, v = _network()
    bbox = [33.0, 35.0, -117.0, -115.0]                     # S N W E: the westernmost degree is outside
    a = R.grid_statistics(lon, lat, v, bbox=bbox)
    grid = V.station_grid(lon, lat, 1.0, bbox)
    vs = np.ascontiguousarray(v[:, grid.order])
    yard = yardstick(vs, grid.start)
    inside = grid.cell >= 0
    assert (~inside).sum() > 10 and inside.sum() > 50
    for k in ST:
        got = getattr(a, k)
        assert got.shape == lon.shape
        if k == 'st_nobs':
            assert (got[~inside] == 0).all()
        else:
            assert np.isnan(got[~inside]).all(), k
    compare({**{k: getattr(a, k)[grid.order] for k in ST}, **{k: getattr(a, k) for k in OF + AB}}, yard, tag='bbox')
    perm = np.random.default_rng(9).permutation(lon.size)
    b = R.grid_statistics(lon[perm], lat[perm], v[:, perm], bbox=bbox)
    for k in ST:                                            # a station's own sums do not depend on where it stands
        assert getattr(b, k).tobytes() == getattr(a, k)[perm].tobytes(), k
    for k in ('nstations', 'cell_nobs', 'abs_median'):
        assert np.array_equal(getattr(b, k), getattr(a, k), equal_nan=True), k
    assert np.array_equal(a.grid_heatmap, np.where(a.nstations > 0, a.nstations.astype(float), np.nan).reshape(grid.grid_dim).T, equal_nan=True)


# ---- golden g22: the reference's create_DF ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag,spacing', [('s1', 1.0), ('s05', 0.5)])
def test_golden_g22(tag, spacing):
    g = np.load(GOLDEN)
    lon, lat, v = g['lon'], g['lat'], g['values']
    res = R.grid_statistics(lon, lat, v, spacing=spacing)
    assert res.plotbbox == g[f'{tag}_plotbbox'].tolist() and list(res.grid.grid_dim) == g[f'{tag}_grid_dim'].tolist()
    assert np.array_equal(res.grid_heatmap, g[f'{tag}_grid_heatmap'], equal_nan=True)
    assert res.st_nobs[int(g['rowless_station'])] == 0 and res.st_nobs[int(g['lone_station'])] == 1
    yard = yardstick(np.ascontiguousarray(v[:, res.grid.order]), res.grid.start)
    gmap = lambda a: np.asarray(a).reshape(res.grid.grid_dim).T
    for name, k in MAPS.items():
        got, want = getattr(res, name), g[f'{tag}_{name}']
        assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want)), name
        ok = ~np.isnan(want)
        if name == 'grid_delay_absolute_median':
            assert got[ok].tobytes() == want[ok].tobytes(), name
            continue
        err = np.abs(got[ok] - want[ok]); tol = gmap(yard[k][1])[ok]
        print(f'g22 {tag} {name}: max |d| {err.max():.3e}, largest share of twice its bound {(err / (2 * tol)).max():.3f}')
        assert (err <= 2 * tol).all(), (name, err, tol)
    if tag == 's1':
        assert np.isnan(res.grid_delay_stdev[1, 0]) and not np.isnan(res.grid_delay_mean[1, 0])       # the lone single-row station


# ---- the C ABI: refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loc', [L.RDR_HOST, L.RDR_DEVICE], ids=['host', 'device'])
def test_refusals_leave_the_outputs_untouched(loc):
    import torch
    ctx = R.Context.default()
    n, nd, nc = 7, 3, 3
    v = series(nd, n, 11)
    i64 = lambda a: np.array(a, dtype=np.int64)
    host = dict(v=v, cs=i64([0, 4, 4, 7]), cs_first=i64([1, 4, 4, 7]), cs_last=i64([0, 4, 4, 6]), cs_down=i64([0, 5, 4, 7]),
                cs_slots=i64([0, 524289, 1 << 20, 1 << 20]))
    for k in ST + OF + AB:
        host[k] = np.full(n if k in ST else nc, -7, dtype=np.int64 if k in ('st_nobs', 'nstations', 'cell_nobs') else np.float64)
    if loc == L.RDR_DEVICE:
        bufs = {k: torch.from_numpy(a).cuda() for k, a in host.items()}
        torch.cuda.synchronize()
        read = lambda k: bufs[k].cpu().numpy()
    else:
        bufs = {k: a.copy() for k, a in host.items()}
        read = lambda k: bufs[k]

    def gs(v_='v', cs='cs', n_=n, nd_=nd, nc_=nc, loc_=loc, **null):
        p = lambda k: None if null.get(k, k) is None else L.ptr(bufs[k])
        return ctx.lib.rdr_grid_stats(ctx.handle, None if v_ is None else L.ptr(bufs[v_]), n_, nd_, None if cs is None else L.ptr(bufs[cs]), nc_,
                                      *[p(k) for k in ST + OF + AB], loc_)
    none = lambda *ks: {k: None for k in ks}
    for kw, text in ((dict(v_=None), 'NULL argument'), (dict(cs=None), 'NULL argument'), (dict(loc_=2), 'loc must be RDR_HOST or RDR_DEVICE'),
                     (dict(loc_=-1), 'loc must be RDR_HOST or RDR_DEVICE'), (dict(n_=0), 'n must be 1 .. 2^20 stations (got 0)'),
                     (dict(n_=(1 << 20) + 1), 'n must be 1 .. 2^20 stations'), (dict(nd_=0), 'nd must be 1 .. 4096 dates (got 0)'),
                     (dict(nd_=4097), 'nd must be 1 .. 4096 dates (got 4097)'), (dict(nc_=0), 'ncells must be 1 .. 2^20 cells (got 0)'),
                     (dict(nc_=(1 << 20) + 1), 'ncells must be 1 .. 2^20 cells'),
                     (dict(cs='cs_first'), 'cell_start[0] must be 0 (got 1)'), (dict(cs='cs_last'), 'cell_start[ncells] must be n = 7 (got 6)'),
                     (dict(cs='cs_down'), 'cell_start is not ascending at index 2'),
                     (none('st_mean'), 'st_nobs, st_mean and st_stdev come together'), (none('st_nobs', 'st_mean', 'st_stdev'), 'st_median only with them'),
                     (none('nstations'), 'nstations, mean_of_means and mean_of_stdevs come together'),
                     (none('nstations', 'mean_of_means', 'mean_of_stdevs'), 'mean_of_medians only with them'),
                     (none('abs_stdev'), 'cell_nobs, abs_mean and abs_stdev come together'), (none('cell_nobs', 'abs_mean', 'abs_stdev'), 'abs_median only with them'),
                     (none(*(ST + OF + AB)), 'every output group is NULL'),
                     # 524289 stations x 4096 dates = 2^31 + 4096 slots: refused on cell_start alone, before `values` is looked at
                     (dict(cs='cs_slots', n_=1 << 20, nd_=4096), 'cell 0 holds more than 2^31 - 1 slots (524289 stations x 4096 dates)')):
        assert gs(**kw) == L.RDR_ERR_INVALID, kw
        assert text in L.last_error(ctx.handle), (text, L.last_error(ctx.handle))
    ctx.synchronize()
    for k in ST + OF + AB:                                  # the sentinels are still there
        assert np.array_equal(read(k), host[k]), k
    assert gs() == L.RDR_OK                                 # and the same buffers make a valid call
    ctx.synchronize()
    compare({k: read(k) for k in ST + OF + AB}, yardstick(v, host['cs']), tag='after the refusals')
