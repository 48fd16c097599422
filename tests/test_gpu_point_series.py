"""GPU: tropo_delay_point_series - a date series at stations for every line of sight - against the loop of tropo_delay calls it
replaces: the same bytes, the same "missing delay values" log lines, the first exception in date order."""
import datetime as dt
import logging

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HL = [0.0, 500.0, 1500.0, 3000.0]
XP = np.linspace(-119.5, -115.5, 31); YP = np.linspace(34.5, 31.5, 27)            # 31 x 27 intermediate grid x 4 heights


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _wm(c, scale=1.0, hole=False):
    """a processed weather model as a mapping (file order (z, y, x)); hole: a NaN block over the scene in all four fields"""
    d = dict(x=c['xs'], y=c['ys'], z=c['zs'])
    for k in ('wet', 'hydro', 'wet_total', 'hydro_total'):
        a = (c[k] * scale).astype(c[k].dtype)
        if hole:
            a[:, 16:22, 14:22] = np.nan
        d[k] = a
    return d


def _files(n, hole=1):
    from raider_amd.synthetic import synthetic_cube
    return [_wm(synthetic_cube(40, 44, 24, seed=10 + e), 1.0 + 0.03 * e, hole=(e == hole)) for e in range(n)]


def _dates(n):
    return [dt.datetime(2020, 1, 1) + dt.timedelta(days=12 * i) for i in range(n)]


def _stations(n=300, seed=3):
    rng = np.random.default_rng(seed)
    return rng.uniform(32.0, 34.0, n), rng.uniform(-119.0, -116.0, n), rng.uniform(0.0, 2900.0, n), rng.uniform(30.0, 45.0, n)


def _critical(caplog, fn):
    caplog.clear()
    with caplog.at_level(logging.CRITICAL):
        out = fn()
    return out, [r.getMessage() for r in caplog.records if r.levelno >= logging.CRITICAL]


def _series_vs_loop(files, aoi_factory, los, out_proj, caplog, routes):
    from raider_amd.delay import tropo_delay, tropo_delay_point_series
    dates = _dates(len(files))
    ser, crit_s = _critical(caplog, lambda: tropo_delay_point_series(dates, files, aoi_factory(), los, HL, out_proj))
    loop, crit_l = _critical(caplog, lambda: [tropo_delay(t, f, aoi_factory(), los, HL, out_proj) for t, f in zip(dates, files)])
    assert len(ser) == len(loop)
    assert crit_s == crit_l and sum('missing delay values' in m for m in crit_l) == sum(1 for f in files if np.isnan(f['wet_total']).any())
    for e, (a, b) in enumerate(zip(ser, loop)):
        assert _same(a[0], b[0]) and _same(a[1], b[1]), e
    assert ser.routes == routes, ser.routes
    return ser


@pytest.mark.parametrize('crs', [4326, 32611])
@pytest.mark.parametrize('los_kind', ['zenith', 'conventional', 'raytracing'])
def test_series_equals_the_loop(los_kind, crs, caplog):
    from raider_amd.delay import PointsAOI, transformPoints
    from raider_amd.losreader import Conventional, Raytracing, Zenith
    la, lo, hg, inc = _stations()
    los = {'zenith': lambda: Zenith(), 'conventional': lambda: Conventional(inc=inc, heading=0 * inc),
           'raytracing': lambda: Raytracing(inc=39.0, heading=-167.9)}[los_kind]()
    if crs == 4326:
        xp, yp = XP, YP
    else:                                                              # the same scene as a 31 x 27 grid in UTM zone 11 N
        yx = transformPoints(la, lo, 0 * la, 4326, crs)
        xp = np.linspace(yx[:, 1].min() - 5000.0, yx[:, 1].max() + 5000.0, 31); yp = np.linspace(yx[:, 0].max() + 5000.0, yx[:, 0].min() - 5000.0, 27)
    files = _files(4)
    ser = _series_vs_loop(files, lambda: PointsAOI(la, lo, hg, xp, yp), los, crs, caplog, ['stacked'] * 4)
    w0, w1 = np.asarray(ser[0][0]), np.asarray(ser[1][0])
    assert w0.shape == (300,) and np.isfinite(w0).all() and 0 < np.isnan(w1).sum() < 300 and not _same(w0, np.asarray(ser[2][0]))


def test_mixed_routes_single_date_and_exceptions_in_date_order(caplog):
    from raider_amd.delay import PointsAOI, tropo_delay_point_series, tropo_delay_series
    from raider_amd.losreader import Conventional, Raytracing, Zenith
    la, lo, hg, inc = _stations(100, seed=4)
    files = _files(3, hole=2)
    aoi = lambda: PointsAOI(la, lo, hg, XP, YP)
    conv = Conventional(inc=inc, heading=0 * inc)
    # one date on another z axis: the others still share their call
    odd = dict(files[1], z=files[1]['z'] + 1.0)
    for los in (Zenith(), conv, Raytracing(inc=39.0, heading=-167.9)):
        _series_vs_loop([files[0], odd, files[2]], aoi, los, 4326, caplog, ['stacked', 'per-date', 'stacked'])
    # a single date, and two dates that do not agree: per date
    _series_vs_loop(files[:1], aoi, Zenith(), 4326, caplog, ['per-date'])
    _series_vs_loop([files[0], odd], aoi, conv, 4326, caplog, ['per-date', 'per-date'])
    # a one-node intermediate axis is nothing the one-call route takes: the loop's own host sequence answers
    from raider_amd.delay import tropo_delay
    one = lambda: PointsAOI(la, lo, hg, XP, YP[:1])
    try:
        want = [tropo_delay(t, f, one(), Zenith(), HL) for t, f in zip(_dates(2), files[:2])]
    except Exception as exc:
        with pytest.raises(type(exc)):
            tropo_delay_point_series(_dates(2), files[:2], one(), Zenith(), HL)
    else:
        got = tropo_delay_point_series(_dates(2), files[:2], one(), Zenith(), HL)
        assert got.routes == ['per-date'] * 2 and all(_same(a[0], b[0]) and _same(a[1], b[1]) for a, b in zip(got, want))
    # an exception on one date surfaces in date order, as the loop raises it: here the second file lacks its total fields
    broken = {k: v for k, v in files[1].items() if k not in ('wet_total', 'hydro_total')}
    with pytest.raises(Exception) as loop_exc:
        [tropo_delay(t, f, aoi(), Zenith(), HL) for t, f in zip(_dates(3), [files[0], broken, files[2]])]
    with pytest.raises(type(loop_exc.value)) as ser_exc:
        tropo_delay_point_series(_dates(3), [files[0], broken, files[2]], aoi(), Zenith(), HL)
    assert str(ser_exc.value) == str(loop_exc.value)
    # tropo_delay_series keeps its routing: zenith and projected stations go date by date there
    for los in (Zenith(), conv):
        assert tropo_delay_series(_dates(3), files, aoi(), los, HL).routes == ['per-date'] * 3
    with pytest.raises(ValueError, match='3 dates but 2'):
        tropo_delay_point_series(_dates(3), files[:2], aoi(), Zenith(), HL)


def test_per_date_divisors_reach_the_device_stacked(caplog):
    """a projected line of sight whose divisor differs by date (what an orbit file gives after setTime): the stacked call takes the
    [D, n] divisors and still equals the loop"""
    from raider_amd.delay import PointsAOI
    from raider_amd.losreader import Conventional
    la, lo, hg, inc = _stations(100, seed=5)

    class DriftingLOS(Conventional):
        def _divisor_source(self):
            day = (self._time - dt.datetime(2020, 1, 1)).days
            return 'div', np.cos(np.deg2rad(self._inc + 0.01 * day))

    files = _files(3)
    _series_vs_loop(files, lambda: PointsAOI(la, lo, hg, XP, YP), DriftingLOS(inc=inc, heading=0 * inc), 4326, caplog, ['stacked'] * 3)
