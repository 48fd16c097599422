"""CPU: the host logic of the temporal interpolation (raider_amd/time_interp.py) against the reference's answers (golden g16,
tools/gen_golden_time_interp.py) and the planning of tropo_delay_interp_series with the device calls replaced by recorders."""
import datetime as dt
import logging
from types import SimpleNamespace

import numpy as np
import pytest

EPOCH = dt.datetime(2020, 1, 1)
T = lambda s: EPOCH + dt.timedelta(seconds=float(s))


def test_nearest_times_and_weights_equal_the_reference(golden):
    from raider_amd.time_interp import get_nearest_wmtimes, get_weights_time_interp
    g = golden('g16_time_interp')
    assert str(g['epoch']) == EPOCH.isoformat()
    assert set(g['nw_step_h']) == {1, 3, 6} and (g['nw_n'] == 1).any() and (g['nw_n'] == 2).any()
    for q, step, n, t1, t2, w1, w2 in zip(*(g[k] for k in ('nw_query_s', 'nw_step_h', 'nw_n', 'nw_t1_s', 'nw_t2_s', 'nw_w1', 'nw_w2'))):
        got = get_nearest_wmtimes(T(q), int(step))
        assert isinstance(got, list) and len(got) == n and got[0] == T(t1) and got[-1] == T(t2), (T(q), step, got)
        if n == 2:
            w = get_weights_time_interp(got, T(q))
            assert w[0] == w1 and w[1] == w2                                  # the same expressions on the same doubles: the same bits
            assert np.isclose(w[0] + w[1], 1)
    # the reference's docstring example (utilFcns.py:885-887)
    assert get_nearest_wmtimes(dt.datetime(2020, 1, 1, 11, 35, 0), 3) == [dt.datetime(2020, 1, 1, 9, 0), dt.datetime(2020, 1, 1, 12, 0)]
    # the known answers of the reference's test/test_temporal_interpolate.py
    for t1, t2, q, w1, loose in zip(*(g[k] for k in ('ka_t1_s', 'ka_t2_s', 'ka_query_s', 'ka_w1', 'ka_allclose'))):
        w = get_weights_time_interp([T(t1), T(t2)], T(q))
        assert np.isclose(w[0] + w[1], 1)
        if not loose:
            assert w[0] == w1 and w[1] == 1 - w1
        else:                  # that test compares delays with np.allclose (rtol 1e-5) against inverse-distance weights: 1 % of weight apart
            assert abs(w[0] - w1) < 0.01


def test_weights_that_do_not_sum_to_one_return_none(caplog):
    from raider_amd.time_interp import get_weights_time_interp
    with caplog.at_level(logging.ERROR):
        assert get_weights_time_interp([dt.datetime(2020, 1, 1, 12), dt.datetime(2020, 1, 1, 15)], dt.datetime(2020, 1, 1, 17)) is None
    assert 'Time interpolation weights do not sum to one' in caplog.text


def test_round_date_and_round_time():
    from raider_amd.time_interp import get_dt, round_date, round_time
    assert get_dt(dt.datetime(2020, 1, 1, 5), dt.datetime(2020, 1, 1, 0)) == 18000.0 and get_dt(dt.datetime(2020, 1, 1), dt.datetime(2020, 1, 1, 5)) == 18000.0
    h = lambda n: dt.timedelta(hours=n)
    assert round_date(dt.datetime(2020, 1, 1, 11, 35), h(3)) == dt.datetime(2020, 1, 1, 12)
    assert round_date(dt.datetime(2020, 1, 1, 22, 40), h(3)) == dt.datetime(2020, 1, 2, 0)
    assert round_date(dt.datetime(2020, 1, 1, 10, 30), h(3)) == dt.datetime(2020, 1, 1, 9)          # a tie rounds down (utilFcns.py:339)
    assert round_date(dt.datetime(2020, 1, 1, 6), h(6)) == dt.datetime(2020, 1, 1, 6)
    assert round_time(dt.datetime(2020, 1, 1, 10, 30), 3 * 3600) == dt.datetime(2020, 1, 1, 12)     # a tie rounds up (utilFcns.py:427)
    assert round_time(dt.datetime(2020, 1, 1, 23, 40, 0, 250000), 3600) == dt.datetime(2020, 1, 2, 0)


def test_get_weather_file_cases_equal_the_reference(golden, monkeypatch, caplog):
    from raider_amd import time_interp as TI
    g = golden('g16_time_interp')
    files = [f'/data/weather_files/HRRR_2020_01_01_T{h:02d}_00_00_32N_36N_121W_114W.nc' for h in (12, 13, 11)]
    calls = []
    monkeypatch.setattr(TI, 'combine_weather_files', lambda wfiles, time, model, interp_method='center_time', **kw: calls.append((interp_method, kw)) or 'combined')
    seen = set()
    for method, nfiles, ntimes, verdict in zip(g['gw_method'], g['gw_nfiles'], g['gw_ntimes'], g['gw_verdict']):
        method, verdict = str(method), str(verdict)
        calls.clear(); caplog.clear()
        try:
            with caplog.at_level(logging.WARNING):
                got = TI.getWeatherFile(files[:nfiles], list(range(ntimes)), dt.datetime(2020, 1, 1, 12, 20), 'HRRR', method)
            mine = 'none' if got is None else 'combine' if got == 'combined' else 'file0'
            assert mine != 'file0' or got == files[0]
            assert (mine == 'combine') == (len(calls) == 1) and (not calls or calls[0][0] == method)
        except Exception as exc:
            mine = type(exc).__name__
        assert mine == verdict, (method, nfiles, ntimes, mine, verdict)
        seen.add((method, verdict))
        if mine == 'none':
            assert 'No weather model data was successfully processed.' in caplog.text
        if method == 'center_time' and nfiles == ntimes and mine == 'file0':
            assert 'Time interpolation is not needed as exact time is available' in caplog.text
        if method == 'center_time' and nfiles == 1 and ntimes != 1:
            assert 'One datetime is not available to download, defaulting to nearest available date' in caplog.text
    assert {('none', 'file0'), ('center_time', 'combine'), ('center_time', 'file0'), ('center_time', 'WrongNumberOfFiles'), ('azimuth_time_grid', 'combine'),
            ('azimuth_time_grid', 'WrongNumberOfFiles'), ('nearest', 'ValueError'), ('none', 'none')} <= seen
    assert issubclass(TI.WrongNumberOfFiles, Exception) and str(TI.WrongNumberOfFiles(2, 3)).startswith('The number of files downloaded does not match')


def test_combined_file_names_equal_the_reference(golden):
    from raider_amd.time_interp import STYLE, combined_file_name
    g = golden('g16_time_interp')
    for first, q, name in zip(g['fn_first'], g['fn_query_s'], g['fn_name']):
        got = combined_file_name(f'/data/wm/{first}', T(q), 'center_time')
        assert got.name == str(name) and str(got.parent) == '/data/wm'
    assert combined_file_name('GMAO_2020_01_24_T12_00_00_32N_36N_121W_114W.nc', dt.datetime(2020, 1, 24, 13, 52, 44),
                              'center_time').name == 'GMAO_2020_01_24T13_52_44_timeInterp_32N_36N_121W_114W.nc'
    assert STYLE['azimuth_time_grid'] == str(g['fn_style_azimuth'])
    assert combined_file_name('HRRR_2020_01_24_T12_00_00_32N_36N_121W_114W.nc', dt.datetime(2020, 1, 24, 13, 52, 44),
                              'azimuth_time_grid').name == 'HRRR_2020_01_24T13_52_44_timeInterpAziGrid_32N_36N_121W_114W.nc'


def test_combine_refuses_before_the_device():
    from raider_amd.time_interp import NoWeatherModelData, combine_weather_files
    with pytest.raises(ValueError, match='not available with interpolation method "none"'):
        combine_weather_files([], dt.datetime(2020, 1, 1), 'GMAO', interp_method='none')
    with pytest.raises(NoWeatherModelData):
        combine_weather_files([], dt.datetime(2020, 1, 1), 'GMAO', times=[])


# ---- planning of the series with recorders in place of the device calls ------------------------------------------------------------
def _recorders(monkeypatch):
    from raider_amd import delay as D
    from raider_amd import time_interp as TI
    rec = SimpleNamespace(combine=[], series=[], points=[])

    def combine(wfiles, time, model, interp_method='center_time', orbit=None, write=False, times=None, ctx=None):
        rec.combine.append(dict(wfiles=list(wfiles), time=time, model=model, method=interp_method, orbit=orbit, times=list(times)))
        return ('combined', time)

    def series(which):
        def run(datetimes, files, aoi, los, height_levels=None, out_proj=4326, zref=None):
            which.append(dict(datetimes=list(datetimes), files=list(files), aoi=aoi, los=los, height_levels=height_levels, out_proj=out_proj, zref=zref))
            res = D.SeriesResult([(SimpleNamespace(attrs={}), None) if which is rec.series else (np.zeros(1), np.ones(1)) for _ in datetimes])
            res.routes = ['stacked'] * len(res)
            return res
        return run
    monkeypatch.setattr(TI, 'combine_weather_files', combine)
    monkeypatch.setattr(D, 'tropo_delay_series', series(rec.series))
    monkeypatch.setattr(D, 'tropo_delay_point_series', series(rec.points))
    return rec


DATES = [dt.datetime(2020, 1, 1, 13, 52, 44), dt.datetime(2020, 1, 13, 13, 52, 44), dt.datetime(2020, 1, 25, 13, 52, 44)]


def _models(step):
    out = {}
    for d in DATES:
        day = dt.datetime(d.year, d.month, d.day)
        for h in range(0, 25, step):
            out[day + dt.timedelta(hours=h)] = f'/wm/GMAO_{(day + dt.timedelta(hours=h)):%Y_%m_%d_T%H_%M_%S}_32N_36N_121W_114W.nc'
    return out


def test_series_requests_the_right_model_times_and_stacks_once(monkeypatch):
    from raider_amd.delay import GridAOI, PointsAOI
    from raider_amd.time_interp import tropo_delay_interp_series
    grid = GridAOI(np.linspace(0.0, 1.0, 3), np.linspace(1.0, 0.0, 3))
    los = SimpleNamespace()
    # center_time, 3 h step: 12:00 and 15:00 of every date; ONE stacked call for the three dates
    rec = _recorders(monkeypatch)
    models = _models(3)
    res = tropo_delay_interp_series(DATES, models, grid, los, height_levels=[0.0, 100.0], zref=9000.0, interpolate_time='center_time', time_step_hours=3, model_name='GMAO')
    assert [c['times'] for c in rec.combine] == [[d.replace(hour=12, minute=0, second=0), d.replace(hour=15, minute=0, second=0)] for d in DATES]
    assert [c['wfiles'] for c in rec.combine] == [[models[t] for t in c['times']] for c in rec.combine]
    assert all(c['method'] == 'center_time' and c['model'] == 'GMAO' for c in rec.combine)
    assert len(rec.series) == 1 and not rec.points
    call = rec.series[0]
    assert call['datetimes'] == DATES and call['files'] == [('combined', d) for d in DATES]
    assert call['aoi'] is grid and call['los'] is los and call['height_levels'] == [0.0, 100.0] and call['zref'] == 9000.0 and call['out_proj'] == 4326
    assert res.routes == ['stacked'] * 3
    for (ds, hydro), d in zip(res, DATES):
        assert hydro is None and ds.attrs == dict(model_name='GMAO', interpolation_method='center_time',
                                                  model_times_used=[d.strftime('%Y%m%dT12:00:00'), d.strftime('%Y%m%dT15:00:00')])
    # the step defaults to 6 h
    rec = _recorders(monkeypatch)
    tropo_delay_interp_series(DATES[:1], _models(6), grid, los, interpolate_time='center_time')
    assert rec.combine[0]['times'] == [dt.datetime(2020, 1, 1, 12), dt.datetime(2020, 1, 1, 18)]
    # none: the one model time round_date gives, the file itself, no combination; a points AOI goes to the point series
    rec = _recorders(monkeypatch)
    pts = PointsAOI(np.array([0.5]), np.array([0.5]), np.array([0.0]))
    models = _models(3)
    res = tropo_delay_interp_series(DATES, models, pts, los, interpolate_time='none', time_step_hours=3)
    assert not rec.combine and not rec.series and len(rec.points) == 1
    assert rec.points[0]['files'] == [models[d.replace(hour=15, minute=0, second=0)] for d in DATES]          # 13:52:44 is nearer to 15:00
    assert all(isinstance(r[0], np.ndarray) for r in res)                                                     # (no attributes on point results)
    # azimuth_time_grid, 1 h step: the three model times around the acquisition, the orbit handed on
    rec = _recorders(monkeypatch)
    models = _models(1)
    orbit = object()
    az_dates = [DATES[0], dt.datetime(2020, 1, 13, 13, 1, 0)]
    tropo_delay_interp_series(az_dates, models, grid, los, interpolate_time='azimuth_time_grid', time_step_hours=1, model_name='HRRR', orbit=orbit)
    # within one step + 300 s (s1_azimuth_timing.py:269-323): 13:52:44 has 14:00 and 13:00 (15:00 is 4036 s away); 13:01:00 has three
    assert [c['times'] for c in rec.combine] == [[dt.datetime(2020, 1, 1, 14), dt.datetime(2020, 1, 1, 13)],
                                                 [dt.datetime(2020, 1, 13, 13), dt.datetime(2020, 1, 13, 14), dt.datetime(2020, 1, 13, 12)]]
    assert all(c['method'] == 'azimuth_time_grid' and c['orbit'] is orbit for c in rec.combine)
    assert len(rec.series) == 1
    with pytest.raises(NotImplementedError, match='Only none, center_time, and azimuth_time_grid'):
        tropo_delay_interp_series(DATES[:1], models, grid, los, interpolate_time='linear')


def test_series_missing_file_rules(monkeypatch, caplog):
    from raider_amd.delay import GridAOI
    from raider_amd.time_interp import DatetimeFailed, NoWeatherModelData, tropo_delay_interp_series
    grid = GridAOI(np.linspace(0.0, 1.0, 3), np.linspace(1.0, 0.0, 3))
    los = SimpleNamespace()
    # center_time skips a missing file: one file is left, the reference's warning, no combination
    rec = _recorders(monkeypatch)
    models = _models(3)
    del models[dt.datetime(2020, 1, 13, 15)]
    with caplog.at_level(logging.WARNING):
        tropo_delay_interp_series(DATES, models, grid, los, interpolate_time='center_time', time_step_hours=3, model_name='GMAO')
    assert 'One datetime is not available to download, defaulting to nearest available date' in caplog.text
    assert len(rec.combine) == 2 and rec.series[0]['files'][1] == models[dt.datetime(2020, 1, 13, 12)]
    # a date within the threshold of a model time asks for that one time only
    rec = _recorders(monkeypatch); caplog.clear()
    with caplog.at_level(logging.WARNING):
        tropo_delay_interp_series([dt.datetime(2020, 1, 1, 12, 0, 30)], models, grid, los, interpolate_time='center_time', time_step_hours=3)
    assert not rec.combine and rec.series[0]['files'] == [models[dt.datetime(2020, 1, 1, 12)]]
    assert 'Time interpolation is not needed as exact time is available' in caplog.text
    # none left: NoWeatherModelData; the other two methods do not go on without a file
    with pytest.raises(NoWeatherModelData, match='Weather model processing failed for all times'):
        tropo_delay_interp_series(DATES[:1], {}, grid, los, interpolate_time='center_time', time_step_hours=3)
    with pytest.raises(DatetimeFailed, match='Weather model GMAO failed to download for datetime 2020-01-13 15:00:00'):
        tropo_delay_interp_series(DATES, models, grid, los, interpolate_time='none', time_step_hours=3, model_name='GMAO')
    hourly = _models(1)
    del hourly[dt.datetime(2020, 1, 1, 14)]
    with pytest.raises(DatetimeFailed):
        tropo_delay_interp_series(DATES[:1], hourly, grid, los, interpolate_time='azimuth_time_grid', time_step_hours=1, model_name='HRRR', orbit=object())


def test_public_names():
    import raider_amd as R
    for name in ('get_dt', 'round_date', 'round_time', 'get_nearest_wmtimes', 'get_weights_time_interp', 'getWeatherFile', 'combine_weather_files',
                 'tropo_delay_interp', 'tropo_delay_interp_series', 'WrongNumberOfFiles', 'DatetimeFailed', 'NoWeatherModelData'):
        assert hasattr(R, name), name
