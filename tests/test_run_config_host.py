"""The run-configuration layer on the host: raider_amd.run_config / models / checkArgs / processWM / cli against what the reference
answers (tests/golden/g18_run_config.npz, written by tools/gen_golden_run_config.py) and against cases written out here for what the
reference cannot run under the generator's stand-ins (box containment, the raster extension).  No GPU: where a device step would
run (raster bounds, the raw-file producer, the series call) it is stubbed, as tests/test_point_series_host.py stubs plans."""
import datetime as dt
import json
import logging
from pathlib import Path

import numpy as np
import pytest

GOLD = Path(__file__).resolve().parent / 'golden'
FILES = GOLD / 'ref_files'
STATIONS = FILES / 'scenario_6_stations.csv'


@pytest.fixture(scope='module')
def g18(golden):
    g = golden('g18_run_config')
    return lambda k: json.loads(str(g[k])) if g[k].dtype.kind == 'U' and g[k].ndim == 0 and str(g[k])[:1] in '[{' else g[k]


def outcome(fn):
    try:
        return ['ok', fn()]
    except Exception as exc:
        return ['raise', [type(exc).__name__, str(exc)]]


# ---- g18: parsing ----------------------------------------------------------------------------------------------------------
def test_parse_dates_as_the_reference(g18):
    from raider_amd.run_config import DateGroupUnparsed, parse_dates
    cases, want = g18('dt_cases'), g18('dt_results')
    assert len(cases) >= 12
    got = [outcome(lambda c=c: [d.isoformat() for d in parse_dates(DateGroupUnparsed(**c)).date_list]) for c in cases]
    assert got == want


def test_time_group_as_the_reference(g18):
    from raider_amd.run_config import TimeGroup
    cases, want = g18('tm_cases'), g18('tm_results')

    def run(c):
        g = TimeGroup(**c)
        return [g.time.isoformat(), g.end_time.isoformat(), g.interpolate_time]
    got = [outcome(lambda c=c: run(c)) for c in cases]
    assert got == want
    assert sum(w[0] == 'raise' for w in want) >= 3
    # every entry of the format table is met by a case that parses
    assert {'T13:52:45.5', 'T135245.25', '135245.75', 'T13:52:45', '13:52:45', 'T135245', '135245', 'T13:52', 'T1352', '13:52', 'T13', ''} <= \
        {c.get('time') for c, w in zip(cases, want) if w[0] == 'ok'}
    assert TimeGroup(time=dt.time(1, 2, 3)).end_time == dt.time(1, 2, 33)


def test_parse_bbox_as_the_reference(g18):
    from raider_amd.run_config import parse_bbox
    cases, want = g18('bb_cases'), g18('bb_results')
    got = [outcome(lambda c=c: [float(v) for v in parse_bbox(c)]) for c in cases]
    assert got == want
    assert len({w[1][1] for w in want if w[0] == 'raise'}) == 4          # all four messages


def test_get_heights_as_the_reference(g18, caplog):
    from raider_amd.run_config import AOIGroupUnparsed, HeightGroupUnparsed, RuntimeGroup, get_heights
    cases, want = g18('hg_cases'), g18('hg_results')

    def run(c):
        aoi = dict(c['aoi'])
        if 'station_file' in aoi:
            aoi['station_file'] = str(STATIONS)
        g = get_heights(HeightGroupUnparsed(**c['height']), AOIGroupUnparsed(**aoi), RuntimeGroup(output_directory='out_dir'))
        return dict(dem=None if g.dem is None else Path(g.dem).as_posix(), use_dem_latlon=g.use_dem_latlon, height_file_rdr=g.height_file_rdr,
                    height_levels=None if g.height_levels is None else [float(v) for v in g.height_levels])
    with caplog.at_level(logging.WARNING, logger='RAiDER'):
        got = [outcome(lambda c=c: run(c)) for c in cases]
    assert got == want
    below = sum(1 for w in want if w[0] == 'ok' and w[1]['height_levels'] and min(w[1]['height_levels']) < 0)
    assert below >= 1 and sum('height levels below the topography' in r.message for r in caplog.records) == below


def test_dem_coverage_check_uses_the_buffer(tmp_path):
    """validators.py:95-112: an existing DEM must hold the bounding box within 0.2 degrees."""
    from raider_amd.rawraster import write_envi
    from raider_amd.run_config import AOIGroupUnparsed, HeightGroupUnparsed, RuntimeGroup, get_heights
    dem = tmp_path / 'dem.dat'
    write_envi(np.zeros((11, 11), np.float32), dem, nodata=0.0, geotransform=(-92.0, 0.1, 0.0, 38.0, 0.0, -0.1), proj=4326)   # W..E = -92..-91, S..N = 37..38
    rt = RuntimeGroup(output_directory=str(tmp_path))
    ok = get_heights(HeightGroupUnparsed(dem=str(dem)), AOIGroupUnparsed(bounding_box='36.85 38.15 -92.15 -90.85'), rt)
    assert ok.dem == str(dem)
    with pytest.raises(ValueError, match='Existing DEM does not cover the area of the input lat/lon points'):
        get_heights(HeightGroupUnparsed(dem=str(dem)), AOIGroupUnparsed(bounding_box='36.7 38 -92 -91'), rt)


def test_delay_file_names_as_the_reference(g18):
    from raider_amd.checkArgs import makeDelayFileNames
    from raider_amd.losreader import Conventional, Raytracing, Zenith
    kinds = dict(Zenith=Zenith(), Conventional=Conventional(inc=30.0), Raytracing=Raytracing(inc=30.0, heading=-10.0), none=None)
    cases, want = g18('fn_cases'), g18('fn_results')
    assert len(cases) == 24
    for c, w in zip(cases, want):
        date = None if c['date'] is None else dt.datetime.fromisoformat(c['date'])
        got = makeDelayFileNames(date, kinds[c['los']], c['ext'], c['model'], Path(c['out']))
        assert [Path(p).as_posix() for p in got] == w, c


def test_raster_extensions():
    """What the reference's inverted rasterio table gives for GTiff is the name its own test reads: `..._ztd.tiff`
    (test/test_intersect.py:56); ENVI / ISCE carry the generic extension of checkArgs.py:104-105."""
    from raider_amd.checkArgs import get_raster_ext, makeDelayFileNames
    assert get_raster_ext('GTiff') == 'tiff' and get_raster_ext('gtiff') == 'tiff'
    assert get_raster_ext('ENVI') == '.dat' and get_raster_ext('isce') == '.dat'
    with pytest.raises(ValueError, match='nc is not a valid gdal/rasterio file format for rasters'):      # (the driver's name is NETCDF)
        get_raster_ext('nc')
    wet, hydro = makeDelayFileNames(dt.datetime(2020, 1, 30, 13, 52, 45), None, get_raster_ext('GTiff'), 'ERA5', Path('output'))
    assert hydro == 'output/ERA5_hydro_20200130T135245_ztd.tiff'
    with pytest.raises(ValueError, match='HFA is not a valid gdal/rasterio file format for rasters'):
        get_raster_ext('HFA')


# ---- g18: models -----------------------------------------------------------------------------------------------------------
def test_model_facts_bounds_and_file_names_as_the_reference(g18):
    from raider_amd import models as M
    facts, names = g18('md_facts'), [str(n) for n in g18('md_models')]
    assert set(names) >= {'ERA5', 'ERA5T', 'ERAI', 'HRES', 'GMAO', 'MERRA2', 'NCMR'}
    boxes, spacings, when = g18('md_boxes'), g18('md_spacings'), dt.datetime.fromisoformat(str(g18('md_when')))
    for name in names:
        m, f = getattr(M, name)(), facts[name]
        assert (m.Model(), m._dataset, m.dtime(), m._model_level_type) == (f['Model'], f['dataset'], f['dtime'], f['level_type']), name
        assert m._valid_range[0].isoformat() == f['valid_from']
        assert np.float64(m.getLLRes()).tobytes() == np.float64(g18(f'md_llres_{name}')).tobytes(), name
        want, k = g18(f'md_bounds_{name}'), 0
        for spacing in spacings:
            for b in boxes:
                m.set_latlon_bounds(list(b), output_spacing=None if np.isnan(spacing) else float(spacing))
                got = m.get_latlon_bounds()
                assert got.dtype == np.float64 and got.tobytes() == want[k].tobytes(), (name, b, spacing, got, want[k])     # bit for bit
                assert M.make_weather_model_filename(m.Model(), when, got) == f['filenames'][k]
                k += 1
        assert Path(M.make_raw_weather_data_filename('wm_dir', m.Model(), when)).as_posix() == f['raw_filename']
        m.setTime(when)
        m.set_wmLoc('wm_dir')
        assert Path(m.out_file(m.get_wmLoc())).as_posix() == 'wm_dir/' + f['filenames'][-1]


def test_projected_models_and_unknown_names(g18):
    from raider_amd import models as M
    from raider_amd.llreader import BoundingBox
    h, ak = M.HRRR(), M.HRRRAK()
    assert (h.Model(), h._dataset, h.dtime(), ak.Model(), ak._dataset, ak.dtime()) == ('HRRR', 'hrrr', 1, 'HRRR-AK', 'hrrrak', 3)      # hrrr.py:209-233,381-384
    assert h.getLLRes() == 3.0 / 111 and h._valid_range[0] == dt.datetime(2016, 7, 15, tzinfo=dt.timezone.utc)
    h._cast_to_hrrrak()
    assert (h.Model(), h._dataset, h.dtime(), h._proj) == (ak.Model(), ak._dataset, ak.dtime(), ak._proj)
    h6 = M.HRES()
    h6.set_latlon_bounds([37, 38, -92, -91])
    assert np.allclose(h6.get_latlon_bounds(), [37 - 6 * 9 / 111, 38 + 6 * 9 / 111, -92 - 6 * 9 / 111, -91 + 6 * 9 / 111], rtol=0, atol=1e-12)
    assert g18('md_unknown')[1][0] == 'ModuleNotFoundError'                  # ... which validators.py:40-45 turns into:
    for name in ('WRFX', 'hrrr-ak'):
        with pytest.raises(NotImplementedError, match=f'Model {name.upper().replace("-", "")} is not yet fully implemented, please contribute!'):
            M.parse_weather_model(name, BoundingBox([37, 38, -92, -91]))
    m = M.parse_weather_model('era-5', BoundingBox([37, 38, -92, -91]))
    assert m.Model() == 'ERA-5'
    with pytest.raises(ValueError, match='The requested location is unavailable for GMAO'):
        M.GMAO().checkValidBounds([95, 96, -92, -91])
    M.GMAO().checkValidBounds([10, 12, -200, -190])                          # meets the world after the move by 360 degrees


def test_check_time_against_range_and_lag():
    from raider_amd import models as M
    now = dt.datetime.now(dt.timezone.utc)
    e5 = M.ERA5()
    e5.checkTime(dt.datetime(2020, 1, 30, 13, 52, 45))
    for bad in (dt.datetime(1949, 12, 31), (now - dt.timedelta(days=30)).replace(tzinfo=None)):
        with pytest.raises(M.DatetimeOutsideRange, match='is outside the available date range for weather model ERA-5'):
            e5.checkTime(bad)
    with pytest.raises(M.DatetimeOutsideRange):
        M.ERAI().checkTime(dt.datetime(2019, 9, 1))
    M.HRRR().checkTime((now - dt.timedelta(hours=4)).replace(tzinfo=None))
    with pytest.raises(M.DatetimeOutsideRange):
        M.HRRR().checkTime((now - dt.timedelta(hours=2)).replace(tzinfo=None))
    with pytest.raises(ValueError, match='should be a Python datetime object'):
        e5.checkTime('2020-01-01')
    assert M._months_back(dt.datetime(2020, 5, 31), 3) == dt.datetime(2020, 2, 29)


# Six model extents as (W, S, E, N): the bounds in the names of the three processed ERA-5 cubes under tests/golden/ref_files, one on GMAO's
# 0.3125 degree longitudes, and two that leave the world box, east and west.  (The reference's own answers cannot be recorded: see the
# generator's text.  The expectations follow from weatherModel.py:510-531 read as geometry: closed containment; +-360 copies grown by 1e-5.)
CUBE_EXTENTS = [(-41.0, -5.0, -37.0, -2.0), (-120.0, 32.0, -115.0, 35.0), (-159.0, 69.0, -152.0, 73.0), (-93.4375, 36.25, -90.0, 38.75),
                (178.0, 9.0, 181.0, 13.0), (-181.5, -20.0, -178.0, -15.0)]
CONTAINMENT = [
    # (model box index, input SNWE, covered)
    (0, (-4.5, -2.5, -40.5, -37.5), True), (0, (-5.0, -2.0, -41.0, -37.0), True), (0, (-5.1, -2.0, -41.0, -37.0), False),
    (0, (-4.5, -2.5, -40.5, -36.9), False), (1, (33, 34, -118, -117), True), (1, (33, 34, -121, -117), False), (2, (70, 72, -158, -153), True),
    (2, (70, 73.5, -158, -153), False), (3, (37, 38, -92, -91), True), (3, (37, 38, -94, -91), False),
    # across +-180: the model's copies moved by 360 degrees count
    (4, (10, 12, 178.5, 180.5), True), (4, (10, 12, -181.5, -179.5), True), (4, (10, 12, 178.5, 181.5), False), (4, (10, 12, -179.5, -178.5), False),
    (4, (10, 12, 181.0, 181.00001), True), (4, (10, 12, 181.0, 181.1), False),
    (5, (-19, -16, 178.6, 181.9), True), (5, (-19, -16, -181, -179), True), (5, (-19, -16, 177, 179), False),
]


@pytest.mark.parametrize('which,snwe,covered', CONTAINMENT)
def test_box_containment(which, snwe, covered):
    """weatherModel.py:510-531 on boxes: plain containment inside the world box; a model extent that leaves it is taken with its copies
    moved by +-360 degrees, each grown by 1e-5 degrees."""
    from raider_amd.models import box_containment
    S, N, W, E = snwe
    assert box_containment(CUBE_EXTENTS[which], (W, S, E, N)) == (covered, False)


def test_world_wide_model_covers_everything():
    from raider_amd.models import box_containment
    assert box_containment((-180, -90, 180, 90), (-170, -80, 170, 80)) == (True, True)
    assert box_containment((-180.5, -90, 179.75, 90), (100, -80, 179.9, 80)) == (True, True)           # copies overlap: one band round the globe
    assert box_containment((-180, -89.75, 180, 90), (-170, -80, 170, 80)) == (True, False)


# ---- g18: checkArgs ----------------------------------------------------------------------------------------------------------
def _config(tmp_path, aoi, dates, time, runtime, los=None):
    from raider_amd import models as M
    from raider_amd import run_config as RC
    from raider_amd.losreader import Zenith
    rt = RC.RuntimeGroup(output_directory=str(tmp_path / 'output'), **runtime)
    return RC.RunConfig(weather_model=M.ERA5(), date_group=RC.parse_dates(RC.DateGroupUnparsed(**dates)), time_group=RC.TimeGroup(time=time),
                        aoi_group=RC.AOIGroup(aoi=aoi), height_group=RC.HeightGroup(None, False, None, None),
                        los_group=RC.LOSGroup(los=los or Zenith()), runtime_group=rt)


def test_check_args_as_the_reference(g18, tmp_path):
    from raider_amd.checkArgs import checkArgs
    from raider_amd.llreader import BoundingBox, StationFile
    cases, want = g18('ca_cases'), g18('ca_results')
    assert {c['kind'] for c in cases} == {'station', 'bbox'}
    for i, (c, w) in enumerate(zip(cases, want)):
        aoi = StationFile(STATIONS) if c['kind'] == 'station' else BoundingBox([37, 38, -92, -91])
        (tmp_path / str(i)).mkdir()
        cfg = checkArgs(_config(tmp_path / str(i), aoi, c['dates'], c['time'], c['runtime']))
        outdir = cfg.runtime_group.output_directory
        rel = lambda p: '' if p == '' else Path(p).relative_to(outdir).as_posix()
        assert [rel(p) for p in cfg.wetFilenames] == w['wet'] and [rel(p) for p in cfg.hydroFilenames] == w['hydro'], c
        assert [d.isoformat() for d in cfg.date_group.date_list] == w['dates']
        assert cfg.runtime_group.weather_model_directory.relative_to(outdir).as_posix() == w['wm_dir'] and cfg.runtime_group.weather_model_directory.is_dir()
        assert (cfg.weather_model.get_wmLoc() == str(cfg.runtime_group.weather_model_directory)) == w['wmLoc_is_wm_dir']
        if c['kind'] == 'station':
            assert Path(cfg.wetFilenames[0]).read_text() == w['csv']


def test_check_args_raster_names_orbit_warning_and_los_time(tmp_path, caplog):
    from raider_amd.checkArgs import checkArgs

    class Rasters:                       # (any AOI that is neither a bounding box nor a station file means rasters)
        def type(self):
            return 'radar_rasters'

    class Los:
        def setTime(self, t):
            self.time = t
    los = Los()
    cfg = _config(tmp_path, Rasters(), dict(date_list=[20200130, 20200131]), '13:52:45', {}, los=los)
    cfg.los_group.orbit_file = 'orbit.EOF'
    with caplog.at_level(logging.WARNING, logger='RAiDER'):
        cfg = checkArgs(cfg)
    assert [Path(p).name for p in cfg.wetFilenames] == ['ERA5_wet_20200130T135245_std.tiff', 'ERA5_wet_20200131T135245_std.tiff']
    assert [Path(p).name for p in cfg.hydroFilenames] == ['ERA5_hydro_20200130T135245_std.tiff', 'ERA5_hydro_20200131T135245_std.tiff']
    assert los.time == dt.datetime(2020, 1, 30, 13, 52, 45)
    assert sum('Only one orbit file is being used' in r.message for r in caplog.records) == 1


# ---- YAML -------------------------------------------------------------------------------------------------------------------
def _write_yaml(path, cfg):
    import yaml
    path.write_text(yaml.safe_dump(cfg))
    return path


BASE = dict(weather_model='ERA5', look_dir='right', date_group=dict(date_start=20200130), time_group=dict(time='13:52:45', interpolate_time='none'))


def test_yaml_round_trip_bounding_box(tmp_path, caplog):
    from raider_amd import run_config as RC
    from raider_amd.losreader import Zenith
    cfg = dict(BASE, aoi_group=dict(bounding_box='37 38 -92 -91', lat_file=None), height_group=dict(height_levels='0 100 500'),
               los_group=None, runtime_group=dict(output_directory=str(tmp_path / 'out')), cube_spacing_in_m=5000.0)
    with caplog.at_level(logging.WARNING, logger='RAiDER'):
        rc = RC.read_run_config_file(_write_yaml(tmp_path / 'run.yaml', cfg))
    assert any('cube_spacing_in_m is deprecated' in r.message for r in caplog.records)
    assert rc.aoi_group.aoi.type() == 'bounding_box' and rc.aoi_group.aoi.bounds() == [37.0, 38.0, -92.0, -91.0] and rc.aoi_group.aoi._cube_spacing_m == 5000.0
    assert rc.weather_model.Model() == 'ERA-5' and rc.look_dir == 'right' and rc.date_group.date_list == [dt.date(2020, 1, 30)]
    assert rc.time_group.time == dt.time(13, 52, 45) and rc.time_group.end_time == dt.time(13, 53, 15) and rc.time_group.interpolate_time == 'none'
    assert rc.height_group.height_levels == [0.0, 100.0, 500.0] and rc.height_group.dem == tmp_path / 'out' / 'GLO30.dem'
    assert isinstance(rc.los_group.los, Zenith) and rc.los_group.ray_trace is False and rc.los_group.zref is None
    rt = rc.runtime_group
    assert (rt.raster_format, rt.file_format, rt.output_projection, rt.verbose, rt.download_only) == ('GTiff', 'GTiff', 'EPSG:4326', True, False)
    assert rt.weather_model_directory == tmp_path / 'out' / 'weather_files' and rt.cube_spacing_in_m == 5000.0
    assert RC.RuntimeGroup().cube_spacing_in_m == 2000.0 and RC.RuntimeGroup().weather_model_directory == Path('weather_files')


def test_yaml_round_trip_station_file(tmp_path):
    from raider_amd import run_config as RC
    cfg = dict(BASE, aoi_group=dict(station_file=str(STATIONS)), runtime_group=dict(output_directory=str(tmp_path), weather_model_directory=str(FILES)))
    rc = RC.read_run_config_file(_write_yaml(tmp_path / 'run.yaml', cfg))
    aoi = rc.aoi_group.aoi
    assert aoi.type() == 'station_file' and str(aoi._filename) == str(STATIONS) and rc.runtime_group.weather_model_directory == FILES
    assert rc.height_group.dem == tmp_path / 'GLO30.dem'
    RC.require_dem(rc)                                    # the file has a Hgt_m column: nothing is asked for


def test_yaml_round_trip_lat_lon_rasters(tmp_path, monkeypatch):
    from raider_amd import llreader
    from raider_amd import run_config as RC
    from raider_amd.losreader import Conventional
    monkeypatch.setattr(llreader, 'bounds_from_latlon_rasters', lambda la, lo: ((15.76, 21.49, -101.64, -98.24), 4326, None))     # (a device pass)
    s4 = FILES / 'scenario_4'
    cfg = dict(BASE, look_dir='Left', aoi_group=dict(lat_file=str(s4 / 'lat.rdr'), lon_file=str(s4 / 'lon.rdr')), height_group=dict(dem=str(s4 / 'warpedDEM.dem')),
               los_group=dict(los_file=str(s4 / 'los.rdr'), zref=20000.0), runtime_group=dict(output_directory=str(tmp_path), raster_format='ENVI'))
    rc = RC.read_run_config_file(_write_yaml(tmp_path / 'run.yaml', cfg))
    aoi = rc.aoi_group.aoi
    assert aoi.type() == 'radar_rasters' and aoi._demfile == str(s4 / 'warpedDEM.dem') and aoi.bounds() == [15.76, 21.49, -101.64, -98.24]
    assert rc.look_dir == 'left' and isinstance(rc.los_group.los, Conventional) and rc.los_group.zref == 20000.0 and rc.runtime_group.raster_format == 'ENVI'
    RC.require_dem(rc)


def test_query_region_precedence(tmp_path, monkeypatch):
    from raider_amd import run_config as RC
    made = []
    for cls in ('GeocodedFile', 'RasterRDR', 'StationFile', 'BoundingBox', 'Geocube'):
        monkeypatch.setattr(RC, cls, lambda *a, _c=cls, **k: made.append((_c, a, k)) or _c)
    everything = RC.AOIGroupUnparsed(bounding_box='37 38 -92 -91', geocoded_file='x/SRTM_3.tif', lat_file='lat', lon_file='lon', station_file='s.csv', geo_cube='c.nc')
    assert RC.get_query_region(everything, RC.HeightGroupUnparsed(dem='d.dem', use_dem_latlon=True), 2000.0) == 'GeocodedFile' and made[-1][2]['is_dem'] is True
    assert RC.get_query_region(everything, RC.HeightGroupUnparsed(dem='d.dem', height_file_rdr='h'), 2000.0) == 'RasterRDR' and made[-1][1] == ('lat', 'lon', 'h', 'd.dem')
    order = ['StationFile', 'BoundingBox', 'GeocodedFile', 'Geocube']
    for drop, want in zip((('lat_file', 'lon_file'), ('station_file',), ('bounding_box',), ('geocoded_file',)), order):
        for k in drop:
            setattr(everything, k, None)
        assert RC.get_query_region(everything, RC.HeightGroupUnparsed(), 2000.0) == want
    assert made[-2][0] == 'GeocodedFile' and made[-2][2]['is_dem'] is True                  # the SRTM / GLO name rule
    for name, is_dem in (('glo_30.tif', True), ('scene.tif', False)):
        RC.get_query_region(RC.AOIGroupUnparsed(geocoded_file=name), RC.HeightGroupUnparsed(), None)
        assert made[-1][2]['is_dem'] is is_dem
    with pytest.raises(ValueError, match='Lats are out of S/N bounds'):
        RC.get_query_region(RC.AOIGroupUnparsed(bounding_box=[-95, 10, 0, 1]), RC.HeightGroupUnparsed(), None)


ERRORS = [
    (dict(time_group=dict(interpolate_time='none')), ValueError, 'You must specify a "time" in the input config file'),
    (dict(look_dir='up'), ValueError, 'Unknown look direction up'),
    (dict(look_dir=3), ValueError, 'Unknown look direction 3'),
    (dict(aoi_group=dict(lon_file='lon.rdr')), ValueError, 'A lon_file must be specified if a lat_file is specified'),
    (dict(aoi_group=None), ValueError, 'No valid query points or bounding box found in the configuration file'),
    (dict(los_group=dict(los_cube='los.nc')), NotImplementedError, 'LOS_cube is not yet implemented'),
    (dict(weather_model='WRF'), NotImplementedError, 'Model WRF is not yet fully implemented, please contribute!'),
    (dict(date_group=None), ValueError, 'Inputs must include either date_list or date_start'),
    (dict(aoi_group=dict(bounding_box='38 37 -92 -91')), ValueError, 'Bounding box has no size'),
]


@pytest.mark.parametrize('change,exc,text', ERRORS)
def test_configuration_errors(tmp_path, change, exc, text):
    from raider_amd.run_config import read_run_config_file
    cfg = dict(BASE, aoi_group=dict(bounding_box='37 38 -92 -91'), runtime_group=dict(output_directory=str(tmp_path)))
    cfg.update(change)
    with pytest.raises(exc, match=text):
        read_run_config_file(_write_yaml(tmp_path / 'run.yaml', cfg))


def test_broken_yaml(tmp_path):
    from raider_amd.run_config import read_run_config_file
    (tmp_path / 'run.yaml').write_text('look_dir: [right\n')
    with pytest.raises(ValueError, match='Something is wrong with the yaml file'):
        read_run_config_file(tmp_path / 'run.yaml')


def test_a_dem_that_would_be_downloaded_raises_with_its_path(tmp_path):
    from raider_amd import run_config as RC
    stations = tmp_path / 'stations.csv'
    stations.write_text('ID,Lat,Lon\nA,33.1,-116.8\nB,33.8,-118.3\n')
    cfg = dict(BASE, aoi_group=dict(station_file=str(stations)), runtime_group=dict(output_directory=str(tmp_path / 'out')))
    rc = RC.read_run_config_file(_write_yaml(tmp_path / 'run.yaml', cfg))
    with pytest.raises(RC.DEMNotFound, match='has no Hgt_m column') as e:
        RC.require_dem(rc)
    assert e.value.path == tmp_path / 'out' / 'GLO30.dem' and str(tmp_path / 'out' / 'GLO30.dem') in str(e.value) and isinstance(e.value, FileNotFoundError)
    (tmp_path / 'out').mkdir()
    (tmp_path / 'out' / 'GLO30.dem').write_bytes(b'')
    RC.require_dem(rc)
    assert rc.aoi_group.aoi._demfile == str(tmp_path / 'out' / 'GLO30.dem')


# ---- prepareWeatherModel ---------------------------------------------------------------------------------------------------
def _processed_file(path, xs, ys):
    from raider_amd.h5write import write_netcdf4
    xs, ys = np.asarray(xs, np.float64), np.asarray(ys, np.float64)
    write_netcdf4(path, dict(y=ys.size, x=xs.size), {'y': (('y',), ys, {}), 'x': (('x',), xs, {})}, dict(title='stand-in'))


def _era5(tmp_path, bounds=(37, 38, -92, -91)):
    from raider_amd.models import ERA5
    m = ERA5()
    m.set_wmLoc(str(tmp_path))
    m.set_latlon_bounds(list(bounds))
    return m


WHEN = dt.datetime(2020, 1, 30, 13, 52, 45)


def test_prepare_processed_file_exists(tmp_path, caplog):
    from raider_amd.processWM import ExistingWeatherModelTooSmall, prepareWeatherModel
    m = _era5(tmp_path)
    name = tmp_path / 'ERA-5_2020_01_30_T13_52_45_36N_39N_93W_90W.nc'
    _processed_file(name, np.arange(-92.75, -90.2, 0.25), np.arange(36.5, 38.6, 0.25))
    with caplog.at_level(logging.WARNING, logger='RAiDER'):
        assert prepareWeatherModel(m, WHEN, [37, 38, -92, -91]) == str(name)
    assert any('Processed weather model already exists' in r.message for r in caplog.records)
    assert m.bbox == (-92.75, 36.5, -90.25, 38.5) and m.getTime() == WHEN.replace(tzinfo=dt.timezone.utc)
    with pytest.raises(ExistingWeatherModelTooSmall, match='does not cover all of the input points'):
        prepareWeatherModel(m, WHEN, [36, 38, -92, -91])
    assert prepareWeatherModel(m, WHEN, [36, 38, -92, -91], download_only=True) is None


def test_prepare_raw_file_is_processed_and_written(tmp_path, monkeypatch):
    from raider_amd import processWM as P
    m = _era5(tmp_path)
    raw = tmp_path / 'ERA-5_2020_01_30_T13_52_45.nc'
    raw.write_bytes(b'raw')
    calls = []

    class Processed:
        class pointwise:
            grid = (np.arange(36.5, 38.6, 0.25), np.arange(-92.75, -90.2, 0.25), np.arange(3.0))

        def to_netcdf(self, path, time=None, model_name=None):
            calls.append(('write', Path(path).name, time, model_name))
            _processed_file(path, self.pointwise.grid[1], self.pointwise.grid[0])
            return str(path)
    monkeypatch.setattr(P, 'load_raw_model', lambda model, path, bounds: calls.append(('load', Path(path).name, list(bounds))) or Processed())
    out = P.prepareWeatherModel(m, WHEN, [37, 38, -92, -91])
    assert Path(out).name == 'ERA-5_2020_01_30_T13_52_45_36N_39N_93W_90W.nc' and Path(out).exists()
    assert calls == [('load', raw.name, [36.5, 38.5, -92.75, -90.25]), ('write', Path(out).name, WHEN.replace(tzinfo=dt.timezone.utc), 'ERA-5')]
    assert P.prepareWeatherModel(m, WHEN, [37, 38, -92, -91]) == out and len(calls) == 2            # the second time the processed file is found


def test_prepare_raw_file_of_another_provider(tmp_path):
    from raider_amd import processWM as P
    from raider_amd.models import GMAO
    m = GMAO()
    m.set_wmLoc(str(tmp_path))
    (tmp_path / 'GMAO_2020_01_30_T13_52_45.nc').write_bytes(b'raw')
    with pytest.raises(NotImplementedError, match='raw GMAO files are not read here'):
        P.prepareWeatherModel(m, WHEN, [37, 38, -92, -91])


def test_prepare_nothing_on_disk(tmp_path):
    from raider_amd import processWM as P
    m = _era5(tmp_path)
    with pytest.raises(P.WeatherModelFileNotFound) as e:
        P.prepareWeatherModel(m, WHEN, [37, 38, -92, -91])
    assert isinstance(e.value, FileNotFoundError)
    assert e.value.processed == str(tmp_path / 'ERA-5_2020_01_30_T13_52_45_36N_39N_93W_90W.nc') and e.value.raw == str(tmp_path / 'ERA-5_2020_01_30_T13_52_45.nc')
    assert e.value.processed in str(e.value) and e.value.raw in str(e.value)
    with pytest.raises(P.TryToKeepGoingError):                       # outside the model's range: what a failed fetch raises (processWM.py:75-78)
        P.prepareWeatherModel(m, dt.datetime(1949, 1, 1), [37, 38, -92, -91])


def test_float32_level_heights_are_the_references(tmp_path):
    """What the raw route hands the device producer: hybrid-level pressures and heights in the reference's float32 - the bytes of the
    oracle's restatement of calcgeoh + geo_to_ht, which tests/test_ref_files.py pins on the cubes the real RAiDER wrote - and metres
    from the float64 evaluation."""
    from oracle import raider_oracle as O
    from raider_amd.processWM import ecmwf_model_levels_float32
    from raider_amd.weather import ecmwf_l137, read_ecmwf_model_level_file
    tab = ecmwf_l137()
    for name in ('ERA-5_2019_11_17_T20_51_58.nc', 'ERA-5_2022_08_29_T17_00_01.nc'):
        r = read_ecmwf_model_level_file(FILES / name)
        p, h = ecmwf_model_levels_float32(r['z'], r['lnsp'], r['t'], r['q'], r['lats'], tab['a'], tab['b'])
        op, oh = O.ecmwf_model_levels(r['z'], r['lnsp'], r['t'], r['q'], r['lats'], tab['a'], tab['b'])
        assert p.dtype == h.dtype == np.float32 and p.shape == r['t'].shape[1:] + (137,) and np.all(np.diff(h, axis=2) > 0)
        assert p.tobytes() == op.tobytes() and h.tobytes() == oh.tobytes()
        _, h64 = O.ecmwf_model_levels(r['z'], r['lnsp'], r['t'], r['q'], r['lats'], tab['a'], tab['b'], dtype=np.float64)
        assert 0.5 < np.abs(h64 - h).max() < 5.0
    with pytest.raises(ValueError, match='these three numbers should be equal'):
        ecmwf_model_levels_float32(r['z'], r['lnsp'], r['t'], r['q'], r['lats'], a=tab['a'][:-1], b=tab['b'])


# ---- the driver --------------------------------------------------------------------------------------------------------------
class Recorder:
    """Stands in for prepareWeatherModel and the two series entries of raider_amd.cli."""

    def __init__(self, monkeypatch, missing=(), broken=(), no_model=(), series_raises=False):
        from raider_amd import cli
        from raider_amd.delay import SeriesResult
        self.prepared, self.series_calls, self.single_calls = [], [], []

        def prepare(model, tt, bounds, download_only=False, makePlots=False):
            self.prepared.append(tt)
            if tt in missing:
                raise cli.WeatherModelFileNotFound(model.Model(), tt, 'processed.nc', 'raw.nc')
            return None if download_only else f'/wm/{tt:%Y%m%dT%H%M%S}.nc'

        def delays(t):
            n = N_STATIONS
            return np.full(n, t.day / 100.0), np.full(n, 2.0 + t.day / 100.0)

        def series(datetimes, models, aoi, los, **kw):
            self.series_calls.append((list(datetimes), dict(models), kw))
            if series_raises:
                raise RuntimeError('a date failed')
            res = SeriesResult([None if t in no_model else delays(t) for t in datetimes])
            res.routes = [None if t in no_model else 'stacked' for t in datetimes]
            return res

        def single(t, models, aoi, los, **kw):
            self.single_calls.append(t)
            if t in broken:
                raise RuntimeError(f'{t} is broken')
            return delays(t)
        monkeypatch.setattr(cli, 'prepareWeatherModel', prepare)
        monkeypatch.setattr(cli, 'tropo_delay_interp_series', series)
        monkeypatch.setattr(cli, 'tropo_delay_interp', single)


def _station_run(tmp_path, dates, method='none', time='13:52:45'):
    cfg = dict(BASE, date_group=dict(date_list=dates), time_group=dict(time=time, interpolate_time=method), aoi_group=dict(station_file=str(STATIONS)),
               runtime_group=dict(output_directory=str(tmp_path / 'out'), weather_model_directory=str(tmp_path / 'wm')))
    return str(_write_yaml(tmp_path / 'run.yaml', cfg))


N_STATIONS = sum(1 for line in STATIONS.read_text().splitlines()[1:] if line.strip())          # (scenario_6: distinct stations)


def _total(path):
    import pandas as pd
    return pd.read_csv(path, float_precision='round_trip')['totalDelay'].to_numpy()


def test_driver_hands_every_date_to_one_series_call(tmp_path, monkeypatch):
    from raider_amd import cli
    rec = Recorder(monkeypatch)
    paths = cli.calcDelays([_station_run(tmp_path, [20200130, 20200131, 20200201])])
    days = [dt.datetime(2020, 1, 30, 13, 52, 45), dt.datetime(2020, 1, 31, 13, 52, 45), dt.datetime(2020, 2, 1, 13, 52, 45)]
    assert rec.prepared == days and len(rec.series_calls) == 1 and rec.single_calls == []          # prepared at the acquisition time (raider.py:293)
    datetimes, models, kw = rec.series_calls[0]
    assert datetimes == days
    assert models == {d.replace(minute=0, second=0) + dt.timedelta(hours=1): f'/wm/{d:%Y%m%dT%H%M%S}.nc' for d in days}      # keyed by model time
    assert (kw['interpolate_time'], kw['time_step_hours'], kw['model_name'], kw['orbit'], kw['out_proj']) == ('none', 1, 'ERA-5', None, 'EPSG:4326')
    assert [p.name for p in paths] == [f'ERA5_Delay_{d:%Y%m%dT%H%M%S}_ztd.csv' for d in days] and all(p.parent == tmp_path / 'out' for p in paths)
    for p, d in zip(paths, days):
        np.testing.assert_array_equal(_total(p), np.full(N_STATIONS, d.day / 100.0) + np.full(N_STATIONS, 2.0 + d.day / 100.0))
    assert cli.last_run == dict(routes=['stacked'] * 3, fallback=False)


def test_driver_missing_model_raises_after_the_dates_before_it(tmp_path, monkeypatch):
    from raider_amd import cli
    rec = Recorder(monkeypatch, missing=[dt.datetime(2020, 2, 1, 13, 52, 45)])
    with pytest.raises(cli.DatetimeFailed, match='Weather model ERA-5 failed to download for datetime 2020-02-01 13:52:45'):
        cli.calcDelays([_station_run(tmp_path, [20200130, 20200131, 20200201, 20200202])])
    assert len(rec.prepared) == 3 and [len(c[0]) for c in rec.series_calls] == [2]                  # the fourth date is never reached
    for day, has in ((30, True), (31, True)):
        assert 'totalDelay' in (tmp_path / 'out' / f'ERA5_Delay_202001{day}T135245_ztd.csv').read_text()
    assert 'totalDelay' not in (tmp_path / 'out' / 'ERA5_Delay_20200201T135245_ztd.csv').read_text()     # (checkArgs' copy of the station file)


def test_driver_center_time_skips_a_missing_model_time(tmp_path, monkeypatch):
    from raider_amd import cli
    rec = Recorder(monkeypatch, missing=[dt.datetime(2020, 1, 30, 14)])
    paths = cli.calcDelays([_station_run(tmp_path, [20200130, 20200131], method='center_time', time='13:30:00')])
    assert rec.prepared == [dt.datetime(2020, 1, 30, 13), dt.datetime(2020, 1, 30, 14), dt.datetime(2020, 1, 31, 13), dt.datetime(2020, 1, 31, 14)]
    assert sorted(rec.series_calls[0][1]) == [dt.datetime(2020, 1, 30, 13), dt.datetime(2020, 1, 31, 13), dt.datetime(2020, 1, 31, 14)] and len(paths) == 2
    rec = Recorder(monkeypatch, missing=[dt.datetime(2020, 1, 31, 13), dt.datetime(2020, 1, 31, 14)])
    with pytest.raises(cli.NoWeatherModelData, match='Weather model processing failed for all times'):
        cli.calcDelays([_station_run(tmp_path, [20200130, 20200131], method='center_time', time='13:30:00')])
    assert [c[0] for c in rec.series_calls] == [[dt.datetime(2020, 1, 30, 13, 30)]]


def test_driver_skips_a_date_without_a_model_and_a_date_that_fails(tmp_path, monkeypatch, caplog):
    from raider_amd import cli
    d30, d31, d01 = dt.datetime(2020, 1, 30, 13, 52, 45), dt.datetime(2020, 1, 31, 13, 52, 45), dt.datetime(2020, 2, 1, 13, 52, 45)
    Recorder(monkeypatch, no_model=[d31])
    paths = cli.calcDelays([_station_run(tmp_path, [20200130, 20200131, 20200201])])
    assert [p.name for p in paths] == ['ERA5_Delay_20200130T135245_ztd.csv', 'ERA5_Delay_20200201T135245_ztd.csv'] and cli.last_run['routes'] == ['stacked', None, 'stacked']
    # RuntimeError from the series call: the dates go one by one, the broken one is logged and skipped, the values are the same
    rec = Recorder(monkeypatch, series_raises=True, broken=[d31])
    with caplog.at_level(logging.WARNING, logger='RAiDER'):
        again = cli.calcDelays([_station_run(tmp_path, [20200130, 20200131, 20200201])])
    assert rec.single_calls == [d30, d31, d01] and [p.name for p in again] == [p.name for p in paths]
    assert cli.last_run == dict(routes=['per-date', None, 'per-date'], fallback=True)
    assert any('running the 3 dates one by one' in r.getMessage() for r in caplog.records)
    assert [r.getMessage() for r in caplog.records if r.levelno == logging.ERROR] == [f'Datetime {d31} failed']
    np.testing.assert_array_equal(_total(again[1]), np.full(N_STATIONS, 1 / 100.0) + np.full(N_STATIONS, 2.0 + 1 / 100.0))


def test_driver_download_only_and_missing_file(tmp_path, monkeypatch):
    from raider_amd import cli
    rec = Recorder(monkeypatch)
    assert cli.calcDelays([_station_run(tmp_path, [20200130, 20200131]), '--download_only']) == []
    assert len(rec.prepared) == 2 and rec.series_calls == [] and rec.single_calls == []
    with pytest.raises(FileNotFoundError, match='nowhere.yaml'):
        cli.calcDelays([str(tmp_path / 'nowhere.yaml')])
    # a model file that is not to be had fails a download-only run as it fails any other (raider.py:316-318 comes before :333)
    rec = Recorder(monkeypatch, missing=[dt.datetime(2020, 1, 31, 13, 52, 45)])
    with pytest.raises(cli.DatetimeFailed, match='failed to download for datetime 2020-01-31 13:52:45'):
        cli.calcDelays([_station_run(tmp_path, [20200130, 20200131, 20200201]), '--download_only'])
    assert len(rec.prepared) == 2 and rec.series_calls == []
    rec = Recorder(monkeypatch, missing=[dt.datetime(2020, 1, 30, 13), dt.datetime(2020, 1, 30, 14)])
    # (center_time leaves a missing model time out, and a download-only run ends before the files are counted: raider.py:332-338)
    assert cli.calcDelays([_station_run(tmp_path, [20200130], method='center_time', time='13:30:00'), '--download_only']) == []
