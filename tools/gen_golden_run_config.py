#!/usr/bin/env python3
"""Generate tests/golden/g18_run_config.npz by RUNNING THE REFERENCE (imported in place through oracle.refharness.ref_import).

A generator: it runs only where the reference is present; no test calls it.  Re-run with
    python tools/gen_golden_run_config.py

What it holds (data only: inputs and the reference's answers; structured answers as JSON text, floats as float64 arrays):
  dt_*   validators.parse_dates on a dozen date_group spellings (ISO dates, or the exception's class and text)
  tm_*   types.TimeGroup on one spelling per entry of its format table, with and without a time zone and an end time, and on four
         bad ones (time, end_time as ISO times, or class and text)
  bb_*   validators.parse_bbox results and its four messages
  hg_*   validators.get_heights: height_levels as a string and as lists (below zero included), and where `dem` ends up
  fn_*   checkArgs.makeDelayFileNames for Zenith / Conventional / Raytracing / no line of sight x nc / h5 / tif, with and without a date
  md_*   per model (ERA5, ERA5T, ERAI, HRES, GMAO, MERRA2, NCMR): getLLRes(), dtime(), _dataset, Model(); set_latlon_bounds on the nine
         boxes of gen_golden_llreader.py with and without output_spacing; make_weather_model_filename / make_raw_weather_data_filename
         for those bounds
  ca_*   the wetFilenames / hydroFilenames checkArgs makes for a station-file configuration and for bounding-box configurations
         (file_format GTiff, nc, h5, hdf5), relative to the output directory, and the columns and rows of the copied station file

What the harness's stand-ins cannot run, and is therefore NOT in the golden:
  * WeatherModel.checkContainment / checkValidBounds and with them parse_weather_model: the stand-in shapely has boxes without
    `contains` / `intersects` / `buffer`.  tests/test_run_config_host.py pins raider_amd.models.box_containment on cases written out there.
  * get_raster_ext and the checkArgs names of a raster configuration: the stand-in rasterio has no driver table
    (raster_driver_extensions), and RasterRDR cannot open rasters with it.  `GTiff` is pinned on the name the reference's own test reads
    (test/test_intersect.py:56: `..._ztd.tiff`).
  * HRRR / HRRR-AK facts: models/hrrr.py imports geopandas and herbie and reads a shape file on import.  (GMAO and MERRA2 import h5py /
    pydap at the top and use them only to fetch and load: this generator seeds empty modules of those names so that the constructors run.)
  * read_run_config_file itself: RAiDER.cli.raider imports the GUNW and AWS layers.  Its parts are called one by one.
"""
import datetime as dt
import json
import sys
import tempfile
import types
import warnings
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from oracle.refharness import ref_import  # noqa: E402

ref_import.import_reference()
for _name in ('h5py', 'pydap', 'pydap.cas', 'pydap.cas.urs', 'pydap.client'):          # (see the text above: imported, never called here)
    try:
        __import__(_name)
    except ImportError:
        sys.modules[_name] = types.ModuleType(_name)
        if '.' in _name:
            setattr(sys.modules[_name.rsplit('.', 1)[0]], _name.rsplit('.', 1)[1], sys.modules[_name])

import RAiDER.checkArgs as ref_check  # noqa: E402
import RAiDER.cli.types as ref_types  # noqa: E402
import RAiDER.cli.validators as ref_val  # noqa: E402
import RAiDER.llreader as ref_ll  # noqa: E402
import RAiDER.losreader as ref_los  # noqa: E402
import RAiDER.models.weatherModel as ref_wm  # noqa: E402

GOLD = REPO / 'tests' / 'golden'
FILES = GOLD / 'ref_files'
BOXES = [[37, 38, -92, -91], [33.0, 34.0, -118.25, -116.75], [20, 27, -115, -104], [-5.2, -2.3, -41.1, -37.4], [61.5, 64.25, -150.0, -147.5],
         [-72.3, -66.1, 55.0, 63.0], [85.0, 90.0, 10.0, 40.0], [-90.0, -88.5, -30.0, 30.0], [10.0, 12.0, 178.5, 179.9]]      # gen_golden_llreader.py


def outcome(fn):
    """('ok', value) or ('raise', [class name, text])."""
    try:
        return ['ok', fn()]
    except Exception as exc:
        return ['raise', [type(exc).__name__, str(exc)]]


def date_cases(out):
    cases = [dict(date_list='20200103, 20200104'), dict(date_list=20200130), dict(date_list=[20200101, '2020-01-05', 20200110]),
             dict(date_list='2020-01-03'), dict(date_start=20200130), dict(date_start='2020-01-30', date_end='2020-02-02'),
             dict(date_start=20200101, date_end=20200110, date_step=3), dict(date_start='20200101', date_end='20200110', date_step='4'),
             dict(date_start=15), dict(date_start=245), dict(), dict(date_start='yesterday'), dict(date_start=20200110, date_end=20200101),
             dict(date_start=20200228, date_end=20200301)]
    got = [outcome(lambda c=c: [d.isoformat() for d in ref_val.parse_dates(ref_types.DateGroupUnparsed(**c)).date_list]) for c in cases]
    out['dt_cases'], out['dt_results'] = np.array(json.dumps(cases)), np.array(json.dumps(got))
    print(f'  parse_dates: {len(cases)} cases, {sum(g[0] == "raise" for g in got)} raise')


def time_cases(out):
    cases = [dict(time='T13:52:45.5'), dict(time='T135245.25'), dict(time='135245.75'), dict(time='T13:52:45'), dict(time='13:52:45'),
             dict(time='T135245'), dict(time='135245'), dict(time='T13:52'), dict(time='T1352'), dict(time='13:52'), dict(time='T13'), dict(time=''),
             dict(time='T13:52:45Z'), dict(time='13:52:45+0100'), dict(time='T1352Z'), dict(time='T13-0800'), dict(time=135245),
             dict(time='13:52:45', end_time='13:53:30'), dict(time='13:52:45', end_time='T135245', interpolate_time='center_time'),
             dict(time='23:59:29'),
             # the bad ones
             dict(), dict(time='noon'), dict(time='23:59:45'), dict(time='13:52:45', end_time='13:52:44'), dict(time='25:00:00')]

    def run(c):
        g = ref_types.TimeGroup(**c)
        return [g.time.isoformat(), g.end_time.isoformat(), g.interpolate_time]
    got = [outcome(lambda c=c: run(c)) for c in cases]
    out['tm_cases'], out['tm_results'] = np.array(json.dumps(cases)), np.array(json.dumps(got))
    print(f'  TimeGroup: {len(cases)} cases, {sum(g[0] == "raise" for g in got)} raise')


def bbox_cases(out):
    cases = ['37 38 -92 -91', ' 33.5  34   -118.25 -116.75 ', [20, 27, -115, -104], [-5.2, -2.3, -41.1, -37.4], (-90, 90, -180, 180),
             '37 38 -92', [38, 37, -92, -91], [37, 38, -91, -91], [-91, 38, -92, -91], [37, 91, -92, -91], [37, 38, -181, -91], [37, 38, 170, 190],
             '37 38 -92 -91 5']
    got = [outcome(lambda c=c: [float(v) for v in ref_val.parse_bbox(c)]) for c in cases]
    out['bb_cases'], out['bb_results'] = np.array(json.dumps(cases)), np.array(json.dumps(got))
    print(f'  parse_bbox: {len(cases)} cases, {sum(g[0] == "raise" for g in got)} raise')


def height_cases(out):
    station = str(FILES / 'scenario_6_stations.csv')
    cases = [dict(height=dict(height_levels='0 100 200 500'), aoi=dict(bounding_box='37 38 -92 -91')),
             dict(height=dict(height_levels='[-100, 0, 1500]'), aoi=dict(bounding_box='37 38 -92 -91')),
             dict(height=dict(height_levels=[0, 50.5, 1000]), aoi=dict(bounding_box='37 38 -92 -91')),
             dict(height=dict(height_levels=[-10, 0]), aoi=dict(bounding_box='37 38 -92 -91')),
             dict(height=dict(), aoi=dict(bounding_box='37 38 -92 -91')),
             dict(height=dict(height_file_rdr='hgt.rdr'), aoi=dict(lat_file='lat.rdr', lon_file='lon.rdr')),
             dict(height=dict(dem='not_there.dem'), aoi=dict(lat_file='lat.rdr', lon_file='lon.rdr')),
             dict(height=dict(dem='user.dem'), aoi=dict(station_file='ref_files/scenario_6_stations.csv')),
             dict(height=dict(), aoi=dict(station_file='ref_files/scenario_6_stations.csv'))]

    def run(c):
        aoi = dict(c['aoi'])
        if 'station_file' in aoi:
            aoi['station_file'] = station
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            g = ref_val.get_heights(ref_types.HeightGroupUnparsed(**c['height']), ref_types.AOIGroupUnparsed(**aoi),
                                    ref_types.RuntimeGroup(output_directory='out_dir'))
        return dict(dem=None if g.dem is None else Path(g.dem).as_posix(), use_dem_latlon=g.use_dem_latlon, height_file_rdr=g.height_file_rdr,
                    height_levels=None if g.height_levels is None else [float(v) for v in g.height_levels])
    got = [outcome(lambda c=c: run(c)) for c in cases]
    out['hg_cases'], out['hg_results'] = np.array(json.dumps(cases)), np.array(json.dumps(got))
    print(f'  get_heights: {len(cases)} cases')


def file_name_cases(out):
    conv = ref_los.Conventional.__new__(ref_los.Conventional)          # (makeDelayFileNames only asks isinstance(los, Zenith))
    ray = ref_los.Raytracing.__new__(ref_los.Raytracing)
    kinds = dict(Zenith=ref_los.Zenith(), Conventional=conv, Raytracing=ray, none=None)
    when = dt.datetime(2020, 1, 30, 13, 52, 45)
    cases, got = [], []
    for los in kinds:
        for ext in ('nc', 'h5', 'tif'):
            for date in (when, None):
                cases.append(dict(los=los, ext=ext, date=None if date is None else date.isoformat(), model='ERA5', out='some_dir'))
                got.append([Path(p).as_posix() for p in ref_check.makeDelayFileNames(date, kinds[los], ext, 'ERA5', Path('some_dir'))])
    out['fn_cases'], out['fn_results'] = np.array(json.dumps(cases)), np.array(json.dumps(got))
    print(f'  makeDelayFileNames: {len(cases)} cases')


def model_cases(out):
    names = ['ERA5', 'ERA5T', 'ERAI', 'HRES', 'GMAO', 'MERRA2', 'NCMR']
    when = dt.datetime(2020, 1, 30, 13, 52, 45)
    facts, done = {}, []
    for name in names:
        try:
            _, Model = ref_val.get_wm_by_name(name)
            m = Model()
        except Exception as exc:
            print(f'  model {name}: not available here ({type(exc).__name__}: {exc})')
            continue
        done.append(name)
        facts[name] = dict(Model=m.Model(), dataset=m._dataset, dtime=m.dtime(), level_type=m._model_level_type,
                           valid_from=m._valid_range[0].isoformat())
        out[f'md_llres_{name}'] = np.float64(m.getLLRes())
        bounds, fnames = [], []
        for spacing in (None, 0.05):
            for b in BOXES:
                m.set_latlon_bounds(list(b), output_spacing=spacing)
                got = np.array(m.get_latlon_bounds(), dtype=np.float64)
                bounds.append(got)
                fnames.append(ref_wm.make_weather_model_filename(m.Model(), when, got))
        out[f'md_bounds_{name}'] = np.array(bounds)
        facts[name]['filenames'] = fnames
        facts[name]['raw_filename'] = Path(ref_wm.make_raw_weather_data_filename('wm_dir', m.Model(), when)).as_posix()
    out['md_models'], out['md_facts'] = np.array(done), np.array(json.dumps(facts))
    out['md_boxes'], out['md_spacings'], out['md_when'] = np.array(BOXES, dtype=float), np.array([np.nan, 0.05]), np.array(when.isoformat())
    unknown = outcome(lambda: ref_val.get_wm_by_name('WRFX'))
    out['md_unknown'] = np.array(json.dumps(unknown))
    print(f'  models: {done}; unknown -> {unknown[1][0]}')


def check_args_cases(out):
    import RAiDER.models.era5 as ref_era5
    cases = [dict(kind='station', dates=dict(date_start=20200130), time='13:52:45', runtime=dict()),
             dict(kind='station', dates=dict(date_list=[20200130, 20200131]), time='T00:00:00', runtime=dict()),
             dict(kind='bbox', dates=dict(date_start=20200130), time='13:52:45', runtime=dict()),
             dict(kind='bbox', dates=dict(date_start=20200101, date_end=20200103), time='T23:00:00', runtime=dict(file_format='nc')),
             dict(kind='bbox', dates=dict(date_start=20200130), time='13:52:45', runtime=dict(file_format='h5')),
             dict(kind='bbox', dates=dict(date_start=20200130), time='13:52:45', runtime=dict(file_format='.hdf5'))]
    got = []
    for c in cases:
        with tempfile.TemporaryDirectory() as tmp:
            outdir = Path(tmp) / 'output'
            aoi = (ref_ll.StationFile(FILES / 'scenario_6_stations.csv') if c['kind'] == 'station' else ref_ll.BoundingBox([37, 38, -92, -91]))
            rt = ref_types.RuntimeGroup(output_directory=str(outdir), **c['runtime'])
            cfg = ref_types.RunConfig(weather_model=ref_era5.ERA5(), date_group=ref_val.parse_dates(ref_types.DateGroupUnparsed(**c['dates'])),
                                      time_group=ref_types.TimeGroup(time=c['time']), aoi_group=ref_types.AOIGroup(aoi=aoi),
                                      height_group=ref_types.HeightGroup(None, False, None, None),
                                      los_group=ref_types.LOSGroup(los=ref_los.Zenith()), runtime_group=rt)
            cfg = ref_check.checkArgs(cfg)
            rel = lambda p: '' if p == '' else Path(p).relative_to(outdir).as_posix()
            rec = dict(wet=[rel(p) for p in cfg.wetFilenames], hydro=[rel(p) for p in cfg.hydroFilenames],
                       dates=[d.isoformat() for d in cfg.date_group.date_list], wm_dir=Path(rt.weather_model_directory).relative_to(outdir).as_posix(),
                       wmLoc_is_wm_dir=cfg.weather_model.get_wmLoc() == str(rt.weather_model_directory))
            if c['kind'] == 'station':
                rec['csv'] = Path(cfg.wetFilenames[0]).read_text()
            got.append(rec)
    out['ca_cases'], out['ca_results'] = np.array(json.dumps(cases)), np.array(json.dumps(got))
    print(f'  checkArgs: {len(cases)} configurations')


def main():
    warnings.filterwarnings('ignore')
    out = {}
    date_cases(out)
    time_cases(out)
    bbox_cases(out)
    height_cases(out)
    file_name_cases(out)
    model_cases(out)
    check_args_cases(out)
    out['_meta'] = np.array(json.dumps(dict(ref_import.provenance(), numpy=np.__version__,
                                            # (the suite's provenance check of g*.npz asks for the family's generator by name)
                                            generator='tools/gen_golden_run_config.py, companion of oracle/refharness/gen_golden.py')))
    path = GOLD / 'g18_run_config.npz'
    np.savez_compressed(path, **out)
    print(f'g18_run_config: {path.stat().st_size / 1024:.1f} KiB  keys={len(out)}')


if __name__ == '__main__':
    main()
