#!/usr/bin/env python3
"""Generate tests/golden/g17_llreader.npz by RUNNING THE REFERENCE (imported in place through oracle.refharness.ref_import).

A generator: it runs only where the reference is present; no test calls it.  Re-run with
    python tools/gen_golden_llreader.py

What it holds (data only: inputs and the reference's answers):
  cb_*   utilFcns.clip_bbox on boxes and spacings, negative and positive, on and off multiples of the spacing
  ab_*   BoundingBox(box, cube_spacing_in_m).add_buffer(ll_res) -> bounds(), for mid and high latitudes (|lat| > 60), a box that
         reaches +-90 and one that crosses +-180, with and without a requested cube spacing
  br_*   AOI.calc_buffer_ray for asc / desc x right over incidence angles and integration heights ('left' fails the reference's
         own assertion: recorded as the exception's name)
  sp_*   set_output_spacing / get_output_spacing for EPSG:4326 and a metric CRS (EPSG:4978)
  xy_*   set_output_xygrid(4326) after add_buffer: the two axes, one pair of keys per case
  st_*   bounds_from_csv and StationFile.readLL / readZ on the two station files under tests/golden/ref_files
  fb_*   utilFcns.get_file_and_band on plain names, `file;band` strings and a string with two semicolons

What the harness's stand-in rasterio cannot do is not recorded: opening rasters, statistics, rowcol.  Those parts of llreader are pinned
by formulas written out in tests/test_llreader_host.py and tests/test_gpu_llreader.py.
"""
import json
import sys
import warnings
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from oracle.refharness import ref_import  # noqa: E402

ref_import.import_reference()
import RAiDER.llreader as ref_ll  # noqa: E402
import RAiDER.utilFcns as ref_util  # noqa: E402

GOLD = REPO / 'tests' / 'golden'
FILES = GOLD / 'ref_files'


def clip_cases(out):
    boxes = [[36.925, 38.075, -92.075, -90.925], [-5.3, -2.1, -41.0, -37.5], [0.0, 0.0, 0.0, 0.0], [61.37, 72.01, -159.99, -152.5],
             [-90.0, -77.7, 170.2, 180.3], [15.7637, 21.4936, -101.6384, -98.2418]]
    spacings = [0.02, 0.05, 0.1, 0.25, 0.03, 1.0]
    rows, sp, res = [], [], []
    for b in boxes:
        for s in spacings:
            rows.append(b); sp.append(s); res.append([float(v) for v in ref_util.clip_bbox(b, s)])
    out['cb_box'], out['cb_spacing'], out['cb_result'] = np.array(rows), np.array(sp), np.array(res)
    print(f'  clip_bbox: {len(rows)} cases')


BOXES = [[37, 38, -92, -91], [33.0, 34.0, -118.25, -116.75], [20, 27, -115, -104], [-5.2, -2.3, -41.1, -37.4], [61.5, 64.25, -150.0, -147.5],
         [-72.3, -66.1, 55.0, 63.0], [85.0, 90.0, 10.0, 40.0], [-90.0, -88.5, -30.0, 30.0], [10.0, 12.0, 178.5, 179.9]]


def buffer_cases(out):
    box, res, cube, got = [], [], [], []
    for b in BOXES:
        for ll_res in (0.03, 0.1, 0.25, 0.3125):
            for cs in (None, 2000.0, 5000.0):
                aoi = ref_ll.BoundingBox(list(b), cube_spacing_in_m=cs)
                aoi.add_buffer(ll_res)
                box.append(b); res.append(ll_res); cube.append(np.nan if cs is None else cs); got.append([float(v) for v in aoi.bounds()])
    out['ab_box'], out['ab_ll_res'], out['ab_cube_spacing_m'], out['ab_bounds'] = np.array(box, dtype=float), np.array(res), np.array(cube), np.array(got)
    print(f'  add_buffer: {len(box)} cases')


def ray_buffer_cases(out):
    box, direction, look, inc, maxz, got = [], [], [], [], [], []
    for b in BOXES:
        for d in ('asc', 'desc', 'ASC'):
            for ia, mz in ((30, 80), (20.5, 40.0), (45, 80)):
                aoi = ref_ll.BoundingBox(list(b))
                box.append(b); direction.append(d); look.append('right'); inc.append(ia); maxz.append(mz)
                got.append([float(v) for v in aoi.calc_buffer_ray(d, lookDir='right', incAngle=ia, maxZ=mz)])
    out['br_box'], out['br_direction'], out['br_look'] = np.array(box, dtype=float), np.array(direction), np.array(look)
    out['br_inc'], out['br_maxz'], out['br_bounds'] = np.array(inc, dtype=float), np.array(maxz, dtype=float), np.array(got)
    verdict = []
    for look_dir in ('left', 'light', 'Right'):
        try:
            ref_ll.BoundingBox([37, 38, -92, -91]).calc_buffer_ray('asc', lookDir=look_dir)
            verdict.append('ok')
        except Exception as exc:
            verdict.append(type(exc).__name__)
    out['br_look_cases'], out['br_look_verdict'] = np.array(['left', 'light', 'Right']), np.array(verdict)
    print(f'  calc_buffer_ray: {len(box)} cases; look directions {dict(zip(out["br_look_cases"], verdict))}')


def spacing_cases(out):
    ll, cube, deg, metric = [], [], [], []
    for ll_res in (0.05, 0.1, 0.25):
        for cs in (None, 2000.0, 30.0):
            aoi = ref_ll.BoundingBox([20, 27, -115, -104], cube_spacing_in_m=cs)
            aoi.set_output_spacing(ll_res=ll_res)
            ll.append(ll_res); cube.append(np.nan if cs is None else cs)
            deg.append(float(aoi.get_output_spacing(4326))); metric.append(float(aoi.get_output_spacing(4978)))
    out['sp_ll_res'], out['sp_cube_spacing_m'], out['sp_deg'], out['sp_metric'] = np.array(ll), np.array(cube), np.array(deg), np.array(metric)


def xygrid_cases(out):
    cases = [(BOXES[0], 0.03, None), (BOXES[1], 0.25, 2000.0), (BOXES[3], 0.1, None), (BOXES[4], 0.3125, 5000.0), (BOXES[6], 0.25, None)]
    out['xy_box'] = np.array([c[0] for c in cases], dtype=float)
    out['xy_ll_res'] = np.array([c[1] for c in cases])
    out['xy_cube_spacing_m'] = np.array([np.nan if c[2] is None else c[2] for c in cases])
    for i, (b, ll_res, cs) in enumerate(cases):
        aoi = ref_ll.BoundingBox(list(b), cube_spacing_in_m=cs)
        aoi.add_buffer(ll_res)
        aoi.set_output_xygrid(4326)
        out[f'xy_xpts_{i}'], out[f'xy_ypts_{i}'] = np.asarray(aoi.xpts, dtype=float), np.asarray(aoi.ypts, dtype=float)
    print(f'  set_output_xygrid: {len(cases)} cases')


def station_cases(out):
    names = ['scenario_2/stations.csv', 'scenario_6_stations.csv']
    out['st_file'] = np.array(names)
    for i, name in enumerate(names):
        path = FILES / name
        out[f'st_bounds_{i}'] = np.array(ref_ll.bounds_from_csv(path), dtype=float)
        aoi = ref_ll.StationFile(path)
        lats, lons = aoi.readLL()
        out[f'st_lats_{i}'], out[f'st_lons_{i}'], out[f'st_hgts_{i}'] = np.asarray(lats, dtype=float), np.asarray(lons, dtype=float), np.asarray(aoi.readZ(), dtype=float)
        out[f'st_aoi_bounds_{i}'] = np.array(aoi.bounds(), dtype=float)
    print(f'  station files: {names}')


def file_band_cases(out):
    strings = ['lat.rdr', ' geom/lat.rdr ', 'los.rdr;2', ' geom/los.rdr ; 1 ', '/data/a b/los.rdr;12', 'a;b;c', 'los.rdr;x']
    path, band = [], []
    for s in strings:
        try:
            p, b = ref_util.get_file_and_band(s)
            path.append(str(p)); band.append(b)
        except Exception as exc:
            path.append(type(exc).__name__); band.append(-1)
    out['fb_string'], out['fb_path'], out['fb_band'] = np.array(strings), np.array(path), np.array(band)
    print('  get_file_and_band:', list(zip(strings, path, band)))


def main():
    warnings.filterwarnings('ignore')
    out = {}
    clip_cases(out)
    buffer_cases(out)
    ray_buffer_cases(out)
    spacing_cases(out)
    xygrid_cases(out)
    station_cases(out)
    file_band_cases(out)
    out['_meta'] = np.array(json.dumps(dict(ref_import.provenance(), numpy=np.__version__,
                                            # (the suite's provenance check of g*.npz asks for the family's generator by name)
                                            generator='tools/gen_golden_llreader.py, companion of oracle/refharness/gen_golden.py')))
    path = GOLD / 'g17_llreader.npz'
    np.savez_compressed(path, **out)
    print(f'g17_llreader: {path.stat().st_size / 1024:.1f} KiB  keys={len(out)}')


if __name__ == '__main__':
    main()
