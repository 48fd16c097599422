#!/usr/bin/env python3
"""Generate tests/golden/g15_pressure_levels.npz, tests/golden/ref_files/ERA-5_2018_03_27_T13_00_00.nc and
raider_amd/data/ecmwf_pl_heights.txt by RUNNING THE REFERENCE (imported in place through oracle.refharness.ref_import).

A generator: it runs only where the reference is present; no test calls it.  Re-run with
    python tools/gen_golden_pressure_levels.py
Needs oracle/_ref (oracle/build_ref.sh) for the reference's native `interpolate` extension.

(a) the reference's `test/scenario_7` raw ERA-5 pressure-level file (copied verbatim: data) through its own ERA5 class in
    pressure-level mode: `load_weather` (ECMWF._load_pressure_level, models/ecmwf.py:252-303), then the processing chain of
    WeatherModel.load (models/weatherModel.py:251-260).  When no real xarray is importable, the harness's stand-in gets a Dataset
    read from the file with scipy, so that the reference's loader opens it by path.  The packed int16 fields are decoded as the CF
    convention has it for float64 scale_factor / add_offset: in float64; the float32 coordinate variables are widened to float64, so
    that the reference's formulas run in float64 throughout and the fixture pins the formulas, not one float32 realisation of their
    round-off (DESIGN.md 6.5 has the same choice for the model-level front end).
(b) WeatherModel._get_heights / utilFcns.geo_to_ht on small synthetic states for the three kinds of height field (geopotential,
    geopotential height, geometric height) with latitudes per row and per node.  Arrays are stored in the loaded layout
    (ny, nx, nlev), surface first, rows and columns ascending; the test makes the file layouts from them.
"""
import json
import shutil
import sys
import warnings
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))

from oracle.refharness import ref_import  # noqa: E402

ref_import.import_reference()

import xarray as xr  # noqa: E402  (the harness's stand-in unless a real one is installed)
from RAiDER.models.era5 import ERA5  # noqa: E402
from RAiDER.models.model_levels import LEVELS_25_HEIGHTS  # noqa: E402
from RAiDER.models.weatherModel import WeatherModel  # noqa: E402

GOLD = REPO / 'tests' / 'golden'
RAW = ref_import.REF_ROOT / 'test' / 'scenario_7' / 'ERA-5_2018_03_27_T13_00_00.nc'


def dataset_from_netcdf3(path):
    from scipy.io import netcdf_file
    data, coords = {}, {}
    with netcdf_file(str(path), 'r', mmap=False) as f:
        for name, v in f.variables.items():
            raw = np.array(v.data)
            if name in f.dimensions:
                coords[name] = raw.astype(np.float64) if raw.dtype.kind == 'f' else raw.astype(raw.dtype.newbyteorder('='))
                continue
            out = raw.astype(np.float64)
            out *= np.float64(getattr(v, 'scale_factor', 1.0))
            out += np.float64(getattr(v, 'add_offset', 0.0))
            fill = getattr(v, '_FillValue', None)
            if fill is not None:
                out[raw == fill] = np.nan
            data[name] = (v.dimensions, out)
    return xr.Dataset(data_vars=data, coords=coords)


def from_file(out):
    dst = GOLD / 'ref_files' / RAW.name
    dst.parent.mkdir(parents=True, exist_ok=True)
    shutil.copyfile(RAW, dst)
    if hasattr(xr, 'register_dataset'):
        xr.register_dataset(str(dst), dataset_from_netcdf3(dst))
    m = ERA5()
    m.setLevelType('pl')
    m.load_weather(f=str(dst))
    out['a_zlevels'] = np.asarray(m._zlevels, dtype=np.float64)
    # every step is per column: the fixture keeps every third row and column of the full run, and the last of each (the file size limit)
    ny, nx = m._zs.shape[:2]
    rows, cols = np.unique(np.r_[0:ny:3, ny - 1]), np.unique(np.r_[0:nx:3, nx - 1])
    out['a_rows'], out['a_cols'] = rows, cols
    blk = lambda v: np.ascontiguousarray(np.asarray(v)[np.ix_(rows, cols)])
    for k in ('_zs', '_p', '_t', '_q', '_xs', '_ys'):
        out['a' + k] = blk(getattr(m, k))
    print('  state:', {k: (out['a' + k].dtype, out['a' + k].shape) for k in ('_zs', '_p', '_t', '_q', '_xs', '_ys')})
    m._find_e()
    m._uniform_in_z()
    m._checkForNans()
    m._get_wet_refractivity()
    m._get_hydro_refractivity()
    m._adjust_grid(m.get_latlon_bounds())
    m._getZTD()
    out['a_out_zs'] = np.asarray(m._zs, dtype=np.float64)
    out['a_out_xs'], out['a_out_ys'] = np.asarray(m._xs), np.asarray(m._ys)
    out['a_t_out'], out['a_p_out'], out['a_e_out'] = blk(m._t), blk(m._p), blk(m._e)
    out['a_wet'], out['a_hydro'] = blk(m._wet_refractivity), blk(m._hydrostatic_refractivity)
    out['a_wet_total'], out['a_hydro_total'] = blk(m._wet_ztd), blk(m._hydrostatic_ztd)
    print('  cubes:', m._wet_refractivity.dtype, m._wet_refractivity.shape, 'zs', out['a_out_zs'][[0, 1, -1]], 'NaNs', int(np.isnan(m._wet_refractivity).sum()))


def synthetic(out):
    class Model(WeatherModel):
        def _fetch(self, *a):
            pass

        def load_weather(self, *a, **k):
            pass

    rng = np.random.default_rng(15)
    nlev, ny, nx = 5, 3, 70
    lat1 = np.array([-61.25, 12.5, 78.75])
    lon1 = -120.0 + 0.25 * np.arange(nx)
    lat2 = lat1[:, None] + 0.013 * np.arange(nx)[None, :] + rng.uniform(-0.01, 0.01, (ny, nx))          # a projected grid's latitudes
    gh = np.sort(rng.uniform(-300.0, 79000.0, (ny, nx, nlev)), axis=2)                                  # geopotential height, m
    m = Model()
    out['b_h0'] = gh * 9.80665 * (1 + 1e-3 * rng.uniform(-1, 1, gh.shape))                              # geopotential, m2 s-2
    out['b_h1'] = gh
    out['b_h2'] = gh + rng.uniform(0, 50.0, gh.shape)                                                   # geometric height, m
    out['b_lat1'], out['b_lat2'] = lat1, lat2
    out['b_p1'] = np.array([100000.0, 85000.0, 50000.0, 10000.0, 100.0])
    out['b_p3'] = out['b_p1'] * (1 + 0.01 * rng.uniform(-1, 1, gh.shape))
    out['b_t'] = 288.0 - 0.0065 * np.minimum(gh, 11000.0) + rng.normal(0, 1.0, gh.shape)
    out['b_q'] = 0.012 * np.exp(-gh / 2400.0) * (1 + 0.1 * rng.uniform(-1, 1, gh.shape))
    _, lat1_full = np.meshgrid(lon1, lat1)                                                              # ecmwf.py:287
    for tag, lats in (('lat1', lat1_full), ('lat2', lat2)):
        m._get_heights(lats, out['b_h0'] / m._g0)                                                       # ecmwf.py:284-290
        out[f'b_zs0_{tag}'] = m._zs.copy()
        m._get_heights(lats, out['b_h1'])                                                               # hrrr.py:312
        out[f'b_zs1_{tag}'] = m._zs.copy()
    print('  synthetic:', out['b_zs0_lat1'].dtype, out['b_zs0_lat1'].shape, 'top', float(out['b_zs1_lat2'].max()))


def main():
    warnings.filterwarnings('ignore')
    out = {}
    from_file(out)
    synthetic(out)
    out['level_heights'] = np.array(LEVELS_25_HEIGHTS, dtype=np.float64)
    with open(REPO / 'raider_amd' / 'data' / 'ecmwf_pl_heights.txt', 'w') as f:                         # repr: the float64 round-trips
        f.write('# heights in m that ECMWF pressure-level states are resampled to, descending\n')
        f.writelines(repr(float(v)) + '\n' for v in out['level_heights'])
    out['_meta'] = np.array(json.dumps(dict(ref_import.provenance(), numpy=np.__version__, xarray=getattr(xr, '__version__', 'harness stand-in'),
                                            # (the suite's provenance check of g*.npz asks for the family's generator by name)
                                            generator='tools/gen_golden_pressure_levels.py, companion of oracle/refharness/gen_golden.py')))
    path = GOLD / 'g15_pressure_levels.npz'
    np.savez_compressed(path, **out)
    print(f'g15_pressure_levels: {path.stat().st_size / 1024:.1f} KiB  keys={list(out)}')


if __name__ == '__main__':
    main()
