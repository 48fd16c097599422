"""Host side of the pressure-level front end (raider_amd.weather): the reader of raw ERA-5 / HRES pressure-level files
(models/ecmwf.py:252-279 of the reference), the shipped height table (models/ecmwf.py:38-40) and the argument checks that run
before anything touches the device.  No GPU."""
from pathlib import Path

import numpy as np
import pytest

RAW = Path(__file__).resolve().parent / 'golden' / 'ref_files' / 'ERA-5_2018_03_27_T13_00_00.nc'      # the reference's test/scenario_7 file, whole (467 KiB)


def test_reader_returns_the_file_in_its_own_order_with_flags(golden):
    from raider_amd.weather import read_ecmwf_pressure_level_file
    r = read_ecmwf_pressure_level_file(RAW)
    assert r['z'].shape == r['t'].shape == r['q'].shape == (37, 24, 67) and r['z'].dtype == np.float64
    assert r['lats'].shape == (24,) and r['lons'].shape == (67,)
    assert r['level'][0] == 100.0 and r['level'][-1] == 100000.0 and r['level'].size == 37          # hPa x 100, top first
    assert r['top_first'] is True and r['rows_descending'] is True and r['cols_descending'] is False
    assert r['lats'][0] == 21.5 and r['lats'][-1] == 15.75 and np.array_equal(r['ys'], r['lats'][::-1])
    assert r['lons'][0] == -107.25 and r['lons'][-1] == -90.75 and np.array_equal(r['xs'], r['lons'])
    assert not np.isnan(r['z']).any() and 180.0 < r['t'].min() < r['t'].max() < 320.0 and 0.0 < r['q'].max() < 0.03
    # the state the reference holds after loading this file (g15 keeps a subset of its columns): the same numbers, re-ordered
    g = golden('g15_pressure_levels')
    sub = np.ix_(g['a_rows'], g['a_cols'])
    loaded = lambda v: v[::-1, ::-1].transpose(1, 2, 0)[sub]              # levels and rows flipped, (lev, y, x) -> (y, x, lev)
    assert np.array_equal(loaded(r['t']), g['a_t']) and np.array_equal(loaded(r['q']), g['a_q'])
    assert np.array_equal(np.broadcast_to(r['level'][::-1], g['a_p'].shape), g['a_p'])
    assert np.array_equal(np.meshgrid(r['xs'], r['ys'])[0][sub], g['a_xs']) and np.array_equal(np.meshgrid(r['xs'], r['ys'])[1][sub], g['a_ys'])


def test_reader_crops_to_ll_bounds():
    from raider_amd.weather import read_ecmwf_pressure_level_file
    full = read_ecmwf_pressure_level_file(RAW)
    r = read_ecmwf_pressure_level_file(RAW, ll_bounds=(17.0, 19.5, -100.0, -95.25))
    assert np.array_equal(r['ys'], np.arange(17.0, 19.75, 0.25)) and np.array_equal(r['xs'], np.arange(-100.0, -95.0, 0.25))
    my, mx = np.isin(full['lats'], r['lats']), np.isin(full['lons'], r['lons'])
    for k in ('z', 't', 'q'):
        assert r[k].flags.c_contiguous and np.array_equal(r[k], full[k][:, my][:, :, mx])
    assert r['rows_descending'] is True and r['top_first'] is True
    with pytest.raises(RuntimeError, match='no data in z'):
        read_ecmwf_pressure_level_file(RAW, ll_bounds=(40.0, 41.0, -100.0, -95.0))


def test_reader_wraps_longitudes_and_reports_other_orders(tmp_path):
    """A file written the other way round: levels surface first, latitudes ascending, longitudes descending and above 180."""
    from scipy.io import netcdf_file
    from raider_amd.weather import read_ecmwf_pressure_level_file
    lev, lat, lon = np.array([1000, 500, 10], np.int32), np.array([10.0, 10.25], np.float32), np.array([181.0, 180.75, 180.5, 180.25], np.float32)
    rng = np.random.default_rng(0)
    path = tmp_path / 'pl.nc'
    packed = {}
    with netcdf_file(str(path), 'w') as f:
        for name, vals, typ in (('longitude', lon, 'f4'), ('latitude', lat, 'f4'), ('level', lev, 'i4'), ('time', np.array([0], np.int32), 'i4')):
            f.createDimension(name, vals.size)
            f.createVariable(name, typ, (name,))[:] = vals
        for name, scale, off in (('z', 7.25, 235790.5), ('t', 0.0017, 246.5), ('q', 2.8e-7, 0.0093)):
            v = f.createVariable(name, 'i2', ('time', 'level', 'latitude', 'longitude'))
            packed[name] = rng.integers(-32000, 32000, (1, 3, 2, 4)).astype(np.int16)
            v[:] = packed[name]
            v.scale_factor = np.float64(scale); v.add_offset = np.float64(off)
    r = read_ecmwf_pressure_level_file(path)
    assert np.array_equal(r['lons'], [-179.0, -179.25, -179.5, -179.75]) and np.array_equal(r['xs'], r['lons'][::-1])
    assert r['top_first'] is False and r['rows_descending'] is False and r['cols_descending'] is True
    assert np.array_equal(r['level'], [100000.0, 50000.0, 1000.0])
    assert np.array_equal(r['t'], packed['t'][0].astype(np.float64) * 0.0017 + 246.5)


def test_height_table_is_the_reference_table(golden):
    from raider_amd.weather import ecmwf_pressure_level_heights
    g = golden('g15_pressure_levels')
    tab = ecmwf_pressure_level_heights()
    assert tab.dtype == np.float64 and np.array_equal(tab, g['level_heights'])
    assert np.array_equal(np.flipud(tab), g['a_zlevels'])                  # what the reference resampled the fixture file to
    assert np.all(np.diff(tab) < 0)


def test_arguments_are_checked_before_any_device_call(monkeypatch):
    from raider_amd import weather as W

    def no_device(*a, **k):
        raise AssertionError('the device was reached')
    monkeypatch.setattr(W.Context, 'default', classmethod(no_device))
    nlev, ny, nx = 5, 3, 7
    f = np.ones((nlev, ny, nx)); p = np.ones(nlev); lats = np.zeros(ny)
    for kind in (3, -1, 'geopotential', None):
        with pytest.raises(ValueError, match='height_kind'):
            W.pressure_level_state(f, p, f, f, lats, height_kind=kind)
    with pytest.raises(ValueError, match='temperature and humidity'):
        W.pressure_level_state(f, p, f[:-1], f, lats)
    with pytest.raises(ValueError, match='temperature and humidity'):
        W.pressure_level_state(f, p, f, f.transpose(1, 2, 0), lats)
    with pytest.raises(ValueError, match='height field'):
        W.pressure_level_state(f[0], p, f[0], f[0], lats)
    with pytest.raises(ValueError, match='pressure'):
        W.pressure_level_state(f, np.ones(nlev + 1), f, f, lats)
    with pytest.raises(ValueError, match='pressure'):
        W.pressure_level_state(f, np.ones((ny, nx, nlev)), f, f, lats)
    for bad in (np.zeros((nx, ny)), np.zeros((ny, nx + 1)), np.zeros(ny + 1), np.zeros((ny, nx, 1))):
        with pytest.raises(ValueError, match='latitudes'):
            W.pressure_level_state(f, p, f, f, bad, height_kind=1)
    with pytest.raises(ValueError, match=r'\(nlev, 3, 8\)'):
        W.cubes_from_pressure_levels(np.arange(8.0), np.arange(3.0), f, p, f, f, lats)
    with pytest.raises(RuntimeError, match='Not a valid humidity type'):
        W.cubes_from_pressure_levels(np.arange(7.0), np.arange(3.0), f, p, f, f, lats, humidity_type='dewpoint')
    with pytest.raises(ValueError, match='height_kind'):
        W.cubes_from_pressure_levels(np.arange(7.0), np.arange(3.0), f, p, f, f, lats, height_kind=7)
