"""GPU: the pressure-level front end of the cube producer (rdr_pressure_level_state, raider_amd.weather) against golden g15, made by
running the reference: ECMWF._load_pressure_level (models/ecmwf.py:252-303) and the chain of WeatherModel.load on its own
test/scenario_7 raw ERA-5 pressure-level file, and WeatherModel._get_heights / utilFcns.geo_to_ht on small synthetic states.

g15 holds the reference's float64 evaluation (the generator decodes the packed fields in float64 and widens the float32 coordinate
variables), and every third row and column of the file's 24 x 67 columns plus the last ones (`a_rows`, `a_cols`): the whole state
would pass the size limit for a committed file; every step is per column."""
import datetime as dt
import itertools
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

RAW = Path(__file__).resolve().parent / 'golden' / 'ref_files' / 'ERA-5_2018_03_27_T13_00_00.nc'
# Heights of kinds 0 and 1: the only inexact step is the device cos / sin of latitude inside geo_to_ht, a few ulp of a quantity whose
# float64 ulp at 80 km is 1.5e-11 m; 1e-9 m is a tenth of the project's ray-parity bound.
H_ATOL = 1e-9
E_RTOL = 2.5e-7          # tests/test_gpu_producer.py: e passes through exp(), <= 1 ulp of f32 after the cast; wet is built on it (2 x)
HRRR = dict(proj='lcc', lat_1=38.5, lat_2=38.5, lat_0=38.5, lon_0=262.5, x_0=0.0, y_0=0.0, a=6371229.0, b=6371229.0)


def _file_layout(v, top_first, rows_desc, cols_desc):
    """(ny, nx, nlev) surface first, ascending -> (nlev, ny, nx) as a file with these orders holds it"""
    f = v.transpose(2, 0, 1)
    if top_first: f = f[::-1]
    if rows_desc: f = f[:, ::-1]
    if cols_desc: f = f[:, :, ::-1]
    return np.ascontiguousarray(f)


def _state_case(g, kind, p3, lat2, top_first, rows_desc, cols_desc):
    lay = lambda v: _file_layout(v, top_first, rows_desc, cols_desc)
    p = lay(g['b_p3']) if p3 else (g['b_p1'][::-1].copy() if top_first else g['b_p1'])
    if lat2:
        lats = g['b_lat2'][::-1] if rows_desc else g['b_lat2']
        lats = np.ascontiguousarray(lats[:, ::-1] if cols_desc else lats)
    else:
        lats = g['b_lat1'][::-1].copy() if rows_desc else g['b_lat1']
    want_zs = g['b_h2'] if kind == 2 else g[f'b_zs{kind}_lat{2 if lat2 else 1}']
    want_p = g['b_p3'] if p3 else np.broadcast_to(g['b_p1'], g['b_t'].shape)
    return (lay(g[f'b_h{kind}']), p, lay(g['b_t']), lay(g['b_q']), lats), (want_zs, want_p, g['b_t'], g['b_q'])


@pytest.mark.parametrize('kind', [0, 1, 2])
def test_state_matches_reference_for_every_order(golden, kind):
    """nlev = 5, ny = 3, nx = 70 (one full wave plus a tail, crossing the 32-wide transpose tile twice): every combination of level,
    row and column order, 1-D and 3-D pressure, 1-D and 2-D latitudes."""
    from raider_amd.weather import pressure_level_state
    g = golden('g15_pressure_levels')
    assert g['b_t'].shape == (3, 70, 5)
    worst = 0.0
    for p3, lat2, top_first, rows_desc, cols_desc in itertools.product((False, True), repeat=5):
        args, (want_zs, want_p, want_t, want_q) = _state_case(g, kind, p3, lat2, top_first, rows_desc, cols_desc)
        zs, p, t, q = pressure_level_state(*args, height_kind=kind, top_first=top_first, rows_descending=rows_desc, cols_descending=cols_desc)
        case = (kind, p3, lat2, top_first, rows_desc, cols_desc)
        assert zs.shape == (3, 70, 5) and zs.dtype == np.float64 and p.dtype == t.dtype == q.dtype == np.float64
        assert np.array_equal(p, want_p) and np.array_equal(t, want_t) and np.array_equal(q, want_q), case          # only moved
        if kind == 2:
            assert np.array_equal(zs, want_zs), case
        else:
            worst = max(worst, float(np.abs(zs - want_zs).max()))
            np.testing.assert_allclose(zs, want_zs, rtol=0, atol=H_ATOL, err_msg=str(case))
    print(f'height_kind {kind}: worst |zs - reference| = {worst:.3e} m')


def test_state_from_device_tensors(golden):
    """torch tensors on the GPU in -> tensors out, the same values as the host path"""
    import torch
    from raider_amd.weather import pressure_level_state
    g = golden('g15_pressure_levels')
    args, want = _state_case(g, 1, True, True, True, True, False)
    host = pressure_level_state(*args, height_kind=1, rows_descending=True)
    dev = pressure_level_state(*(torch.from_numpy(a).cuda() for a in args), height_kind=1, rows_descending=True)
    for a, b, w in zip(host, dev, want):
        assert b.is_cuda and np.array_equal(a, b.cpu().numpy())
        np.testing.assert_allclose(a, w, rtol=0, atol=H_ATOL)


@pytest.fixture(scope='module')
def era5_model():
    from raider_amd.weather import load_ecmwf_pressure_levels
    return load_ecmwf_pressure_levels(RAW, return_state=True)


def test_raw_file_to_cubes_matches_reference(golden, era5_model):
    """The reference's ERA5 class in pressure-level mode on its own raw file: the loaded state, then t, p and hydro bit-exact, e and
    wet within 1 ulp of f32, ZTDs at the tolerances tests/test_gpu_producer.py holds the producer to against g10."""
    g = golden('g15_pressure_levels')
    m = era5_model
    sub = np.ix_(g['a_rows'], g['a_cols'])
    zs, p, t, q = (v[sub] for v in m.levels)
    assert m.levels[0].shape == (24, 67, 37)
    assert np.array_equal(p, g['a_p']) and np.array_equal(t, g['a_t']) and np.array_equal(q, g['a_q'])
    print(f'raw file: worst |zs - reference| = {np.abs(zs - g["a_zs"]).max():.3e} m')
    np.testing.assert_allclose(zs, g['a_zs'], rtol=0, atol=H_ATOL)
    assert np.all(np.diff(m.levels[0], axis=2) > 0)
    ys, xs, _ = m.pointwise.grid
    assert np.array_equal(xs, g['a_out_xs']) and np.array_equal(ys, g['a_out_ys']) and np.array_equal(m.zs, g['a_out_zs'])
    assert m.proj == 4326 and m.pointwise.dtype == np.float32 and m.total.dtype == np.float64
    assert np.array_equal(m.t[sub], g['a_t_out'])
    assert np.array_equal(m.p[sub], g['a_p_out'])
    np.testing.assert_allclose(m.e[sub], g['a_e_out'], rtol=E_RTOL, atol=0)
    wet, hyd = (v[sub] for v in m.pointwise.read())
    assert np.array_equal(hyd, g['a_hydro'])
    np.testing.assert_allclose(wet, g['a_wet'], rtol=2 * E_RTOL, atol=0)
    wt, ht = (v[sub] for v in m.total.read())
    np.testing.assert_allclose(ht, g['a_hydro_total'], rtol=1e-13, atol=1e-18)
    np.testing.assert_allclose(wt, g['a_wet_total'], rtol=2 * E_RTOL, atol=1e-18)
    for got, want in ((m.t[sub], g['a_t_out']), (m.p[sub], g['a_p_out']), (m.e[sub], g['a_e_out']), (wet, g['a_wet']), (hyd, g['a_hydro']),
                      (wt, g['a_wet_total']), (ht, g['a_hydro_total'])):
        assert np.array_equal(np.isnan(got), np.isnan(want))


def test_both_front_ends_share_geo_to_ht_bit_for_bit():
    """ecmwf_levels_kernel with t = 0 integrates no thickness: the geopotential of every level is the surface geopotential, so its
    heights are geo_to_ht(lat, z_surf / g0) - what pressure_levels_kernel makes of the same geopotential (kind 0) and latitude."""
    from raider_amd.weather import ecmwf_model_levels, pressure_level_state
    rng = np.random.default_rng(3)
    nlev, ny, nx = 4, 3, 37
    z_surf = rng.uniform(-500.0, 60000.0, (ny, nx)).astype(np.float32) * np.float32(9.80665)
    lnsp = np.log(rng.uniform(60000.0, 103000.0, (ny, nx))).astype(np.float32)
    lats = np.array([-88.5, 0.25, 47.125], np.float32)
    a, b = np.array([0.0, 2000.0, 5000.0, 3000.0, 0.0]), np.array([0.0, 0.0, 0.3, 0.7, 1.0])
    zero = np.zeros((nlev, ny, nx), np.float32)
    _, zs_ml = ecmwf_model_levels(z_surf, lnsp, zero, zero, lats, a, b)
    geop = np.broadcast_to(z_surf.astype(np.float64), (nlev, ny, nx))
    zs_pl, _, _, _ = pressure_level_state(geop, np.arange(1.0, nlev + 1), zero, zero, lats.astype(np.float64), height_kind=0)
    assert np.isfinite(zs_ml).all() and np.ptp(zs_ml) > 50000.0
    assert np.array_equal(zs_ml, zs_pl)


@pytest.mark.parametrize('los_kind', ['zenith', 'rays'])
def test_era5_model_traces_like_its_own_file(tmp_path, era5_model, los_kind):
    from raider_amd.delay import GridAOI, tropo_delay
    from raider_amd.losreader import Raytracing, Zenith
    when = dt.datetime(2018, 3, 27, 13)
    path = tmp_path / 'ERA-5_pl.nc'
    era5_model.to_netcdf(path, time=when)
    if los_kind == 'zenith':
        aoi, los = GridAOI(np.linspace(-101.9, -96.1, 7), np.linspace(19.4, 17.6, 5)), Zenith()
    else:
        aoi, los = GridAOI(np.linspace(-101.9, -96.1, 16), np.linspace(19.4, 17.6, 16)), Raytracing(inc=39.0, heading=-167.9)
    a, _ = tropo_delay(when, era5_model, aoi, los, [0.0, 500.0, 3000.0], 4326, None)
    b, _ = tropo_delay(when, str(path), aoi, los, [0.0, 500.0, 3000.0], 4326, None)
    for name in ('wet', 'hydro'):
        got = np.asarray(a[name][:])
        assert np.isfinite(got).all() and got.mean() > 0
        assert np.array_equal(got, np.asarray(b[name][:]))
    assert 1.5 < np.asarray(a['hydro'][:])[0].mean() < 3.5            # a sane hydrostatic delay in metres


def test_hrrr_style_state_through_the_chain(golden):
    """Geopotential height (kind 1), 2-D latitudes, Lambert conformal axes, HRRR's level table: the g15 (b) state through
    cubes_from_pressure_levels; the cube traces where the grid is and is NaN outside, exactly as the cube that
    cubes_from_model_levels makes of the reference's own (zs, p, t, q)."""
    from raider_amd.delay import GridAOI, tropo_delay
    from raider_amd.losreader import Zenith
    from raider_amd.weather import cubes_from_model_levels, cubes_from_pressure_levels
    g = golden('g15_pressure_levels')
    new_z = np.flipud(np.load(Path(__file__).resolve().parent.parent / 'raider_amd' / 'data' / 'hrrr_l50.npz')['level_heights'])
    ny, nx, _ = g['b_t'].shape
    xs, ys = 3000.0 * (np.arange(nx) - nx // 2), 3000.0 * (np.arange(ny) - ny // 2)      # around the projection centre (38.5 N, 97.5 W)
    args, (want_zs, want_p, want_t, want_q) = _state_case(g, 1, True, True, True, False, False)
    m = cubes_from_pressure_levels(xs, ys, *args, height_kind=1, humidity_type='q', new_z=new_z, proj=HRRR, return_state=True)
    assert m.proj == HRRR and np.array_equal(m.zs, new_z)
    np.testing.assert_allclose(m.levels[0], want_zs, rtol=0, atol=H_ATOL)
    assert all(np.array_equal(a, b) for a, b in zip(m.levels[1:], (want_p, want_t, want_q)))
    ref = cubes_from_model_levels(xs, ys, want_zs, want_p, want_t, want_q, 'q', new_z=new_z)
    ref.proj = HRRR
    # 9 longitudes within 44 km of the centre and one 217 km east of it; 3 latitudes within 1.3 km of the middle row, one 11 km north
    aoi = GridAOI(np.r_[np.linspace(-98.0, -97.0, 9), -95.0], np.array([38.6, 38.51, 38.5, 38.49]))
    when = dt.datetime(2020, 1, 1, 12)
    a, _ = tropo_delay(when, m, aoi, Zenith(), [0.0, 500.0, 3000.0], 4326, None)
    b, _ = tropo_delay(when, ref, aoi, Zenith(), [0.0, 500.0, 3000.0], 4326, None)
    inside = np.zeros((3, 4, 10), bool); inside[:, 1:, :9] = True
    for name in ('wet', 'hydro'):
        got = np.asarray(a[name][:])
        assert got.shape == inside.shape and np.isfinite(got[inside]).all() and np.isnan(got[~inside]).all()
        assert np.array_equal(got, np.asarray(b[name][:]), equal_nan=True)
