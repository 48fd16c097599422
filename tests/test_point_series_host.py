"""CPU: the host routing of a date series at query points (tropo_delay_point_series) without a device - which call a line of sight /
AOI / output CRS takes, which dates stack - and the routing of tropo_delay_series that must not move."""
import datetime as dt
from types import SimpleNamespace

import numpy as np
import pytest

LCC = '+proj=lcc +lat_1=38.5 +lat_2=38.5 +lat_0=38.5 +lon_0=262.5 +x_0=0 +y_0=0 +a=6371229 +b=6371229 +units=m +no_defs'
OBLIQUE = '+proj=omerc +lat_0=4 +lonc=115 +alpha=53 +k=0.99984 +x_0=0 +y_0=0 +ellps=GRS80 +units=m'   # nothing the device transforms


def _aois():
    from raider_amd.delay import GridAOI, PointsAOI
    return GridAOI(np.linspace(0.0, 1.0, 3), np.linspace(1.0, 0.0, 3)), PointsAOI(np.array([0.5]), np.array([0.5]), np.array([0.0]))


def test_route_per_line_of_sight_aoi_and_crs():
    from raider_amd.delay import point_series_route
    from raider_amd.losreader import Conventional, Raytracing, Zenith
    grid, pts = _aois()
    ray = Raytracing(inc=35.0, heading=-167.9)
    conv = Conventional(inc=np.array([35.0]), heading=np.array([0.0]))
    for los in (Zenith(), conv, ray):
        for crs in (4326, 32611, LCC):
            assert point_series_route(grid, los, crs) is None          # cube AOIs belong to tropo_delay_series
    for crs in (4326, 32611, LCC, OBLIQUE):                            # (whether the device takes the CRS is decided per date: the model's own CRS counts)
        assert point_series_route(pts, Zenith(), crs) == 'delays'
        assert point_series_route(pts, conv, crs) == 'delays'
    for crs in (4326, 32611, LCC):
        assert point_series_route(pts, ray, crs) == 'rays'
    assert point_series_route(pts, ray, OBLIQUE) is None
    # a foreign projected LOS (no _divisor_source): its own __call__ per date; a foreign ray-traced one without a batch constructor too
    foreign = SimpleNamespace(is_Zenith=lambda: False, is_Projected=lambda: True)
    assert point_series_route(pts, foreign, 4326) is None
    foreign_ray = SimpleNamespace(is_Zenith=lambda: False, is_Projected=lambda: False)
    assert point_series_route(pts, foreign_ray, 4326) is None


def _cube(shape=(4, 5, 6), dtype=np.float32, z0=0.0, proj=None):
    ny, nx, nz = shape
    return SimpleNamespace(shape=shape, dtype=dtype, grid=(np.linspace(30, 34, ny), np.linspace(-120, -115, nx), z0 + np.arange(nz) * 100.0),
                           projection=proj)


def _plan(cube=None, zpts=(0.0, 500.0, 2000.0), zref=15000.0, gridkey=None, divkind=None):
    return dict(cube=cube or _cube(), zpts=np.array(zpts), zref=zref, gridkey=gridkey, divkind=divkind)


def test_which_dates_stack():
    from raider_amd.delay import stacking_dates
    assert stacking_dates({}) == [] and stacking_dates({0: _plan()}) == [] and stacking_dates({0: None, 1: _plan()}) == []
    assert stacking_dates({0: _plan(), 1: _plan(), 2: _plan()}) == [0, 1, 2]
    # a date the one-call route refuses (None), one on another z axis, dtype, projection, height list, top or intermediate grid: per date
    assert stacking_dates({0: _plan(), 1: None, 2: _plan()}) == [0, 2]
    assert stacking_dates({0: _plan(), 1: _plan(_cube(z0=1.0)), 2: _plan()}) == [0, 2]
    assert stacking_dates({0: _plan(), 1: _plan(_cube(dtype=np.float64)), 2: _plan(), 3: _plan(_cube(proj=dict(proj='lcc', lat_1=38.5)))}) == [0, 2]
    assert stacking_dates({0: _plan(), 1: _plan(zpts=(0.0, 500.0)), 2: _plan(zref=14000.0), 3: _plan(gridkey=(3, b'x')), 4: _plan()}) == [0, 4]
    # the FIRST planned date sets the grid: two later dates that agree with each other but not with it stay per date
    assert stacking_dates({0: _plan(), 1: _plan(_cube(z0=1.0)), 2: _plan(_cube(z0=1.0))}) == []
    assert stacking_dates({0: None, 1: _plan(_cube(z0=1.0)), 2: _plan(_cube(z0=1.0)), 3: _plan()}) == [1, 2]
    # an incidence array on one date and a divisor on another do not share a projection mode
    assert stacking_dates({0: _plan(divkind='inc'), 1: _plan(divkind='div'), 2: _plan(divkind='inc')}) == [0, 2]
    # the plan of a date the loop broke at (an exception: missing from the dict) takes no part
    assert stacking_dates({0: _plan(), 1: _plan()}) == [0, 1]


def test_shared_or_per_date_divisor():
    from raider_amd.delay import _series_divisor
    inc = np.array([30.0, 35.0, 40.0])
    assert _series_divisor([dict(div=None), dict(div=None)], (3,)) == {}
    kw = _series_divisor([dict(div=('inc', inc)), dict(div=('inc', inc.copy()))], (3,))
    assert list(kw) == ['inc'] and kw['inc'] is inc
    kw = _series_divisor([dict(div=('inc', 35.0)), dict(div=('inc', 35.0))], (3,))
    assert kw == {'inc': 35.0}
    a, b = np.array([0.8, 0.7, 0.6]), np.array([0.8, 0.7, 0.61])
    kw = _series_divisor([dict(div=('div', a)), dict(div=('div', b))], (3,))
    assert list(kw) == ['divisor'] and kw['divisor'].shape == (2, 3) and np.array_equal(kw['divisor'], np.stack([a, b]))


def test_series_argument_checks_come_before_any_device_work():
    from raider_amd.delay import tropo_delay_point_series
    from raider_amd.losreader import Zenith
    grid, pts = _aois()
    with pytest.raises(ValueError, match='2 dates but 1 weather model files'):
        tropo_delay_point_series([dt.datetime(2020, 1, 1), dt.datetime(2020, 1, 13)], ['only_one.nc'], pts, Zenith())
    with pytest.raises(ValueError, match='points AOI'):
        tropo_delay_point_series([dt.datetime(2020, 1, 1)], ['only_one.nc'], grid, Zenith())


def test_per_date_divisor_axis_is_checked_on_the_host():
    from raider_amd.engine import _series_proj_args
    assert _series_proj_args(3, 4, (4,), None, None) == (0, None, 0, 0.0)
    assert _series_proj_args(3, 4, (4,), 35.0, None) == (2, None, 0, 35.0)
    mode, arr, stride, _ = _series_proj_args(3, 4, (4,), np.full(4, 35.0), None)
    assert (mode, arr.shape, stride) == (1, (4,), 0)
    mode, arr, stride, _ = _series_proj_args(3, 4, (4,), None, np.full((3, 4), 0.8))
    assert (mode, arr.shape, stride) == (3, (12,), 4)
    with pytest.raises(ValueError, match='leading axis of 2'):
        _series_proj_args(3, 4, (4,), None, np.full((2, 4), 0.8))
    with pytest.raises(ValueError, match='not both'):
        _series_proj_args(3, 4, (4,), 35.0, np.full(4, 0.8))


def test_the_cube_series_routes_have_not_moved():
    """tropo_delay_series keeps sending zenith and projected lines of sight date by date: the point series is a NEW name."""
    from raider_amd.delay import series_route, stacked_route
    from raider_amd.losreader import Conventional, Raytracing, Zenith
    grid, pts = _aois()
    ray = Raytracing(inc=35.0, heading=-167.9)
    for los in (Zenith(), Conventional(inc=np.array([35.0]), heading=np.array([0.0]))):
        for aoi in (grid, pts):
            for crs in (4326, 32611, LCC):
                assert series_route(aoi, los, crs) is None and stacked_route(aoi, los, crs) is None
    assert series_route(grid, ray, 4326) == 'cube' and series_route(pts, ray, 4326) == 'points' and series_route(grid, ray, 32611) is None
    assert stacked_route(grid, ray, 32611) == 'cube' and stacked_route(pts, ray, LCC) == 'points' and stacked_route(pts, ray, OBLIQUE) is None
