"""Host side of output grids in a projected CRS: which CRSs take the device routes (delay.grid_projection) and the series route."""
import numpy as np

from raider_amd import _lib as L
from raider_amd.delay import GridAOI, PointsAOI, grid_projection, series_route, stacked_route
from raider_amd.losreader import Conventional, Raytracing, Zenith

HRRR = '+proj=lcc +lat_1=38.5 +lat_2=38.5 +lat_0=38.5 +lon_0=262.5 +x_0=0 +y_0=0 +a=6371229 +b=6371229 +units=m +no_defs'
HRRR_AK = '+proj=stere +lat_0=90 +lon_0=225 +lat_ts=60 +a=6371229 +b=6371229'


def test_grid_projection_of_utm_zones():
    k, p = grid_projection(32611)
    assert k == L.RDR_GRID_TM
    assert np.array_equal(p, [6378137.0, 0.0066943799901413165, 0.0, -117.0, 0.9996, 500000.0, 0.0])
    k, p = grid_projection('EPSG:32735')                       # southern zone 35: false northing 10 000 000
    assert k == L.RDR_GRID_TM and p[3] == 27.0 and p[6] == 10000000.0
    k, p = grid_projection('+proj=utm +zone=33 +south +ellps=WGS84')
    assert k == L.RDR_GRID_TM and p[3] == 15.0 and p[6] == 10000000.0


def test_grid_projection_of_the_conic_model_crss():
    k, p = grid_projection(HRRR)
    assert k == L.RDR_PROJ_LCC
    assert np.array_equal(p, [6371229.0, 0.0, 38.5, 38.5, 38.5, 262.5, 0.0, 0.0])
    k, p = grid_projection(HRRR_AK)
    assert k == L.RDR_PROJ_STERE
    assert p.size == 8 and p[2] == 90.0 and p[3] == 60.0 and p[4] == 1.0 and p[5] == 225.0


def test_grid_projection_refuses_the_rest():
    assert grid_projection(4326) is None
    assert grid_projection('EPSG:4326') is None
    assert grid_projection(4978) is None
    assert grid_projection(3857) is None                      # web Mercator: pyproj only
    assert grid_projection('+proj=stere +lat_0=45 +lon_0=10') is None      # the oblique aspect is not built in
    assert grid_projection('+proj=merc +lon_0=0') is None


def test_series_routes_on_projected_grids():
    """A ray-traced series on a UTM / conic grid is stacked (stacked_route, what tropo_delay_series follows); series_route keeps its
    lon/lat-only answer."""
    xp, yp = np.linspace(3.0e5, 5.2e5, 12), np.linspace(3.8e6, 3.64e6, 9)
    los = Raytracing(inc=36.0, heading=-167.9)
    assert stacked_route(GridAOI(xp, yp), los, 32611) == 'cube'
    assert stacked_route(GridAOI(xp, yp), los, HRRR) == 'cube'
    assert stacked_route(GridAOI(xp, yp), los, HRRR_AK) == 'cube'
    assert stacked_route(GridAOI(xp, yp), los, 4326) == 'cube' == series_route(GridAOI(xp, yp), los, 4326)
    pts = PointsAOI(np.array([33.0]), np.array([-117.0]), np.array([0.0]), xp, yp)
    assert stacked_route(pts, los, 32611) == 'points'
    assert series_route(GridAOI(xp, yp), los, 32611) is None
    assert stacked_route(GridAOI(xp, yp), los, 3857) is None
    assert stacked_route(GridAOI(xp, yp), Zenith(), 32611) is None
    assert stacked_route(GridAOI(xp, yp), Conventional(inc=36.0, heading=0.0), 32611) is None
