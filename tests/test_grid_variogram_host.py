"""Host side of the per-grid-cell variograms (raider_amd/variogram.py: station_grid, GridVariograms; no GPU).

station_grid is the arithmetic of RaiderStats._get_extent (cli/statsPlot.py:1291-1368); tests/golden/g21_grid_variogram.npz
(tools/gen_golden_grid_variogram.py) holds what the reference's own _get_extent returned for spacings 0.5, 1 and 2 with bbox = None.
The harness's shapely stand-in cannot do Polygon.intersects, so the reference's bbox branch could not be recorded: it is pinned here by
a restatement of :1299-1325 (floor / ceil of the box, the two exceptions and their messages)."""
import warnings
from pathlib import Path

import numpy as np
import pytest

from raider_amd import variogram as V

GOLDEN = Path(__file__).resolve().parent / 'golden' / 'g21_grid_variogram.npz'


@pytest.fixture(scope='module')
def g21():
    return np.load(GOLDEN)


@pytest.mark.parametrize('tag, spacing', [('05', 0.5), ('1', 1), ('2', 2)])
def test_grid_is_the_reference_s_bit_for_bit(g21, tag, spacing):
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        sg = V.station_grid(g21['lon'], g21['lat'], spacing=spacing)
    want_spacing = float(g21[f'ext{tag}_spacing'])
    assert sg.spacing == want_spacing
    assert (len(w) == 1 and 'reset to 1' in str(w[0].message)) == (want_spacing != spacing)      # 2 does not divide 3 degrees: reset, as the reference did
    assert np.array(sg.extent, dtype=np.float64).tobytes() == g21[f'ext{tag}_extent'].tobytes()
    assert list(sg.grid_dim) == g21[f'ext{tag}_grid_dim'].tolist()
    assert sg.gridpoints.dtype == np.float64 and sg.gridpoints.tobytes() == g21[f'ext{tag}_gridpoints'].tobytes()
    assert sg.start[0] == 0 and sg.start[-1] == sg.order.size == g21['lon'].size and sg.start.size == sg.gridpoints.shape[0] + 1


def test_stations_fall_into_the_reference_s_cells(g21):
    sg = V.station_grid(g21['lon'], g21['lat'])
    assert np.array_equal(sg.cell, g21['gridnode'])
    assert np.diff(sg.start).tolist() == [0, 9, 10, 12, 30, 45]
    assert np.array_equal(sg.cell[sg.order], np.repeat(np.arange(6), np.diff(sg.start)))
    for c in range(6):                                        # stable: the stations of a cell keep their input order
        assert np.all(np.diff(sg.order[sg.start[c]:sg.start[c + 1]]) > 0)


def test_cells_of_a_hand_made_set():
    #            W edge   interior  E border  N border  NE corner  interior edge (west / south inclusive)   outside the box
    lon = np.array([10.0, 10.3, 13.0, 11.5, 13.0, 11.0, 12.7, 14.2, 9.9])
    lat = np.array([50.0, 51.9, 50.5, 52.0, 52.0, 51.0, 50.2, 50.5, 51.0])
    sg = V.station_grid(lon, lat, bbox=[50.0, 52.0, 10.0, 13.0])
    assert sg.extent == [10.0, 13.0, 50.0, 52.0] and sg.grid_dim == [3, 2]
    ix = np.array([0, 0, 2, 1, 2, 1, 2]); iy = np.array([0, 1, 0, 1, 1, 1, 0])
    assert sg.cell[:7].tolist() == (ix * 2 + (1 - iy)).tolist()
    assert sg.cell[7:].tolist() == [-1, -1]
    assert sorted(sg.order.tolist()) == list(range(7)) and sg.start[-1] == 7
    # the centres: cell g = ix * ny + (ny - 1 - iy) at (W + (ix + 1/2) s, S + (iy + 1/2) s)
    for g, (cx, cy) in enumerate(sg.gridpoints):
        i, j = g // 2, 1 - g % 2
        assert (cx, cy) == (10.0 + i + 0.5, 50.0 + j + 0.5)
    half = V.station_grid(lon, lat, spacing=0.5, bbox=[50.0, 52.0, 10.0, 13.0])
    assert half.grid_dim == [6, 4] and half.cell[2] == 5 * 4 + (3 - 1) and half.cell[4] == 5 * 4 + 0 and half.cell[0] == 3


def test_bbox_branch_restated():
    """:1299-1325: a box that overlaps the data replaces the extent by its own floor / ceil; one that does not, or that exceeds the
    globe, raises with the reference's messages; the clamps of :1329-1336 act on data beyond +-180 / +-90"""
    lon = np.array([10.2, 12.8]); lat = np.array([50.1, 51.7])
    assert V.station_grid(lon, lat, bbox=[49.3, 52.2, 9.5, 12.1]).extent == [9.0, 13.0, 49.0, 53.0]
    assert V.station_grid(lon, lat, bbox=[52.0, 53.0, 13.0, 14.0]).extent == [13.0, 14.0, 52.0, 53.0]       # touching rectangles intersect
    with pytest.raises(ValueError, match='User-specified bounds do not overlap with dataset bounds, adjust bounds and re-run program.'):
        V.station_grid(lon, lat, bbox=[60.0, 61.0, 10.0, 12.0])
    with pytest.raises(ValueError, match='Specified bounds exceed -180/180 lon and/or -90/90 lat, adjust bounds and re-run program.'):
        V.station_grid(lon, lat, bbox=[50.0, 52.0, -181.5, 12.0])
    with pytest.raises(ValueError, match='Specified bounds exceed'):
        V.station_grid(lon, lat, bbox=[50.0, 90.5, 10.0, 12.0])
    far = V.station_grid(np.array([178.5, 180.4]), np.array([-90.2, -88.5]))
    assert far.extent == [178.0, 180.0, -90.0, -88.0] and far.grid_dim == [2, 2]
    assert far.cell.tolist() == [-1, -1] and far.order.size == 0                    # both lie outside the clamped extent (lat -90.2; lon 180.4)
    ok = V.station_grid(np.array([178.5, 180.4, 179.5]), np.array([-89.5, -88.5, -90.2]))
    assert ok.cell.tolist() == [0 * 2 + (1 - 0), -1, -1]


def test_spacing_that_does_not_divide_is_reset():
    lon = np.array([10.2, 12.8]); lat = np.array([50.1, 51.7])                     # 3 x 2 degrees
    with pytest.warns(UserWarning, match='reset to 1'):
        sg = V.station_grid(lon, lat, spacing=2)
    assert sg.spacing == 1 and sg.grid_dim == [3, 2]
    with pytest.warns(UserWarning, match='reset to 1'):
        assert V.station_grid(lon, lat, spacing=0.4).spacing == 1
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert V.station_grid(lon, lat, spacing=0.25).grid_dim == [12, 8]


def test_map_layout():
    """maps are a[g].reshape(nx, ny).T (:3302-3337): [ny, nx], row 0 in the north, column 0 in the west"""
    sg = V.station_grid(np.array([10.2, 12.8]), np.array([50.1, 51.7]))
    gv = V.GridVariograms(grid=sg)
    m_lon = gv.map(sg.gridpoints[:, 0]); m_lat = gv.map(sg.gridpoints[:, 1])
    assert m_lon.shape == (2, 3)
    assert np.array_equal(m_lon, [[10.5, 11.5, 12.5]] * 2) and np.array_equal(m_lat, [[51.5] * 3, [50.5] * 3])


def device_linspace(hmax, nbins):
    """the rule of csrc/cell_variogram_kernels.h, one rounded operation per line"""
    s = np.float64(hmax) * np.float64(0.67)
    step = s / np.float64(nbins)
    e = np.arange(nbins + 1, dtype=np.float64) * step
    e[nbins] = s
    return e


@pytest.mark.parametrize('nbins', [1, 19, 64])
def test_device_linspace_rule_is_numpy_s(nbins):
    rng = np.random.default_rng(nbins)
    hm = np.concatenate([10.0 ** rng.uniform(-3, 7, 900), rng.uniform(1.0, 2.0e5, 100)])
    assert hm.size == 1000
    for h in hm:
        assert device_linspace(h, nbins).tobytes() == np.linspace(0, h * 0.67, nbins + 1).tobytes()


def test_grid_variograms_refuses_before_the_device():
    lon = np.array([10.2, 12.8]); lat = np.array([50.1, 51.7]); v = np.ones((2, 2))
    with pytest.raises(ValueError, match='nbins must be 1 .. 64'):
        V.grid_variograms(lon, lat, v, nbins=65)
    with pytest.raises(ValueError, match='must agree in N'):
        V.grid_variograms(lon, lat, np.ones((2, 3)))
    with pytest.raises(TypeError, match='all NumPy arrays or all GPU tensors'):
        import torch
        V.grid_variograms(torch.from_numpy(lon), lat, v)
    with pytest.raises(ValueError, match='stations inside the grid'):
        V.grid_variograms(lon, lat, v, bbox=[50.0, 51.0, 10.0, 11.0])
