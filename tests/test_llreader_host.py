"""raider_amd.llreader and what it takes from utilFcns / rawraster, on the host: the AOI arithmetic against what the reference itself
returned (golden g17, tools/gen_golden_llreader.py), the reference tests' constructor errors and hard-coded values
(test/test_llreader.py), and the geotransform reader.  Nothing here needs a GPU."""
from pathlib import Path

import numpy as np
import pytest

from raider_amd import llreader, rawraster
from raider_amd.llreader import BoundingBox, GeocodedFile, RasterRDR, StationFile, bounds_from_csv
from raider_amd.utilFcns import clip_bbox, get_file_and_band, rio_extents, rio_profile, transform_bbox

FILES = Path(__file__).parent / 'golden' / 'ref_files'
S4 = FILES / 'scenario_4'
STATIONS_2 = FILES / 'scenario_2' / 'stations.csv'


def _cube_spacing(v):
    return None if np.isnan(v) else float(v)


def test_clip_bbox_equals_the_reference(golden):
    g = golden('g17_llreader')
    for box, spacing, want in zip(g['cb_box'], g['cb_spacing'], g['cb_result']):
        assert [float(v) for v in clip_bbox(list(box), float(spacing))] == list(want), (box, spacing)


def test_add_buffer_equals_the_reference(golden):
    g = golden('g17_llreader')
    assert np.abs(g['ab_box'][:, :2]).max() == 90.0 and (np.abs(g['ab_box'][:, :2]) > 60).any()          # the cases the fixture must hold
    for box, ll_res, cs, want in zip(g['ab_box'], g['ab_ll_res'], g['ab_cube_spacing_m'], g['ab_bounds']):
        aoi = BoundingBox(list(box), cube_spacing_in_m=_cube_spacing(cs))
        aoi.add_buffer(float(ll_res))
        assert [float(v) for v in aoi.bounds()] == list(want), (box, ll_res, cs)
    # the reference's docstring example (llreader.py:104-111)
    aoi = BoundingBox([37, 38, -92, -91]); aoi.add_buffer(0.03)
    assert aoi.bounds() == [36.93, 38.07, -92.07, -90.93]


def test_calc_buffer_ray_equals_the_reference(golden):
    g = golden('g17_llreader')
    assert {'asc', 'desc'} <= set(g['br_direction'])
    for box, d, look, inc, maxz, want in zip(g['br_box'], g['br_direction'], g['br_look'], g['br_inc'], g['br_maxz'], g['br_bounds']):
        got = BoundingBox(list(box)).calc_buffer_ray(str(d), lookDir=str(look), incAngle=float(inc), maxZ=float(maxz))
        assert [float(v) for v in got] == list(want), (box, d, inc, maxz)
    # 'left' fails the reference's own assertion ('right light'), and the same way here
    for look, verdict in zip(g['br_look_cases'], g['br_look_verdict']):
        if verdict == 'ok':
            BoundingBox([37, 38, -92, -91]).calc_buffer_ray('asc', lookDir=str(look))
        else:
            assert verdict == 'AssertionError'
            with pytest.raises(AssertionError, match='Incorrection look direction'):
                BoundingBox([37, 38, -92, -91]).calc_buffer_ray('asc', lookDir=str(look))
    with pytest.raises(AssertionError, match='Incorrection orbital direction'):
        BoundingBox([37, 38, -92, -91]).calc_buffer_ray('north')


def test_output_spacing_and_xygrid_equal_the_reference(golden):
    g = golden('g17_llreader')
    for ll_res, cs, deg, metric in zip(g['sp_ll_res'], g['sp_cube_spacing_m'], g['sp_deg'], g['sp_metric']):
        aoi = BoundingBox([20, 27, -115, -104], cube_spacing_in_m=_cube_spacing(cs))
        aoi.set_output_spacing(ll_res=float(ll_res))
        assert aoi.get_output_spacing(4326) == deg and aoi.get_output_spacing(4978) == metric and aoi.get_output_spacing('EPSG:32611') == metric
    with pytest.raises(AssertionError, match='Must pass lat/lon resolution'):
        BoundingBox([20, 27, -115, -104]).set_output_spacing()
    for i, (box, ll_res, cs) in enumerate(zip(g['xy_box'], g['xy_ll_res'], g['xy_cube_spacing_m'])):
        aoi = BoundingBox(list(box), cube_spacing_in_m=_cube_spacing(cs))
        aoi.add_buffer(float(ll_res))
        aoi.set_output_xygrid(4326)
        assert np.array_equal(aoi.xpts, g[f'xy_xpts_{i}']) and np.array_equal(aoi.ypts, g[f'xy_ypts_{i}']), i
        xp, yp = aoi.xpts.copy(), aoi.ypts.copy()
        aoi.set_output_xygrid('EPSG:4326')
        assert np.array_equal(aoi.xpts, xp) and np.array_equal(aoi.ypts, yp)


def test_reference_test_values():
    """test/test_llreader.py: test_read_bbox, test_aoi_epsg, test_set_output_dir, test_read_station_file, test_bounds_from_csv, test_readZ_sf."""
    bbox = [20, 27, -115, -104]
    query = BoundingBox(bbox)
    assert query.type() == 'bounding_box' and query.bounds() == bbox and query.bounds() is not bbox
    assert query.projection() == 4326 and query.geotransform() is None
    query.set_output_spacing(ll_res=0.05)
    assert query.get_output_spacing(4978) == 0.05 * 1e5
    query.set_output_directory('dummy_directory')
    assert query._output_directory == 'dummy_directory'
    aoi = StationFile(STATIONS_2)
    assert aoi.type() == 'station_file' and aoi.bounds() == [33.746, 36.795, -118.312, -114.892] == bounds_from_csv(STATIONS_2)
    assert np.array_equal(aoi.readZ(), np.full(aoi.readLL()[0].shape, 0.1))


def test_station_files_equal_the_reference(golden, tmp_path):
    g = golden('g17_llreader')
    for i, name in enumerate(g['st_file']):
        path = FILES / str(name)
        assert bounds_from_csv(path) == list(g[f'st_bounds_{i}'])
        aoi = StationFile(path)
        lats, lons = aoi.readLL()
        assert np.array_equal(lats, g[f'st_lats_{i}']) and np.array_equal(lons, g[f'st_lons_{i}']) and np.array_equal(aoi.readZ(), g[f'st_hgts_{i}'])
        assert aoi.bounds() == list(g[f'st_aoi_bounds_{i}'])
    # duplicates are dropped on (Lat, Lon); a file without heights and without a DEM says that nothing is downloaded here
    csv = tmp_path / 's.csv'
    csv.write_text('ID,Lat,Lon\nA,33.1,-117.2\nB,33.5,-117.9\nB2,33.5,-117.9\nC,34.0,-118.4\n')
    aoi = StationFile(csv)
    assert aoi.readLL()[0].tolist() == [33.1, 33.5, 34.0] and aoi.bounds() == [33.1, 34.0, -118.4, -117.2]
    with pytest.raises(FileNotFoundError, match='no DEM was given .* download'):
        aoi.readZ()


def test_get_file_and_band_equals_the_reference(golden):
    g = golden('g17_llreader')
    for s, path, band in zip(g['fb_string'], g['fb_path'], g['fb_band']):
        if band < 0:
            with pytest.raises(ValueError):
                get_file_and_band(str(s))
        else:
            assert get_file_and_band(str(s)) == (Path(str(path)), int(band))


def test_raster_aoi_constructor_errors(tmp_path):
    """test/test_llreader.py::test_latlon_reader_2 and test_badllfiles: every failure to read the pair is a ValueError."""
    with pytest.raises(ValueError, match='2-band file or two single-band files'):
        RasterRDR(lat_file=None, lon_file=None)
    with pytest.raises(ValueError, match='cannot be found'):
        RasterRDR(lat_file='doesnotexist.rdr', lon_file='doesnotexist.rdr')
    lat = str(S4 / 'lat.rdr')
    with pytest.raises(ValueError, match='Could not read lat/lon rasters'):
        RasterRDR(lat_file=lat, lon_file=str(S4 / 'lon_dummy.rdr'))
    with pytest.raises(ValueError, match='Could not read lat/lon rasters'):
        RasterRDR(lat_file=lat, lon_file=str(STATIONS_2))
    with pytest.raises(ValueError, match='Could not read lat/lon rasters'):
        RasterRDR(lat_file=str(STATIONS_2), lon_file=str(S4 / 'lon_dummy.rdr'))
    # mismatching rasters: another size, another geotransform
    rawraster.write_envi(np.ones((5, 9)), tmp_path / 'lon_small.rdr')
    with pytest.raises(ValueError, match='differ in size'):
        RasterRDR(lat_file=lat, lon_file=str(tmp_path / 'lon_small.rdr'))
    rawraster.write_envi(np.ones((5, 9)), tmp_path / 'a.rdr', geotransform=(-118.0, 0.01, 0.0, 34.0, 0.0, -0.01))
    rawraster.write_envi(np.ones((5, 9)), tmp_path / 'b.rdr', geotransform=(-118.0, 0.02, 0.0, 34.0, 0.0, -0.01))
    with pytest.raises(ValueError, match='Affine transform .* does not match'):
        RasterRDR(lat_file=str(tmp_path / 'a.rdr'), lon_file=str(tmp_path / 'b.rdr'))
    rawraster.write_envi(np.ones((5, 9)), tmp_path / 'c.rdr', geotransform=(500000.0, 30.0, 0.0, 3700000.0, 0.0, -30.0), proj=32611)
    with pytest.raises(ValueError, match='Projection information .* does not match'):
        RasterRDR(lat_file=str(tmp_path / 'a.rdr'), lon_file=str(tmp_path / 'c.rdr'))


@pytest.mark.parametrize('gt, proj, crs', [((-118.0, 0.01, 0.0, 34.0, 0.0, -0.01), None, 4326),
                                           ((-101.640625, 0.0009765625, 0.0, 21.5, 0.0, -0.00048828125), 4326, 4326),
                                           ((499980.0, 30.0, 0.0, 3700020.0, 0.0, -30.0), 32611, 32611),
                                           ((300000.5, 12.5, 0.0, 6100000.25, 0.0, -12.5), 32719, 32719)])
def test_geotransform_from_an_envi_header(tmp_path, gt, proj, crs):
    """What write_envi puts into `map info` comes back as the tuple that went in (geographic and UTM), with the CRS it names."""
    rawraster.write_envi(np.arange(35, dtype=np.int16).reshape(7, 5), tmp_path / 'dem.envi', geotransform=gt, proj=proj)
    data, prof = rawraster.rio_open(tmp_path / 'dem.envi')
    assert prof['transform'] == gt and prof['crs'] == crs and data.dtype == np.int16
    assert rio_profile(tmp_path / 'dem.envi')['transform'] == gt


def test_geotransform_from_a_vrt_and_none_without_one(tmp_path):
    a = np.arange(45, dtype=np.float64).reshape(5, 9)
    (tmp_path / 'hgt.rdr').write_bytes(a.tobytes())
    vrt = '''<VRTDataset rasterXSize="9" rasterYSize="5">%s<VRTRasterBand dataType="Float64" band="1">
      <SimpleSource><SourceFilename relativeToVRT="1">hgt.rdr</SourceFilename><SourceBand>1</SourceBand>
      <SourceProperties RasterXSize="9" RasterYSize="5" DataType="Float64" BlockXSize="9" BlockYSize="1" /></SimpleSource></VRTRasterBand></VRTDataset>'''
    (tmp_path / 'hgt.rdr.vrt').write_text(vrt % '<SRS>EPSG:4326</SRS><GeoTransform> -1.0164062500000000e+02,  9.7656250000000000e-04,  0.0,  2.15e+01,  0.0, -4.8828125e-04</GeoTransform>')
    data, prof = rawraster.rio_open(tmp_path / 'hgt.rdr')
    assert np.array_equal(data, a) and prof['transform'] == (-101.640625, 0.0009765625, 0.0, 21.5, 0.0, -0.00048828125) and prof['crs'] == 4326
    # a positive row step (south-up), which an ENVI header cannot say, survives a VRT
    (tmp_path / 'hgt.rdr.vrt').write_text(vrt % '<GeoTransform>10, 0.5, 0, -3, 0, 0.25</GeoTransform>')
    prof = rawraster.rio_open(tmp_path / 'hgt.rdr')[1]
    assert prof['transform'] == (10.0, 0.5, 0.0, -3.0, 0.0, 0.25) and prof['crs'] is None
    (tmp_path / 'hgt.rdr.vrt').write_text(vrt % '')
    assert rawraster.rio_open(tmp_path / 'hgt.rdr')[1]['transform'] is None
    # the reference's radar-geometry rasters carry neither map info nor a GeoTransform
    for name in ('lat.rdr', 'lon.rdr', 'warpedDEM.dem'):
        prof = rawraster.rio_open(S4 / name)[1]
        assert prof['transform'] is None and prof['crs'] is None, name


def test_rio_extents_and_geocoded_file(tmp_path):
    """utilFcns.py:154-161 and GeocodedFile.readLL (llreader.py:342-351) on a 7 x 5 raster, against the formulas written out."""
    gt = (-118.0, 0.25, 0.0, 34.0, 0.0, -0.125)
    h, w = 7, 5
    rawraster.write_envi(np.arange(h * w, dtype=np.float32).reshape(h, w), tmp_path / 'geo.envi', geotransform=gt)
    prof = rio_profile(tmp_path / 'geo.envi')
    S, N, W, E = rio_extents(prof)
    assert (W, E) == (gt[0], gt[0] + (w - 1) * gt[1]) and (N, S) == (gt[3], gt[3] + (w - 1) * gt[4] + (h - 1) * gt[5])
    assert (S, N, W, E) == (33.25, 34.0, -118.0, -117.0)
    aoi = GeocodedFile(tmp_path / 'geo.envi')
    assert aoi.type() == 'geocoded_file' and tuple(aoi.bounds()) == (S, N, W, E) and aoi.geotransform() == gt and aoi.projection() == 4326 and aoi.crs == 4326
    lats, lons = aoi.readLL()
    px, py = (E - W) / w, (N - S) / h
    assert lats.shape == lons.shape == (h, w)
    assert np.array_equal(lons[0], np.array([W + t * px for t in range(w)])) and np.array_equal(lats[:, 0], np.array([S + t * py for t in range(h)]))
    assert np.array_equal(lons, np.broadcast_to(lons[0], (h, w))) and np.array_equal(lats, np.broadcast_to(lats[:, :1], (h, w)))
    with pytest.raises(FileNotFoundError, match='download'):
        aoi.readZ()                                  # not a DEM, and nothing is downloaded
    # a raster that does not say where it lies cannot be a geocoded AOI
    rawraster.write_envi(np.zeros((h, w), dtype=np.float32), tmp_path / 'bare.envi')
    with pytest.raises(ValueError, match='no geotransform'):
        GeocodedFile(tmp_path / 'bare.envi')


def test_transform_bbox_identity_and_exports():
    box = [33.0, 34.0, -118.25, -116.75]
    assert transform_bbox(box, dest_crs=4326, src_crs=4326) is box and transform_bbox(box, dest_crs='EPSG:4326') is box
    import raider_amd
    for name in ('AOI', 'BoundingBox', 'StationFile', 'RasterRDR', 'GeocodedFile', 'Geocube', 'bounds_from_csv', 'bounds_from_latlon_rasters'):
        assert getattr(raider_amd, name) is getattr(llreader, name)


def test_geocube_reads_its_axes_and_heights(tmp_path):
    """llreader.py:366-394: the extent from `latitude` / `longitude`, readZ() = `heights`, from a NetCDF-4 cube file."""
    from raider_amd.h5write import write_netcdf4
    from raider_amd.llreader import Geocube
    lat, lon, h = np.linspace(34.0, 33.0, 5), np.linspace(-118.0, -117.0, 9), np.array([0.0, 100.0, 500.0])
    v = {'heights': (('heights',), h, {}), 'latitude': (('latitude',), lat, {}), 'longitude': (('longitude',), lon, {}),
         'wet': (('heights', 'latitude', 'longitude'), np.zeros((3, 5, 9)), {})}
    write_netcdf4(tmp_path / 'cube.nc', {'heights': 3, 'latitude': 5, 'longitude': 9}, v)
    aoi = Geocube(str(tmp_path / 'cube.nc'))
    assert aoi.type() == 'Geocube' and aoi.bounds() == [33.0, 34.0, -118.0, -117.0] and np.array_equal(aoi.readZ(), h)
    assert aoi.geotransform() == (-118.0625, 0.125, 0.0, 34.125, 0.0, -0.25) and aoi.projection() == 4326
    lats, lons = aoi.readLL()
    assert lats.shape == lons.shape == (9, 5) and np.array_equal(lats[0], lat) and np.array_equal(lons[:, 0], lon)      # np.meshgrid(lats, lons), as the reference writes it
