"""GPU: GeoTIFF tiles and strips decoded on the device - rdr_tiff_lzw_decode (one wave per LZW segment, string table in LDS) and
rdr_tiff_assemble (padding, byte order, predictor 2) - through raider_amd.tifflite and the DEM / LOS routes that now take GeoTIFFs.
References: Pillow's libtiff for the reference's own test DEM, the slow codec of tests/tiff_codec.py for every synthesised stream,
NumPy for the assembly (the arrays the files were made from)."""
import struct
from pathlib import Path

import numpy as np
import pytest

from raider_amd import tifflite
from raider_amd.interpolator import interpolate_elevation, interpolateDEM
from tests import tiff_codec as T
from tests.test_gpu_llreader import nearest_ref
from tests.test_tifflite_host import DEM, _rng_raster, checked

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')


def _dev():
    return torch.device('cuda', 0)


@pytest.fixture(scope='module')
def pillow_dem():
    Image = pytest.importorskip('PIL.Image')
    with Image.open(DEM) as im:
        a = np.array(im)
    assert a.dtype == np.uint16 and a.shape == (569, 558)
    return a


@pytest.fixture(scope='module')
def dem_4326(tmp_path_factory):
    """The fixture's own bytes - libtiff's LZW tiles untouched - with the three GeoKey words that say `projected, EPSG:32618` rewritten
    to `geographic, EPSG:4326`: the DEM routes take lon / lat DEMs only (that refusal stays), and the fixture is in UTM 18N."""
    data = bytearray(DEM.read_bytes())
    old_model, new_model = struct.pack('<4H', 1024, 0, 1, 1), struct.pack('<4H', 1024, 0, 1, 2)
    old_crs, new_crs = struct.pack('<4H', 3072, 0, 1, 32618), struct.pack('<4H', 2048, 0, 1, 4326)
    assert data.count(old_model) == 1 and data.count(old_crs) == 1
    data[data.index(old_model):][:8] = new_model
    k = data.index(old_crs)
    data[k:k + 8] = new_crs
    p = tmp_path_factory.mktemp('dem') / 'small_dem_4326.tif'
    p.write_bytes(bytes(data))
    assert tifflite.TiffInfo(p).crs == 4326
    return p


def test_fixture_equals_pillow_to_numpy_and_to_a_device_tensor(pillow_dem):
    a, prof = tifflite.read(DEM)
    assert isinstance(a, np.ndarray) and a.dtype == np.uint16 and np.array_equal(a, pillow_dem)
    assert prof['crs'] == 32618 and prof['nodata'] == 0.0 and prof['transform'] == (765953.0, 1.5, 0.0, 2045091.0, 0.0, -1.5)
    t, _ = tifflite.read(DEM, device=_dev())
    assert t.is_cuda and t.dtype == torch.uint16 and tuple(t.shape) == (569, 558)
    assert np.array_equal(t.cpu().numpy(), pillow_dem)
    b, _ = tifflite.read(DEM, band=1, device=_dev())
    assert np.array_equal(b.cpu().numpy(), pillow_dem)


def _dem_points(gt, h, w, rng):
    x0, dx, _, y0, _, dy = gt
    xe, ye = x0 + np.arange(w + 1) * dx, y0 + np.arange(h + 1) * dy
    xs = [rng.uniform(xe.min(), xe.max(), 3000), xe, rng.uniform(xe.min(), xe.max(), ye.size), rng.uniform(xe.min() - 50, xe.max() + 50, 500), np.array([np.nan, x0])]
    ys = [rng.uniform(ye.min(), ye.max(), 3000), rng.uniform(ye.min(), ye.max(), xe.size), ye, rng.uniform(ye.min() - 50, ye.max() + 50, 500), np.array([y0, np.nan])]
    return np.concatenate(xs), np.concatenate(ys)


def test_interpolate_elevation_from_the_geotiff(pillow_dem, dem_4326):
    """interpolate_elevation(<GeoTIFF path>, x, y) at points inside, on every pixel edge, outside and NaN equals the NumPy rule
    (tests/test_gpu_llreader.py: nearest_ref) on Pillow's array, for host points and for device points (the DEM is then decoded on
    the device).  Without tifflite the path cannot be read at all: this is the test that fails without the feature.  The fixture is in UTM 18N
    (EPSG:32618) and the DEM routes take lon / lat DEMs only, so the call is made on the same bytes re-tagged EPSG:4326 (fixture
    dem_4326), and the untouched file is shown to be refused by its CRS."""
    gt = (765953.0, 1.5, 0.0, 2045091.0, 0.0, -1.5)
    x, y = _dem_points(gt, 569, 558, np.random.default_rng(3))
    want = nearest_ref(pillow_dem, gt, x, y)
    assert np.isnan(want).sum() > 100 and np.isfinite(want).sum() > 3000
    got = interpolate_elevation(str(dem_4326), x, y)
    assert np.array_equal(got.view(np.int64), want.view(np.int64))
    xt, yt = torch.from_numpy(x).to(_dev()), torch.from_numpy(y).to(_dev())
    got_t = interpolate_elevation(dem_4326, xt, yt)
    assert got_t.is_cuda and np.array_equal(got_t.cpu().numpy().view(np.int64), want.view(np.int64))
    lin = interpolateDEM(dem_4326, (yt, xt))                             # the 1-D branch: bilinear, from the device-decoded DEM as well
    lin_host = interpolateDEM(dem_4326, (y, x))
    assert np.array_equal(lin.cpu().numpy().view(np.int64), lin_host.view(np.int64)) and np.isfinite(lin_host).sum() > 3000
    with pytest.raises(ValueError, match='32618'):
        interpolate_elevation(DEM, x, y)
    from raider_amd.utilFcns import rio_stats
    stats, crs, gt2 = rio_stats(DEM)
    valid = pillow_dem[pillow_dem != 0]
    assert (stats.min, stats.max, stats.count) == (float(valid.min()), float(valid.max()), valid.size) and crs == 32618 and gt2 == gt


def _decode(cases, stride=None, sentinel=0xA5):
    """Every (stream, cap) in one rdr_tiff_lzw_decode call; returns (status, out bytes as (n, stride) with the sentinel where nothing was written)."""
    streams = [s for s, _ in cases]
    caps = np.array([c for _, c in cases], dtype=np.int64)
    stride = stride or int(max(caps.max(), 1) + 7)
    lens = np.array([len(s) for s in streams], dtype=np.int64)
    gap = 5                                                             # bytes between streams in the source buffer: never to be read
    offs = np.cumsum(np.concatenate([[3], lens[:-1] + gap])).astype(np.int64)
    src = np.full(int(offs[-1] + lens[-1] + gap), 0xFF, dtype=np.uint8)
    for o, s in zip(offs, streams):
        src[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
    out = torch.full((len(cases) * stride,), sentinel, dtype=torch.uint8, device=_dev())
    status = tifflite.lzw_decode_device(torch.from_numpy(src).to(_dev()), offs, lens, caps, out, stride)
    return status.cpu().numpy(), out.cpu().numpy().reshape(len(cases), stride)


def _check(cases, status, out, sentinel=0xA5):
    for i, (s, cap) in enumerate(cases):
        want, st = T.lzw_decode(s, cap)
        assert status[i] == st, (i, status[i], st)
        assert out[i, :len(want)].tobytes() == want, i
        assert np.all(out[i, len(want):] == sentinel), i                # nothing written past what the stream gives, nor outside the slot


def test_lzw_streams_against_the_in_test_decoder():
    """Width changes 9 -> 12, a table that fills and is cleared, code == next free entry, EOI before the slot is full, a one-byte
    segment, an odd output size, a stream without EOI that ends as its slot is full."""
    named = {k: v for k, v in T.lzw_cases().items() if not k.startswith('bad_')}
    assert len(named) == 7
    cases = list(named.values())
    status, out = _decode(cases)
    assert not status.any()
    _check(cases, status, out)
    assert out[list(named).index('eoi_before_full'), :33].tobytes() == b'hello world' * 3


def test_300_unequal_segments_in_one_call():
    """More waves than one compute unit holds, sizes from 1 byte to 9 KB (two staging windows), low- and high-entropy bytes."""
    rng = np.random.default_rng(77)
    cases = []
    for i in range(300):
        n = int(rng.integers(1, 9000)) if i % 7 else int(rng.integers(1, 40))
        hi = int(rng.choice([2, 16, 256]))
        d = rng.integers(0, hi, n, dtype=np.uint8).tobytes()
        cases.append((T.lzw_encode(d), n))
    status, out = _decode(cases)
    assert not status.any()
    for i, (s, n) in enumerate(cases):
        assert out[i, :n].tobytes() == T.lzw_decode(s, n)[0] and np.all(out[i, n:] == 0xA5), i


def test_bad_streams_return_a_status_and_touch_nothing_else():
    """Truncated input, a code beyond the table, a first code that is no byte, an output slot shorter than the stream, an empty
    segment - between good ones, in one call.  The slots and the gaps between them hold a sentinel before the call; afterwards every
    byte that the in-test decoder does not produce still holds it.  The same streams (tiff_codec.lzw_cases) pass through the same
    functions on the CPU under AddressSanitizer and UBSan in tests/test_tifflite_host.py; running that suite first is a matter of
    procedure (NOTES.md), not something this test can enforce."""
    named = T.lzw_cases()
    order = ['one_byte', 'bad_truncated', 'odd_output', 'bad_code_beyond_table', 'bad_first_code_not_a_byte', 'run_of_one_byte', 'bad_output_shorter', 'bad_empty',
             'eoi_before_full']
    cases = [named[k] for k in order]
    status, out = _decode(cases)
    assert list(status) == [0, 1, 0, 2, 2, 0, 1, 1, 0]
    _check(cases, status, out)
    assert out[3, :2].tobytes() == b'AB' and np.all(out[4] == 0xA5) and np.all(out[7] == 0xA5)
    # the entry refuses tables that point outside the buffers
    src = torch.zeros(64, dtype=torch.uint8, device=_dev()); dst = torch.zeros(64, dtype=torch.uint8, device=_dev())
    for offs, lens, caps in (([60], [8], [16]), ([-1], [8], [16]), ([0], [8], [65])):
        with pytest.raises(ValueError, match='rdr_tiff_lzw_decode'):
            tifflite.lzw_decode_device(src, np.array(offs), np.array(lens), np.array(caps), dst, 64)


ASSEMBLY = [
    # name, dtype, shape, make_tiff keywords
    ('tiles_edge_padding_lzw', 'int16', (70, 150), dict(tile=(32, 64), compression=5)),
    ('strips_short_last_lzw', 'uint8', (37, 53), dict(rows_per_strip=10, compression=5)),
    ('one_strip_plain_copy', 'float32', (19, 33), dict()),
    ('pred2_uint8_wraps_rows_over_64', 'uint8', (9, 201), dict(tile=(16, 208), compression=5, predictor=2)),
    ('pred2_int16_tiles', 'int16', (40, 131), dict(tile=(16, 80), compression=8, predictor=2)),
    ('pred2_uint32_strips', 'uint32', (11, 129), dict(rows_per_strip=4, compression=8, predictor=2)),
    ('big_endian_uint16_pred2', 'uint16', (21, 67), dict(byteorder='>', compression=5, predictor=2, rows_per_strip=8)),
    ('big_endian_int16_pred2', 'int16', (21, 67), dict(byteorder='>', compression=5, predictor=2, rows_per_strip=8)),
    ('big_endian_float32', 'float32', (21, 67), dict(byteorder='>', tile=(16, 16))),
    ('float64_deflate', 'float64', (21, 67), dict(compression=8, rows_per_strip=5)),
    ('big_endian_float64_bigtiff', 'float64', (5, 9), dict(byteorder='>', big=True)),
    ('chunky_3_bands_pred2', 'int16', (3, 30, 70), dict(tile=(16, 32), compression=5, predictor=2)),
    ('planar_3_bands_pred2', 'uint8', (3, 30, 70), dict(tile=(16, 32), compression=5, predictor=2, planar=2)),
    ('chunky_3_bands_strips_packbits', 'uint8', (3, 30, 70), dict(rows_per_strip=7, compression=32773)),
    ('planar_3_bands_float32_one_strip', 'float32', (3, 12, 20), dict(planar=2)),
]


@pytest.mark.parametrize('name,dtype,shape,kw', ASSEMBLY, ids=[a[0] for a in ASSEMBLY])
def test_assembly_on_the_device(tmp_path, name, dtype, shape, kw):
    """read(device=) of a synthesised file equals the array it was made from (which Pillow, where it reads the variant, has confirmed the
    file holds), bit for bit: all bands and each single band; and read() to NumPy agrees."""
    rng = np.random.default_rng(len(name))
    a = _rng_raster(rng, dtype, shape)
    if 'wraps' in name:
        a[:, ::3] = 255; a[:, 1::3] = 0                                  # differences that wrap modulo 256 all along the row
    p = checked(tmp_path, name + '.tif', a, **kw)
    u = f'u{a.itemsize}'
    t, prof = tifflite.read(p, device=_dev())
    assert t.is_cuda and tuple(t.shape) == a.shape and np.array_equal(t.cpu().numpy().view(u), a.view(u))
    if a.ndim == 3:
        for b in (1, 3):
            one, _ = tifflite.read(p, band=b, device=_dev())
            assert tuple(one.shape) == a.shape[1:] and np.array_equal(one.cpu().numpy().view(u), a[b - 1].view(u))
    host, _ = tifflite.read(p)
    assert host.dtype == a.dtype and np.array_equal(host.view(u), a.view(u))


def test_conventional_los_from_a_two_band_geotiff(tmp_path):
    """Conventional(filename=<2-band float32 LOS GeoTIFF>) divides exactly as with the same two rasters in the ISCE flat-binary form
    (the route that existed), and as with them passed as inc= / heading= up to float32: the file routes take cos(inc) in the raster's
    float32, as the reference does, the array route in float64 - one rounding of the argument's degree -> radian product, one of the
    cosine and one of the result, each 2^-24 relative, the first weighted by inc * tan(inc) <= 0.79 below 45 degrees: 3 * 2^-24."""
    from raider_amd.losreader import Conventional
    from tests.test_rawraster import _los_raster
    rng = np.random.default_rng(2)
    inc, hd = _los_raster(tmp_path, rng)
    checked(tmp_path, 'los.tif', np.stack([inc, hd]), planar=2, compression=8, rows_per_strip=4)
    lats = rng.uniform(30, 31, (6, 8)); lons = rng.uniform(-118, -117, (6, 8)); ztd = rng.uniform(2.0, 2.5, (6, 8))
    out = {}
    for key, kw in (('tif', dict(filename=str(tmp_path / 'los.tif'))), ('rdr', dict(filename=str(tmp_path / 'los.rdr'))), ('arrays', dict(inc=inc, heading=hd))):
        los = Conventional(**kw)
        los.setPoints(lats, lons, np.zeros((6, 8)))
        out[key] = los(ztd)
    assert np.array_equal(out['tif'], out['rdr'])
    np.testing.assert_allclose(out['tif'], out['arrays'], rtol=3 * 2.0 ** -24, atol=0)
    assert np.abs(out['tif'] / out['arrays'] - 1).max() > 0              # (the float32 cosine is really in there)


def test_geocoded_file_aoi_over_the_geotiff_dem(pillow_dem, dem_4326):
    """GeocodedFile(<GeoTIFF>, is_dem=True): extent, geotransform and CRS from the file's tags; readZ() = the DEM sampled at readLL()."""
    from raider_amd.llreader import GeocodedFile
    gt = (765953.0, 1.5, 0.0, 2045091.0, 0.0, -1.5)
    aoi = GeocodedFile(str(dem_4326), is_dem=True)
    assert aoi.type() == 'geocoded_file' and aoi._geotransform == gt and aoi._proj == 4326
    assert tuple(aoi._bounding_box) == (gt[3] + 568 * gt[5], gt[3], gt[0], gt[0] + 557 * gt[1])
    lats, lons = aoi.readLL()
    z = aoi.readZ()
    assert z.shape == lats.shape == (569, 558)
    assert np.array_equal(z.view(np.int64), nearest_ref(pillow_dem, gt, lons, lats).view(np.int64)) and np.isfinite(z).sum() > 300000
