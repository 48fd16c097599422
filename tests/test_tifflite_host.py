"""CPU: raider_amd.tifflite without a device - directory parsing, georeferencing, the refusals, the host decoders (none, deflate,
PackBits; LZW is decoded on the GPU, tests/test_gpu_tifflite.py), the writer, the rio_* wiring, and the host sanitizer check of the
LZW functions the device kernel runs.  Independent decoders: Pillow's libtiff (where installed and where it reads the variant) and
the slow codec of tests/tiff_codec.py; a synthesised file is first shown to decode identically by Pillow, then used."""
import io
import os
import shutil
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

from raider_amd import tifflite
from raider_amd.tifflite import TiffInfo, UnsupportedTIFFFeature
from tests import tiff_codec as T

REPO = Path(__file__).resolve().parent.parent
DEM = REPO / 'tests' / 'golden' / 'ref_files' / 'scenario_0' / 'small_dem.tif'


def pillow_array(data):
    """Pillow's decode of TIFF bytes as (H, W) / (H, W, bands), or None where Pillow is absent or refuses the variant (it says so with
    an OSError - UnidentifiedImageError among them -, a SyntaxError or a ValueError; anything else is a failure)."""
    try:
        from PIL import Image
    except ImportError:
        return None
    try:
        with Image.open(io.BytesIO(data)) as im:
            return np.array(im)
    except (OSError, SyntaxError, ValueError):
        return None


def pillow_reads(arr, kw):
    """The variants Pillow's libtiff is known to read: one band of uint8 / uint16 / int16 / float32 in a little-endian classic file,
    uncompressed, LZW, deflate or PackBits.  For these a None from pillow_array is a failure of the synthesised file, not a skip."""
    try:
        import PIL  # noqa: F401
    except ImportError:
        return False
    return (arr.ndim == 2 and arr.dtype.name in ('uint8', 'uint16', 'int16', 'float32') and kw.get('byteorder', '<') == '<' and not kw.get('big')
            and kw.get('compression', 1) in (1, 5, 8, 32946, 32773))


def checked(tmp_path, name, arr, **kw):
    """make_tiff(arr, **kw) written to tmp_path / name, after Pillow (where it reads the file) has given `arr` back bit for bit."""
    data = T.make_tiff(arr, **kw)
    got = pillow_array(data)
    if kw.get('byteorder') == '>' and kw.get('compression', 1) != 1 and arr.dtype.name not in ('uint8', 'uint16'):
        # Pillow 12 swaps libtiff's (already native) output once more for big-endian files unless the mode is unsigned 16-bit: it returns
        # exactly the byte-swapped raster for int16 / int32 / float32 there, with and without a predictor.  Not a variant Pillow reads;
        # the big-endian uint16 cases, predictor 2 included, are the ones it confirms.
        got = None
    elif pillow_reads(arr, kw):
        assert got is not None, f'{name}: Pillow does not open a variant it is known to read - the synthesised file is malformed'
    if got is not None:
        want = arr if arr.ndim == 2 else arr.transpose(1, 2, 0)
        assert got.shape == want.shape and np.array_equal(got.astype(want.dtype), want), f'{name}: the synthesised file is not what Pillow reads'
    p = tmp_path / name
    p.write_bytes(data)
    return p


def _rng_raster(rng, dtype, shape):
    dt = np.dtype(dtype)
    if dt.kind == 'f':
        return rng.normal(0, 1000, shape).astype(dt)
    info = np.iinfo(dt)
    return rng.integers(info.min, info.max, shape, dtype=dt, endpoint=True)


def test_fixture_directory():
    """The reference's test DEM: 558 x 569 uint16 in 256 x 256 LZW tiles, UTM 18N, nodata 0 - against what Pillow reads of its tags."""
    info = TiffInfo(DEM)
    assert (info.width, info.height, info.count, info.dtype) == (558, 569, 1, np.dtype('uint16'))
    assert info.tiled and (info.tile_w, info.tile_h, info.tiles_x, info.tiles_y) == (256, 256, 3, 3)
    assert info.compression == 5 and info.predictor == 1 and not info.bigtiff and info.byteorder == '<'
    assert info.transform == (765953.0, 1.5, 0.0, 2045091.0, 0.0, -1.5) and info.crs == 32618 and info.nodata == 0.0
    p = info.profile()
    assert {k: p[k] for k in ('width', 'height', 'count', 'dtype', 'crs', 'nodata')} == dict(width=558, height=569, count=1, dtype='uint16', crs=32618, nodata=0.0)
    assert p['tags']['AREA_OR_POINT'] == 'Area' and p['transform'] == info.transform
    PIL = pytest.importorskip('PIL.Image')
    with PIL.open(DEM) as im:
        assert tuple(info.offsets) == tuple(im.tag_v2[324]) and tuple(info.bytecounts) == tuple(im.tag_v2[325])


@pytest.mark.parametrize('big', [False, True], ids=['classic', 'bigtiff'])
@pytest.mark.parametrize('order', ['<', '>'], ids=['little', 'big'])
def test_directory_of_synthesised_files(tmp_path, big, order):
    rng = np.random.default_rng(3)
    a = _rng_raster(rng, 'int16', (37, 53))
    p = checked(tmp_path, 'a.tif', a, big=big, byteorder=order, rows_per_strip=10, scale=(0.5, 0.25, 0), tiepoint=(0, 0, 0, -120.0, 35.0, 0), geokeys=T.GEO_4326,
                nodata=-32768, second_ifd=True)
    info = TiffInfo(p)
    assert info.bigtiff == big and info.byteorder == order and not info.tiled and (info.tile_h, info.tiles_y) == (10, 4)
    assert info.seg_rows(3) == 7 and info.swap == (order == '>')
    assert info.transform == (-120.0, 0.5, 0.0, 35.0, 0.0, -0.25) and info.crs == 4326 and info.nodata == -32768.0
    got, prof = tifflite.read(p)                                        # (the 1 x 1 overview in the second directory is ignored)
    assert got.dtype == np.int16 and np.array_equal(got, a) and prof['width'] == 53 and prof['height'] == 37


def test_georeferencing(tmp_path):
    a = np.zeros((4, 5), dtype=np.uint8)
    # a tie point away from the corner
    p = tmp_path / 't.tif'
    p.write_bytes(T.make_tiff(a, scale=(2.0, 3.0, 0), tiepoint=(1, 2, 0, 100.0, 50.0, 0)))
    assert TiffInfo(p).transform == (98.0, 2.0, 0.0, 56.0, 0.0, -3.0) and TiffInfo(p).crs is None and TiffInfo(p).nodata is None
    # a transformation matrix, north-up and rotated
    m = [2.0, 0.0, 0.0, 10.0, 0.0, -3.0, 0.0, 20.0, 0, 0, 0, 0, 0, 0, 0, 1]
    p.write_bytes(T.make_tiff(a, matrix=m))
    assert TiffInfo(p).transform == (10.0, 2.0, 0.0, 20.0, 0.0, -3.0) and TiffInfo(p).north_up_transform() == TiffInfo(p).transform
    m[1] = 0.5; m[4] = -0.25
    p.write_bytes(T.make_tiff(a, matrix=m))
    assert TiffInfo(p).transform == (10.0, 2.0, 0.5, 20.0, -0.25, -3.0)
    with pytest.raises(UnsupportedTIFFFeature, match='rotated'):
        TiffInfo(p).north_up_transform()
    # PixelIsPoint: GDAL moves the origin by half a pixel
    keys = [1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 2, 3072, 0, 1, 32611]
    p.write_bytes(T.make_tiff(a, scale=(30.0, 30.0, 0), tiepoint=(0, 0, 0, 500000.0, 3700000.0, 0), geokeys=keys))
    info = TiffInfo(p)
    assert info.transform == (499985.0, 30.0, 0.0, 3700015.0, 0.0, -30.0) and info.crs == 32611 and info.tags['AREA_OR_POINT'] == 'Point'
    # the projected key wins over the geographic one; a user-defined projected CRS falls back to it; GDAL_METADATA's item is kept
    keys = [1, 1, 0, 3, 1024, 0, 1, 1, 2048, 0, 1, 4269, 3072, 0, 1, 32767]
    p.write_bytes(T.make_tiff(a, geokeys=keys, nodata='nan', gdal_metadata='<GDALMetadata>\n  <Item name="AREA_OR_POINT">Area</Item>\n</GDALMetadata>'))
    info = TiffInfo(p)
    assert info.crs == 4269 and info.transform is None and np.isnan(info.nodata) and info.tags['AREA_OR_POINT'] == 'Area'


REFUSALS = [
    (dict(compression=7), 'JPEG'), (dict(compression=50000), 'ZSTD'), (dict(compression=34887), 'LERC'), (dict(compression=50001), 'WebP'),
    (dict(compression=8, predictor=3), 'floating-point predictor'), (dict(bits=4), 'sub-byte'), (dict(photometric=3), 'palette'), (dict(photometric=6), 'YCbCr'),
]


@pytest.mark.parametrize('kw,word', REFUSALS, ids=[w for _, w in REFUSALS])
def test_refusals_name_the_feature(tmp_path, kw, word):
    a = np.zeros((4, 6), dtype=np.float32 if kw.get('predictor') == 3 else np.uint8)
    data = T.make_tiff(a, **{k: v for k, v in kw.items() if k != 'predictor'})
    if kw.get('predictor') == 3:
        data = T.make_tiff(a, compression=8, extra=[(317, 'H', [3])])
    p = tmp_path / 'r.tif'
    p.write_bytes(data)
    with pytest.raises(UnsupportedTIFFFeature, match=word):
        tifflite.read(p)


def test_old_style_lzw_is_refused_by_name(tmp_path):
    """An LSB-first stream starts with its 9-bit Clear code as the bytes 00 01; the check runs before anything goes to a device."""
    info = TiffInfo(DEM)
    with pytest.raises(UnsupportedTIFFFeature, match='old-style LZW'):
        tifflite._check_lzw_flavour(info, bytes([0x00, 0x01]))
    tifflite._check_lzw_flavour(info, bytes([0x80, 0x00]))              # MSB-first Clear: fine


LAYOUTS = [dict(rows_per_strip=7), dict(tile=(16, 32)), dict(rows_per_strip=40)]


@pytest.mark.parametrize('compression', [1, 8, 32946, 32773], ids=['none', 'deflate', 'deflate-old', 'packbits'])
@pytest.mark.parametrize('layout', LAYOUTS, ids=['strips', 'tiles', 'one-strip'])
def test_host_decoders_against_pillow(tmp_path, compression, layout):
    rng = np.random.default_rng(11)
    a = (rng.integers(0, 6, (37, 53)) * 40).astype(np.uint8)            # runs, so PackBits has both packet kinds
    a[5, 3:50] = 9
    p = checked(tmp_path, 'x.tif', a, compression=compression, **layout)
    assert np.array_equal(tifflite.read(p)[0], a)
    b = _rng_raster(rng, 'int16', (37, 53))
    p = checked(tmp_path, 'y.tif', b, compression=compression, predictor=2, **layout)      # (none / PackBits: the tag is there and ignored, as in libtiff)
    assert np.array_equal(tifflite.read(p)[0], b)


@pytest.mark.parametrize('dtype', ['uint8', 'uint16', 'uint32', 'int8', 'int16', 'int32', 'float32', 'float64'])
def test_sample_types_bands_and_byte_orders_on_the_host(tmp_path, dtype):
    rng = np.random.default_rng(5)
    a = _rng_raster(rng, dtype, (3, 19, 70))
    for planar in (1, 2):
        for order in '<>':
            p = checked(tmp_path, 'm.tif', a, planar=planar, byteorder=order, compression=8, tile=(16, 16),
                        predictor=2 if np.dtype(dtype).kind != 'f' else 1)
            got, prof = tifflite.read(p)
            assert got.dtype == np.dtype(dtype) and got.shape == (3, 19, 70) and np.array_equal(got.view(f'u{got.itemsize}'), a.view(f'u{a.itemsize}'))
            assert prof['count'] == 3
            one, _ = tifflite.read(p, band=2)
            assert one.shape == (19, 70) and np.array_equal(one.view(f'u{one.itemsize}'), a[1].view(f'u{a.itemsize}'))
    with pytest.raises(IndexError):
        tifflite.read(p, band=4)


@pytest.mark.parametrize('dtype', ['int16', 'float32', 'float64'])
@pytest.mark.parametrize('compress', [None, 'deflate'])
def test_writer_round_trip(tmp_path, dtype, compress):
    """write -> Pillow gives the pixels; write -> read gives array, transform, EPSG and nodata bit for bit; 300 rows of 150 float64
    are 360 KB: several 64 KiB strips."""
    rng = np.random.default_rng(8)
    a = _rng_raster(rng, dtype, (300, 150))
    gt = (-118.25, 0.01 / 3, 0.0, 34.5, 0.0, -0.0025)
    p = tmp_path / 'w.tif'
    tifflite.write(p, a, transform=gt, crs=4326, nodata=-9999.0, compress=compress)
    info = TiffInfo(p)
    assert len(info.offsets) > 1 and info.compression == (8 if compress else 1) and not info.bigtiff
    back, prof = tifflite.read(p)
    assert back.dtype == a.dtype and np.array_equal(back.view(f'u{a.itemsize}'), a.view(f'u{a.itemsize}'))
    assert prof['transform'] == gt and prof['crs'] == 4326 and prof['nodata'] == -9999.0
    got = pillow_array(p.read_bytes())
    if dtype != 'float64':                                              # (Pillow has no 64-bit float mode)
        pytest.importorskip('PIL')
        assert got is not None and np.array_equal(got.astype(a.dtype), a)
    # a projected CRS goes into the projected key; no CRS and no nodata leave the tags out
    tifflite.write(p, a, transform=(500000.0, 30.0, 0.0, 3700000.0, 0.0, -30.0), crs='EPSG:32611')
    prof = tifflite.read(p)[1]
    assert prof['crs'] == 32611 and prof['nodata'] is None and prof['transform'] == (500000.0, 30.0, 0.0, 3700000.0, 0.0, -30.0)
    assert tifflite._geokey(TiffInfo(p).ifd, 3072) == 32611 and tifflite._geokey(TiffInfo(p).ifd, 2048) is None
    with pytest.raises(TypeError, match='int16'):
        tifflite.write(p, a.astype(np.complex64))


def test_bigtiff_layout_of_the_writer(tmp_path, monkeypatch):
    """The writer's BigTIFF branch without 4 GiB of pixels: the size above which it switches (tifflite._BIGTIFF_ABOVE) is lowered, the
    file stays small.  Header (magic 43), 20-byte entries and 8-byte LONG8 offsets are read back.  Offsets beyond 32 bits are not
    exercised: that needs a file of more than 4 GiB."""
    a = np.arange(12, dtype=np.int16).reshape(3, 4)
    assert tifflite._BIGTIFF_ABOVE == 0xFFFF0000
    monkeypatch.setattr(tifflite, '_BIGTIFF_ABOVE', 0)
    p = tmp_path / 'b.tif'
    tifflite.write(p, a, transform=(0.0, 1.0, 0.0, 3.0, 0.0, -1.0), crs=4326, nodata=-1)
    assert p.read_bytes()[:4] == b'II+\x00'
    back, prof = tifflite.read(p)
    assert TiffInfo(p).bigtiff and np.array_equal(back, a) and prof['crs'] == 4326 and prof['nodata'] == -1.0
    got = pillow_array(p.read_bytes())
    assert got is None or np.array_equal(got, a)


def test_rio_routes_take_geotiffs_without_rasterio(tmp_path):
    try:
        import rasterio  # noqa: F401
        pytest.skip('rasterio reads the raster itself')
    except ImportError:
        pass
    from raider_amd import rawraster, utilFcns
    rng = np.random.default_rng(2)
    a = _rng_raster(rng, 'float32', (2, 6, 8))
    p = checked(tmp_path, 'los.tif', a, compression=8, planar=2, scale=(0.1, 0.1, 0), tiepoint=(0, 0, 0, -118.0, 34.0, 0), geokeys=T.GEO_4326, nodata=0)
    data, prof = rawraster.rio_open(p)
    assert data.shape == (2, 6, 8) and np.array_equal(data, a) and prof['count'] == 2 and prof['crs'] == 4326
    assert np.array_equal(utilFcns.rio_open(p, band=2)[0], a[1])
    assert utilFcns.rio_profile(p)['transform'] == (-118.0, 0.1, 0.0, 34.0, 0.0, -0.1)
    with rawraster.open_raster(p) as src:
        assert src.count == 2 and src.nodatavals == (0.0, 0.0) and src.read().shape == (2, 6, 8) and src.read(1).shape == (6, 8)
    # writeDelays: GTiff without rasterio, float64 delays as float32 with the AOI's geotransform
    w = rng.uniform(0, 0.3, (7, 9)); h = rng.uniform(1.8, 2.4, (7, 9)); w[2, 3] = np.nan
    aoi = type('R', (), dict(type=lambda self: 'radar_rasters', projection=lambda self: 'EPSG:4326', geotransform=lambda self: (-118.0, 0.01, 0.0, 34.0, 0.0, -0.01)))()
    utilFcns.writeDelays(aoi, w, h, tmp_path / 'wet.tif', tmp_path / 'hydro.tif', outformat='GTiff', ndv=-9999.0)
    back, prof = utilFcns.rio_open(tmp_path / 'wet.tif')
    assert back.dtype == np.float32 and np.array_equal(back, w.astype(np.float32)) and back[2, 3] == -9999.0
    assert prof['nodata'] == -9999.0 and prof['crs'] == 4326 and prof['transform'] == (-118.0, 0.01, 0.0, 34.0, 0.0, -0.01)
    assert np.array_equal(utilFcns.rio_open(tmp_path / 'hydro.tif')[0], h.astype(np.float32))
    # a `<file>.vrt` beside a TIFF describes the file, on every route: the raw-raster reader gets it (and refuses this empty one)
    shutil.copy(p, tmp_path / 'sided.tif')
    (tmp_path / 'sided.tif.vrt').write_text('<VRTDataset rasterXSize="8" rasterYSize="6"></VRTDataset>')
    with pytest.raises(rawraster.NotARawRaster):
        rawraster.open_raster(tmp_path / 'sided.tif')
    # a non-TIFF without a side-car still goes to the raw-raster route and is refused there
    (tmp_path / 'junk.bin').write_bytes(b'\x01\x02\x03\x04\x05')
    with pytest.raises(rawraster.NotARawRaster):
        rawraster.rio_open(tmp_path / 'junk.bin')


def test_in_test_codec_is_self_consistent_and_matches_pillow(tmp_path):
    """The slow LZW codec: decode(encode(x)) == x for every good case, and an LZW file made with it is what Pillow's libtiff reads."""
    for name, (stream, cap) in T.lzw_cases().items():
        out, status = T.lzw_decode(stream, cap)
        assert (status != 0) == (name.startswith('bad_')), name
    rng = np.random.default_rng(4)
    a = rng.integers(0, 256, (64, 300), dtype=np.uint8)                 # 19 KB of noise per strip: the table fills and is cleared
    data = T.make_tiff(a, compression=5)
    st = {}
    T.lzw_encode(a.tobytes(), stats=st)
    assert st['clears'] >= 1
    pytest.importorskip('PIL')
    assert np.array_equal(pillow_array(data), a)
    seg = data[8:8 + struct.unpack('<I', data[data.index(struct.pack('<HHI', 279, 4, 1)) + 8:][:4])[0]]
    assert T.lzw_decode(seg, a.size) == (a.tobytes(), 0)


def _fnv1a(b):
    h = 1469598103934665603
    for v in b:
        h = ((h ^ v) * 1099511628211) & (2 ** 64 - 1)
    return h


def test_lzw_host_functions_are_clean_under_sanitizers(tmp_path):
    """tools/probes/lzw_host_check.cpp - the __host__ __device__ bit reader, table update and string expansion the device kernel runs -
    built for the CPU with AddressSanitizer and UBSan and fed every stream of lzw_cases(), the damaged ones included, from heap blocks
    of exactly each stream's size: it must exit clean and give the in-test decoder's status, length and bytes.  A stand-alone
    program: nothing with a sanitizer is loaded into this process, and nothing runs on a GPU."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not (shutil.which(hipcc) or Path(hipcc).exists()):
        pytest.skip('no hipcc to build the probe with')
    exe = tmp_path / 'lzw_host_check'
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all',
                    str(REPO / 'tools' / 'probes' / 'lzw_host_check.cpp'), '-o', str(exe)], check=True)
    cases = T.lzw_cases()
    blob = struct.pack('<I', len(cases)) + b''.join(struct.pack('<II', len(s), cap) + s for s, cap in cases.values())
    (tmp_path / 'streams.bin').write_bytes(blob)
    r = subprocess.run([str(exe), str(tmp_path / 'streams.bin')], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-3000:]
    lines = r.stdout.split('\n')[:-1]
    assert len(lines) == len(cases)
    for line, (name, (s, cap)) in zip(lines, cases.items()):
        out, status = T.lzw_decode(s, cap)
        assert line == f'{status} {len(out)} {_fnv1a(out):016x}', name


def test_geocoded_file_aoi_reads_a_geotiff_profile(tmp_path):
    try:
        import rasterio  # noqa: F401
        pytest.skip('rasterio reads the raster itself')
    except ImportError:
        pass
    from raider_amd.llreader import GeocodedFile
    a = np.zeros((20, 30), dtype=np.float32)
    p = checked(tmp_path, 'geo.tif', a, compression=8, scale=(0.01, 0.02, 0), tiepoint=(0, 0, 0, -118.0, 34.0, 0), geokeys=T.GEO_4326)
    aoi = GeocodedFile(str(p))
    assert aoi.type() == 'geocoded_file' and aoi._proj == 4326 and aoi._geotransform == (-118.0, 0.01, 0.0, 34.0, 0.0, -0.02)
    S, N, W, E = aoi._bounding_box
    assert (N, W) == (34.0, -118.0) and np.isclose(S, 34.0 - 19 * 0.02) and np.isclose(E, -118.0 + 29 * 0.01)
    lats, lons = aoi.readLL()
    assert lats.shape == (20, 30)
