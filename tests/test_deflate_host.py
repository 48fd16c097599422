"""CPU: the parts of the device-deflate work that need no device - chunked, filtered datasets of raider_amd.h5write against three
independent readers (raider_amd.h5lite, h5dump, libhdf5's H5Dread through ctypes), tifflite.write's predictor 2 on the host encoder
against tifflite.read and Pillow, and the encoder's size bound.  Chunk bytes are made here by NumPy shuffle + zlib.compress: the
writer lays the file out and never compresses."""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest

from raider_amd import h5lite, h5write, tifflite

REPO = Path(__file__).resolve().parent.parent
DEM = REPO / 'tests' / 'golden' / 'ref_files' / 'scenario_0' / 'small_dem.tif'
H5DUMP = shutil.which('h5dump') or ('/opt/conda/bin/h5dump' if os.path.exists('/opt/conda/bin/h5dump') else None)
LIBHDF5 = '/opt/conda/lib/libhdf5.so'
LIBHDF5_HL = '/opt/conda/lib/libhdf5_hl.so'


def host_chunks(a, chunk, fill, level=6):
    """(packed, offsets): NumPy's restatement of HDF5's chunking + shuffle filter, zlib for deflate."""
    grid = tuple(-(-s // c) for s, c in zip(a.shape, chunk))
    padded = np.full(tuple(g * c for g, c in zip(grid, chunk)), fill, dtype=a.dtype)
    padded[tuple(slice(0, s) for s in a.shape)] = a
    parts = []
    for idx in np.ndindex(*grid):
        blk = np.ascontiguousarray(padded[tuple(slice(i * c, (i + 1) * c) for i, c in zip(idx, chunk))])
        parts.append(zlib.compress(blk.reshape(-1).view(np.uint8).reshape(-1, a.itemsize).T.tobytes(), level))
    return b''.join(parts), np.cumsum([0] + [len(p) for p in parts])


def cube_file(path, a, chunk, fill):
    nz, ny, nx = a.shape
    packed, offs = host_chunks(a, chunk, fill)
    data = h5write.ChunkedData(a.shape, a.dtype, chunk, packed, offs, filters=('shuffle', 'deflate'))
    v = {'z': (('z',), np.arange(nz, dtype=np.float64), {'units': 'm'}), 'y': (('y',), np.linspace(30, 31, ny), {}), 'x': (('x',), np.linspace(-100, -99, nx), {}),
         'wet': (('z', 'y', 'x'), data, {'units': 'm', '_FillValue': fill}),
         'plain': (('z', 'y', 'x'), a, {'units': 'm'})}
    h5write.write_netcdf4(path, {'z': nz, 'y': ny, 'x': nx}, v)
    return v


def _h5():
    h5 = C.CDLL(LIBHDF5, mode=C.RTLD_GLOBAL); hl = C.CDLL(LIBHDF5_HL)
    hid = C.c_int64
    h5.H5open.restype = C.c_int
    h5.H5Fopen.restype = hid; h5.H5Fopen.argtypes = [C.c_char_p, C.c_uint, hid]
    h5.H5Dopen2.restype = hid; h5.H5Dopen2.argtypes = [hid, C.c_char_p, hid]
    h5.H5Dread.restype = C.c_int; h5.H5Dread.argtypes = [hid, hid, hid, hid, hid, C.c_void_p]
    h5.H5Dclose.argtypes = [hid]; h5.H5Fclose.argtypes = [hid]
    hl.H5DSis_attached.restype = C.c_int; hl.H5DSis_attached.argtypes = [hid, hid, C.c_uint]
    assert h5.H5open() >= 0
    return h5, hl, hid


def libhdf5_read(path, name, shape, dtype, scales=()):
    """H5Dread of one dataset in its own element type; asserts that every (axis, scale name) of `scales` is attached."""
    h5, hl, hid = _h5()
    f = h5.H5Fopen(str(path).encode(), 0, 0)
    assert f >= 0
    d = h5.H5Dopen2(f, name.encode(), 0)
    assert d >= 0
    native = hid.in_dll(h5, 'H5T_NATIVE_DOUBLE_g' if np.dtype(dtype) == np.float64 else 'H5T_NATIVE_FLOAT_g').value
    buf = np.full(shape, 7.0, dtype=dtype)
    assert h5.H5Dread(d, native, 0, 0, 0, buf.ctypes.data_as(C.c_void_p)) >= 0
    for ax, nm in scales:
        s = h5.H5Dopen2(f, nm.encode(), 0)
        assert s >= 0 and hl.H5DSis_attached(d, s, ax) == 1
        h5.H5Dclose(s)
    h5.H5Dclose(d); h5.H5Fclose(f)
    return buf


def _bits(a):
    return np.ascontiguousarray(a).view(f'u{a.dtype.itemsize}')


CASES = [((7, 10, 11), (7, 3, 3), 'rng'), ((1, 1, 1), (1, 1, 1), 'rng'), ((7, 10, 11), (7, 3, 3), 'nan')]


@pytest.mark.parametrize('fill', [np.nan, 0.0], ids=['fill_nan', 'fill_zero'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
@pytest.mark.parametrize('shape,chunk,content', CASES, ids=['partial_edges_16_chunks', 'one_element', 'all_nan'])
def test_chunked_filtered_variable_against_three_readers(tmp_path, shape, chunk, content, dtype, fill):
    rng = np.random.default_rng(5)
    a = rng.standard_normal(shape).astype(dtype) if content == 'rng' else np.full(shape, np.nan, dtype=dtype)
    if content == 'rng' and a.size > 4:
        a[0, 1, 2] = np.nan; a[-1, -1, -1] = 0.0
    p = tmp_path / 'c.nc'
    cube_file(p, a, chunk, fill)
    # 1. h5lite
    f = h5lite.File(p)
    got = f['wet'].read()
    assert got.dtype == a.dtype and got.shape == a.shape and np.array_equal(_bits(got), _bits(a))
    assert np.array_equal(_bits(f['plain'].read()), _bits(a))
    fv = np.asarray(f['wet'].attrs['_FillValue']).ravel()[0]
    assert (np.isnan(fv) and np.isnan(fill)) or fv == fill
    assert list(f['wet'].attrs['_Netcdf4Coordinates']) == [0, 1, 2]
    # 2. libhdf5's H5Dread, and its dimension-scale API: the scales are still attached
    if os.path.exists(LIBHDF5) and os.path.exists(LIBHDF5_HL):
        back = libhdf5_read(p, 'wet', shape, dtype, scales=((0, 'z'), (1, 'y'), (2, 'x')))
        assert np.array_equal(_bits(back), _bits(a))
    # 3. h5dump: the layout and filters it reports, and the values
    if H5DUMP is not None:
        hdr = subprocess.run([H5DUMP, '-H', '-p', '-d', '/wet', str(p)], capture_output=True, text=True)
        assert hdr.returncode == 0 and 'error' not in hdr.stderr.lower(), hdr.stderr[-2000:]
        txt = hdr.stdout
        assert 'CHUNKED' in txt and re.search(r'CHUNKED \(\s*' + r',\s*'.join(str(c) for c in chunk) + r'\s*\)', txt), txt
        assert 'PREPROCESSING SHUFFLE' in txt and 'COMPRESSION DEFLATE' in txt
        one = subprocess.run([H5DUMP, '-d', '/wet', '-w', '0', '-m', '%.17g', str(p)], capture_output=True, text=True)
        assert one.returncode == 0 and 'error' not in one.stderr.lower(), one.stderr[-2000:]
        body = re.sub(r'\([0-9,]+\):', ' ', one.stdout.split('DATA {')[1].split('}')[0])
        nums = np.array([float(t) for t in body.replace(',', ' ').split()])
        assert nums.size == a.size and np.array_equal(nums.astype(dtype), a.ravel(), equal_nan=True)


def test_more_than_64_chunks_raise_by_name(tmp_path):
    a = np.zeros((2, 64, 1), dtype=np.float32)
    packed, offs = host_chunks(a, (1, 1, 1), np.nan)
    data = h5write.ChunkedData(a.shape, a.dtype, (1, 1, 1), packed, offs)
    v = {'z': (('z',), np.arange(2.0), {}), 'y': (('y',), np.arange(64.0), {}), 'x': (('x',), np.arange(1.0), {}), 'wet': (('z', 'y', 'x'), data, {})}
    with pytest.raises(ValueError, match=r"'wet' needs 128 chunks"):
        h5write.write_netcdf4(tmp_path / 'm.nc', {'z': 2, 'y': 64, 'x': 1}, v)
    assert not (tmp_path / 'm.nc').exists()
    with pytest.raises(ValueError, match='offsets'):
        h5write.ChunkedData((4, 4), np.float32, (2, 2), b'abcd', [0, 1, 2, 4])
    with pytest.raises(ValueError, match='chunk sizes'):
        h5write.ChunkedData((4, 4), np.float32, (2, 5), b'abcd', [0, 2, 4])


def test_contiguous_files_are_written_as_before(tmp_path):
    """A file without chunked variables: the bytes of the parent commit's writer (sha256 recorded from its output)."""
    rng = np.random.default_rng(11)
    v = {'z': (('z',), np.arange(3.0), {'units': 'm'}), 'y': (('y',), np.arange(4.0), {}), 'x': (('x',), np.arange(5.0), {}),
         'wet': (('z', 'y', 'x'), rng.standard_normal((3, 4, 5)), {'units': 'm'}), 'crs': ((), np.array(-2147483647, dtype=np.int32), {'grid_mapping_name': 'latitude_longitude'})}
    p = tmp_path / 'plain.nc'
    h5write.write_netcdf4(p, {'z': 3, 'y': 4, 'x': 5}, v, {'Conventions': 'CF-1.7'})
    assert hashlib.sha256(p.read_bytes()).hexdigest() == PARENT_SHA['plain.nc']


# ---- tifflite.write(predictor=2, encoder='host') ---------------------------------------------------------------------------------
def pillow_array(path):
    try:
        from PIL import Image
    except ImportError:
        return None
    with Image.open(path) as im:
        return np.array(im)


def rasters():
    """3 x 5 int16; the DEM fixture's 569 x 558 uint16 array (read by Pillow - its LZW tiles are decoded on the GPU otherwise - or,
    without Pillow, a synthetic of that shape and type); a float32 raster whose last strip is short (100 rows of 16 per strip)."""
    rng = np.random.default_rng(21)
    dem = pillow_array(DEM)
    if dem is None:
        y, x = np.mgrid[0:569, 0:558]
        dem = (1000 + 300 * np.sin(x / 50.0) * np.cos(y / 70.0) + rng.integers(0, 3, (569, 558))).astype(np.uint16)
    assert dem.dtype == np.uint16 and dem.shape == (569, 558)
    y, x = np.mgrid[0:100, 0:1024]
    f = (2.3 + 0.2 * np.sin(x / 90.0) * np.cos(y / 31.0)).astype(np.float32)
    f[:7] = -9999.0
    return {'int16_3x5': np.array([[0, 1, -1, 32767, -32768], [5, 5, 5, 5, 5], [-3, 200, -200, 7, 0]], dtype=np.int16), 'dem_uint16': dem, 'f32_short_last_strip': f}


GT = (-118.25, 0.01 / 3, 0.0, 34.5, 0.0, -0.0025)
# sha256 of what the parent commit's tifflite.write / h5write.write_netcdf4 wrote for these calls (recorded from its output)
PARENT_SHA = {
    ('int16_3x5', None): '41e1395b466fb75a894ce0eba57b1d9467d13515a419a8f56fc85a7a337f4028',
    ('int16_3x5', 'deflate'): 'f85de3b2cff8017c8e50655ebaea7055d3fae7d522d36efa9974c7a1a65c0e04',
    ('f32_short_last_strip', None): 'cc0c9a148a48c64e265986820993cc731f8f7a0e4430c2cc963ff710b3a4caa9',
    ('f32_short_last_strip', 'deflate'): '9564bbc7375259b0ab65123733b7dd49523f7039d2bc6b6506c1cc83ade22058',
    'plain.nc': 'cd1ff8e2cd1ac6d5012afd7723bbe57bd7bc46198df28bd651e72bc99386aba5',
}


@pytest.mark.parametrize('name', ['int16_3x5', 'dem_uint16', 'f32_short_last_strip'])
def test_predictor_2_on_the_host_encoder(tmp_path, name):
    a = rasters()[name]
    p = tmp_path / 'p2.tif'
    tifflite.write(p, a, transform=GT, crs=4326, nodata=-9999.0, compress='deflate', predictor=2, encoder='host')
    info = tifflite.TiffInfo(p)
    assert info.predictor == 2 and info.compression == 8
    if name == 'f32_short_last_strip':
        assert len(info.offsets) == 7 and info.tile_h == 16 and info.seg_rows(6) == 4
    back, prof = tifflite.read(p)
    assert back.dtype == a.dtype and np.array_equal(_bits(back), _bits(a))
    assert prof['transform'] == GT and prof['crs'] == 4326 and prof['nodata'] == -9999.0
    got = pillow_array(p)
    if got is not None:
        assert got.shape == a.shape and np.array_equal(got, a)          # (Pillow widens int16 to its 32-bit integer mode: values compare)
    # the same pixels and tags as the default call, in fewer bytes for the smooth rasters
    q = tmp_path / 'p1.tif'
    tifflite.write(q, a, transform=GT, crs=4326, nodata=-9999.0, compress='deflate')
    plain = tifflite.TiffInfo(q)
    assert plain.predictor == 1 and plain.profile()['transform'] == prof['transform']
    if name != 'int16_3x5':
        assert p.stat().st_size < q.stat().st_size


@pytest.mark.parametrize('name', ['int16_3x5', 'f32_short_last_strip'])
@pytest.mark.parametrize('compress', [None, 'deflate'])
def test_default_call_writes_the_bytes_of_the_parent_commit(tmp_path, name, compress):
    a = rasters()[name]
    p = tmp_path / 'd.tif'
    tifflite.write(p, a, transform=GT, crs=4326, nodata=-9999.0, compress=compress)
    assert hashlib.sha256(p.read_bytes()).hexdigest() == PARENT_SHA[(name, compress)]


def test_writer_argument_checks(tmp_path):
    a = np.zeros((3, 4), dtype=np.float32)
    with pytest.raises(ValueError, match='predictor'):
        tifflite.write(tmp_path / 'x.tif', a, compress='deflate', predictor=3)
    with pytest.raises(ValueError, match='encoder'):
        tifflite.write(tmp_path / 'x.tif', a, compress='deflate', encoder='gpu')
    with pytest.raises(ValueError, match="compress='deflate'"):
        tifflite.write(tmp_path / 'x.tif', a, predictor=2)
    try:
        import torch
        gpu = torch.cuda.is_available()
    except ImportError:
        gpu = False
    if not gpu:
        with pytest.raises((RuntimeError, ImportError), match='GPU|torch'):
            tifflite.write(tmp_path / 'x.tif', a, compress='deflate', encoder='device')


# ---- the bound ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 32767, 32768, 32769, 10 ** 6, 2 ** 31])
def test_bound(n):
    from raider_amd import deflate
    b = deflate.bound(n)
    assert n + 6 < b <= n + n // 2048 + 32
    assert b == n + 5 * -(-n // 32768) + 6             # a stored block per 32 KiB sub-block, the zlib header and the Adler-32


def test_delay_cube_to_netcdf_without_compress_writes_the_bytes_of_the_parent_commit(tmp_path):
    from raider_amd.delay import DelayCube
    rng = np.random.default_rng(9)
    shape = (4, 10, 11)
    wet = rng.uniform(0.0, 0.3, shape); hydro = rng.uniform(1.8, 2.4, shape)
    wet[0, 1, 2] = np.nan; hydro[-1, -1, -1] = np.nan
    v = {'wet': wet, 'hydro': hydro, 'z': np.linspace(0.0, 3000.0, 4), 'y': np.linspace(34.0, 33.0, 10), 'x': np.linspace(-118.0, -117.0, 11)}
    cube = DelayCube(v, {'description': 'RAiDER geo cube - ray tracing', 'model_times_used': '2020-01-03T00:00:00', 'reference_time': '2020-01-03T00:00:00',
                         'interpolation_method': 'none', 'source': 'test'})
    for kw in ({}, {'compress': False}):
        p = tmp_path / 'cube.nc'
        cube.to_netcdf(p, **kw)
        assert hashlib.sha256(p.read_bytes()).hexdigest() == '8b5dc27b2dd499189b6c063e06bf00f63328b170500b8db003a88948ea389c76'
    with pytest.raises(ValueError, match='NETCDF4'):
        cube.to_netcdf(tmp_path / 'c3.nc', format='NETCDF3_64BIT', compress=True)


# ---- the encoder's sub-block function on the CPU, under sanitizers --------------------------------------------------------------
def test_deflate_subblock_is_clean_under_sanitizers_and_zlib_reads_its_streams(tmp_path):
    """tools/probes/deflate_host_check.cpp - deflate_subblock() of csrc/deflate_kernels.h, everything a wave of the encode kernel does,
    with 64 threads as the lanes - built for the CPU with AddressSanitizer and UBSan, input and slots in heap blocks of exactly their
    sizes at every source alignment.  It must exit clean, every stream must decode to its input under zlib (which checks the
    Adler-32) and stay within the bound.  A stand-alone program: nothing with a sanitizer is loaded into this process, nothing runs
    on a GPU.  Inputs are kept to a few sub-blocks: the emulation pays two barriers per wave operation."""
    import struct
    from raider_amd import deflate
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler to build the probe with')
    exe = tmp_path / 'deflate_host_check'
    subprocess.run([cxx, '-O1', '-g', '-std=c++17', '-pthread', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
                    str(REPO / 'tools' / 'probes' / 'deflate_host_check.cpp'), '-o', str(exe)], check=True)
    rng = np.random.default_rng(4)
    y, x = np.mgrid[0:24, 0:256]
    d = (np.sin(x / 40.0) * np.cos(y / 55.0) * 2.3 + 2.5).astype(np.float32).view(np.uint32).copy()
    d[:, 1:] = d[:, 1:] - d[:, :-1]
    far = rng.integers(0, 256, 2600, dtype=np.uint8); far[2200:2500] = far[:300]
    cases = [b'\x00', b'ab', bytes(63), bytes(64), b'\xff' * 65, (np.arange(700) % 3).astype(np.uint8).tobytes(), (np.arange(1000) % 259).astype(np.uint8).tobytes(),
             far.tobytes(), rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(), b'the wet and the hydrostatic delay of the troposphere ' * 40,
             d.tobytes(), bytes(32769), b'\xff' * 40000]
    (tmp_path / 'in.bin').write_bytes(struct.pack('<I', len(cases)) + b''.join(struct.pack('<I', len(c)) + c for c in cases))
    r = subprocess.run([str(exe), str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-3000:]
    raw, pos = (tmp_path / 'out.bin').read_bytes(), 0
    for i, c in enumerate(cases):
        n, = struct.unpack_from('<I', raw, pos)
        z = raw[pos + 4:pos + 4 + n]; pos += 4 + n
        assert z[:2] == b'\x78\x01' and zlib.decompress(z) == c, i
        assert n <= deflate.bound(len(c)), (i, n)
    assert pos == len(raw)
