"""The device deflate encoder (rdr_deflate_encode), the chunk cutter (rdr_h5_chunks) and the writers built on them.

Every stream is decoded by zlib itself, which also checks the Adler-32.  The size conditions are derived, not measured: the bound is
the stored form (5 bytes per 32 KiB sub-block + 6), 258 zero bytes cost one 13-bit token.  The ratio test compares against zlib's own
fixed-table encoder (Z_FIXED, level 1) in the same 32 KiB sub-blocks; its margin is the excess recorded in
profiles/r22_deflate.json plus 0.05 for the matcher's input dependence."""
import ctypes as C
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 32768                      # the encoder's sub-block


@pytest.fixture(scope='module')
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch


def _text(n):
    words = [b'delay', b'troposphere', b'wet', b'hydrostatic', b'ray', b'cube', b'level', b'the', b'of', b'zenith', b'model', b'height']
    rng = np.random.default_rng(7)
    out = b' '.join(words[i] for i in rng.integers(0, len(words), n // 4 + 8))
    return out[:n]


def _contents():
    rng = np.random.default_rng(0)
    far = rng.integers(0, 256, 33000, dtype=np.uint8)
    far[32000:32300] = far[:300]
    straddle = rng.integers(0, 256, 1000, dtype=np.uint8)
    straddle[150:250] = straddle[20:120]                  # the copy starts in step 2 (positions 128 .. 191) and ends in step 3
    cases = {'ff': b'\xff' * 70000,
             'period3': (np.arange(40000) % 3).astype(np.uint8).tobytes(),
             'period259': (np.arange(40000) % 259).astype(np.uint8).tobytes(),
             'far': far.tobytes(), 'straddle': straddle.tobytes(),
             'text': _text(70001), 'random': rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()}
    for n in (1, 2, 63, 64, 65, B - 1, B, B + 1, 2 * B + 3):
        cases[f'zeros{n}'] = bytes(n)
        cases[f'text{n}'] = _text(n)
        cases[f'random{n}'] = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    return cases


def _encode_all(cases, torch=None):
    """Every case as one segment of ONE call, at odd offsets; {name: stream}."""
    from raider_amd import deflate
    parts, offs, pos = [], [], 1
    for c in cases.values():
        offs.append(pos)
        parts.append(c)
        pos += len(c) + (1 if len(c) % 2 == 0 else 2)         # the next offset is odd again
    buf = np.full(pos, 0x5A, dtype=np.uint8)
    for o, c in zip(offs, parts):
        buf[o:o + len(c)] = np.frombuffer(c, dtype=np.uint8)
    sizes = [len(c) for c in parts]
    src = torch.from_numpy(buf).cuda() if torch is not None else buf
    packed, oo = deflate.deflate_segments(src, offs, sizes)
    if torch is not None:
        assert packed.is_cuda
        packed = packed.cpu().numpy()
    assert oo[0] == 0 and oo[-1] == packed.size
    return {k: packed[oo[i]:oo[i + 1]].tobytes() for i, k in enumerate(cases)}


@pytest.fixture(scope='module')
def cases():
    return _contents()


@pytest.fixture(scope='module')
def streams(torch_cuda, cases):
    return _encode_all(cases)


def test_round_trip_host_arrays(cases, streams):
    from raider_amd import deflate
    for k, c in cases.items():
        z = streams[k]
        assert z[:2] == b'\x78\x01', k
        assert zlib.decompress(z) == c, k
        assert len(z) <= deflate.bound(len(c)), (k, len(z), deflate.bound(len(c)))


def test_round_trip_device_tensors_gives_the_same_bytes(torch_cuda, cases, streams):
    dev = _encode_all(cases, torch_cuda)
    assert dev == streams


def test_single_segment(torch_cuda, cases):
    from raider_amd import deflate
    c = np.frombuffer(cases['text'], dtype=np.uint8)
    packed, oo = deflate.deflate_segments(c, [0], [c.size])
    assert list(oo) == [0, packed.size]
    assert zlib.decompress(packed.tobytes()) == cases['text']


def test_derived_sizes(cases, streams):
    from raider_amd import deflate
    z = streams[f'zeros{2 * B + 3}']                       # 64 KiB of zeros (and 3): 13 bits per 258 bytes plus framing
    assert len(z) <= 1024, len(z)
    for k in ('random', f'random{B}', f'random{2 * B + 3}'):
        n = len(cases[k])
        assert len(streams[k]) <= n + 5 * -(-n // B) + 6 == deflate.bound(n), k
    assert len(streams['text']) < len(cases['text']) // 2


def _mixed_batch():
    rng = np.random.default_rng(3)
    text = np.frombuffer(_text(200000), dtype=np.uint8)
    buf = np.concatenate([text, rng.integers(0, 4, 150000).astype(np.uint8), np.zeros(50001, dtype=np.uint8)])
    sizes = rng.choice([1, 2, 63, 64, 65, 257, 1000, 4095, 5001], 300)
    sizes[::37] = B + 1
    offs = rng.integers(0, buf.size - sizes.max(), 300) | 1
    return buf, offs, sizes


def test_batch_of_300_is_deterministic_and_stays_inside_its_output(torch_cuda):
    """Raw ABI with a guard pattern behind the bytes the call reports, for a host buffer and for a device tensor."""
    torch = torch_cuda
    from raider_amd import _lib as L, deflate
    buf, offs, sizes = _mixed_batch()
    offs = np.ascontiguousarray(offs, dtype=np.int64); sizes = np.ascontiguousarray(sizes, dtype=np.int64)
    cap = sum(deflate.bound(int(s)) for s in sizes)
    ctx = L.Context.default()
    runs = []
    for loc in (L.RDR_HOST, L.RDR_DEVICE, L.RDR_HOST):
        out = np.full(cap + 256, 0xA5, dtype=np.uint8)
        oo = np.zeros(301, dtype=np.int64)
        if loc == L.RDR_DEVICE:
            s, o = torch.from_numpy(buf).cuda(), torch.from_numpy(out).cuda()
            torch.cuda.synchronize()
            L.check(ctx.lib.rdr_deflate_encode(ctx.handle, L.ptr(s), buf.size, L.ptr(offs), L.ptr(sizes), 300, L.ptr(o), cap, L.ptr(oo), loc), ctx.handle)
            out = o.cpu().numpy()
        else:
            L.check(ctx.lib.rdr_deflate_encode(ctx.handle, L.ptr(buf), buf.size, L.ptr(offs), L.ptr(sizes), 300, L.ptr(out), cap, L.ptr(oo), loc), ctx.handle)
        total = int(oo[-1])
        assert total <= cap
        assert np.all(out[total:] == 0xA5)
        for i in range(300):
            assert zlib.decompress(out[oo[i]:oo[i + 1]].tobytes()) == buf[offs[i]:offs[i] + sizes[i]].tobytes(), i
            assert oo[i + 1] - oo[i] <= deflate.bound(int(sizes[i]))
        runs.append(out[:total].tobytes())
    assert runs[0] == runs[1] == runs[2]


def _zfixed_size(data):
    """zlib's fixed-table encoder at level 1 over the same independent sub-blocks, each stored when that is smaller."""
    total = 6
    for o in range(0, len(data), B):
        part = data[o:o + B]
        co = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
        total += min(len(co.compress(part) + co.flush(zlib.Z_SYNC_FLUSH)), len(part) + 5)
    return total


def _synthetic_cube(dtype):
    z, y, x = np.meshgrid(np.arange(20.0), np.arange(96.0), np.arange(96.0), indexing='ij')
    return (2.3 * np.exp(-z / 7.0) * (1.0 + 0.1 * np.sin(x / 17.0) * np.cos(y / 23.0))).astype(dtype)


def _synthetic_raster():
    y, x = np.mgrid[0:256, 0:256]
    f = (np.sin(x / 40.0) * np.cos(y / 55.0) * 2.3 + 2.5).astype(np.float32)
    f[:16] = 0.0                                           # the no-data band
    return f


# the encoder's excess over zlib Z_FIXED measured on the GPU on exactly these inputs (profiles/r22_deflate.json, ratio_test_inputs:
# 0.0026, 0.0167, 0.0283) + 0.05 for the matcher's input dependence
RATIO_MARGIN = {'cube_f32': 0.0526, 'cube_f64': 0.0667, 'raster_p2': 0.0783}


def ratio_segments(which):
    """The ratio test's inputs as byte strings, one per segment: the shuffled (20, 32, 32) chunks of a (20, 96, 96) synthetic cube in f32
    / f64, or the predictor-2 strips (64 KiB) of a 256 x 256 f32 raster with 16 no-data rows.  (tools/bench_deflate.py records the
    encoder's excess on exactly these.)"""
    from raider_amd import deflate
    if which == 'raster_p2':
        d = _synthetic_raster().view(np.uint32).copy()
        d[:, 1:] = d[:, 1:] - d[:, :-1]
        rows = (1 << 16) // (256 * 4)
        return [d[r:r + rows].tobytes() for r in range(0, 256, rows)]
    a = _synthetic_cube(np.float32 if which == 'cube_f32' else np.float64)
    raw = deflate.h5_chunks_host(a, (20, 32, 32), np.nan, shuffle=True)
    cb = raw.size // 9
    return [raw[k * cb:(k + 1) * cb].tobytes() for k in range(9)]


@pytest.mark.parametrize('which', ['cube_f32', 'cube_f64', 'raster_p2'])
def test_ratio_against_zlib_fixed(torch_cuda, which):
    from raider_amd import deflate
    segs = ratio_segments(which)
    buf = np.frombuffer(b''.join(segs), dtype=np.uint8)
    sizes = [len(s) for s in segs]
    packed, oo = deflate.deflate_segments(buf, np.cumsum([0] + sizes[:-1]), sizes)
    for i, s in enumerate(segs):
        assert zlib.decompress(packed[oo[i]:oo[i + 1]].tobytes()) == s
    ref = sum(_zfixed_size(s) for s in segs)
    z1 = sum(len(zlib.compress(s, 1)) for s in segs)
    print(f'{which}: input {buf.size} device {packed.size} zlib-fixed {ref} zlib-1 {z1} excess {packed.size / ref - 1:.4f}')
    assert packed.size <= ref * (1.0 + RATIO_MARGIN[which]), (packed.size, ref)


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('shuffle', [False, True])
def test_h5_chunks_against_numpy(torch_cuda, dtype, shuffle):
    from raider_amd import deflate
    a = np.random.default_rng(1).standard_normal((7, 10, 11)).astype(dtype)
    want = deflate.h5_chunks_host(a, (7, 3, 3), np.nan, shuffle)
    assert want.size == 16 * 63 * a.itemsize
    got = deflate.h5_chunks(a, (7, 3, 3), np.nan, shuffle)
    assert got.tobytes() == want.tobytes()
    got_dev = deflate.h5_chunks(torch_cuda.from_numpy(a).cuda(), (7, 3, 3), np.nan, shuffle)
    assert got_dev.cpu().numpy().tobytes() == want.tobytes()


def test_abi_errors_write_nothing(torch_cuda):
    from raider_amd import _lib as L, deflate
    ctx = L.Context.default()
    src = np.arange(1000, dtype=np.uint8)
    cap = deflate.bound(1000)

    def call(src_p, nbytes, offs, sizes, out_cap=None, out_null=False, oo_null=False):
        offs = None if offs is None else np.array(offs, dtype=np.int64)
        sizes = None if sizes is None else np.array(sizes, dtype=np.int64)
        n = 1 if sizes is None else sizes.size
        out = np.full(4096, 0xA5, dtype=np.uint8)
        oo = np.full(n + 1, -7, dtype=np.int64)
        rc = ctx.lib.rdr_deflate_encode(ctx.handle, L.ptr(src_p), nbytes, L.ptr(offs), L.ptr(sizes), n, None if out_null else L.ptr(out),
                                        n * cap if out_cap is None else out_cap, None if oo_null else L.ptr(oo), L.RDR_HOST)
        assert rc == L.RDR_ERR_INVALID
        assert np.all(out == 0xA5) and np.all(oo == -7)

    call(None, 1000, [0], [1000])
    call(src, 1000, None, [1000])
    call(src, 1000, [0], None)
    call(src, 1000, [0], [1000], out_null=True)
    call(src, 1000, [0], [1000], oo_null=True)
    call(src, 1000, [1], [1000])                           # one byte beyond src
    call(src, 1000, [-1], [10])
    call(src, 1000, [1001], [1])
    call(src, 1000, [0], [0])
    call(src, 1000, [0, 10], [10, -3])
    call(src, 1000, [0], [1000], out_cap=cap - 1)
    sh, ck, fv = np.array([4, 4], dtype=np.int64), np.array([2, 0], dtype=np.int64), np.zeros(1, dtype=np.float32)
    a, out = np.zeros((4, 4), dtype=np.float32), np.full(64, 0xA5, dtype=np.uint8)
    assert ctx.lib.rdr_h5_chunks(ctx.handle, L.ptr(a), 4, 2, L.ptr(sh), L.ptr(ck), L.ptr(fv), 1, L.ptr(out), L.RDR_HOST) == L.RDR_ERR_INVALID
    assert ctx.lib.rdr_h5_chunks(ctx.handle, L.ptr(a), 3, 2, L.ptr(sh), L.ptr(sh), L.ptr(fv), 1, L.ptr(out), L.RDR_HOST) == L.RDR_ERR_INVALID
    assert ctx.lib.rdr_h5_chunks(ctx.handle, L.ptr(a), 4, 5, L.ptr(sh), L.ptr(sh), L.ptr(fv), 1, L.ptr(out), L.RDR_HOST) == L.RDR_ERR_INVALID
    assert np.all(out == 0xA5)


# ---- end to end: the writers on top of the encoder -----------------------------------------------------------------------------------
def _delay_cube(shape=(4, 10, 11)):
    from raider_amd.delay import DelayCube
    rng = np.random.default_rng(9)
    nz, ny, nx = shape
    wet = rng.uniform(0.0, 0.3, shape); hydro = rng.uniform(1.8, 2.4, shape)
    wet[0, 1, 2] = np.nan; hydro[-1, -1, -1] = np.nan
    v = {'wet': wet, 'hydro': hydro, 'z': np.linspace(0.0, 3000.0, nz), 'y': np.linspace(34.0, 33.0, ny), 'x': np.linspace(-118.0, -117.0, nx)}
    return DelayCube(v, {'description': 'RAiDER geo cube - ray tracing', 'model_times_used': '2020-01-03T00:00:00', 'reference_time': '2020-01-03T00:00:00',
                         'interpolation_method': 'none', 'source': 'test'})


def _check_file(path, want, h5names=None):
    """Every variable of `want` {name: array} read back bit for bit by h5lite and, where libhdf5 is present, by H5Dread."""
    import os
    from raider_amd import h5lite
    from tests.test_deflate_host import LIBHDF5, LIBHDF5_HL, _bits, libhdf5_read
    f = h5lite.File(path)
    for name, a in want.items():
        got = f[name].read()
        assert got.dtype == a.dtype and np.array_equal(_bits(got), _bits(a)), name
        if os.path.exists(LIBHDF5) and os.path.exists(LIBHDF5_HL) and a.ndim == 3:
            back = libhdf5_read(path, name, a.shape, a.dtype, scales=tuple(enumerate(h5names)) if h5names else ())
            assert np.array_equal(_bits(back), _bits(a)), name
    return f


def test_delay_cube_to_netcdf_compressed(torch_cuda, tmp_path):
    from raider_amd import h5lite
    cube = _delay_cube()
    plain = tmp_path / 'plain.nc'; packed = tmp_path / 'packed.nc'; again = tmp_path / 'again.nc'
    cube.to_netcdf(plain)
    cube.to_netcdf(again, compress=False)
    assert plain.read_bytes() == again.read_bytes()
    cube.to_netcdf(packed, compress=True)
    want = {k: np.asarray(cube.variables[k], dtype=np.float64) for k in ('wet', 'hydro', 'z', 'y', 'x')}
    f = _check_file(packed, want, h5names=('z', 'y', 'x'))
    g = h5lite.File(plain)
    for name in ('wet', 'hydro'):
        assert dict(f[name].attrs.items()).keys() == dict(g[name].attrs.items()).keys()
        assert f[name].attrs['units'] == 'm' and np.isnan(f[name].attrs['_FillValue']).all()
    assert dict(f.attrs.items()) == dict(g.attrs.items())
    # the default chunks are the GUNW rule; others can be asked for, a variable beyond 64 chunks is refused by name
    cube.to_netcdf(again, compress=True, chunks=(2, 4, 11))
    _check_file(again, want)
    with pytest.raises(ValueError, match='chunks'):
        cube.to_netcdf(again, compress=True, chunks=(1, 1, 1))
    with pytest.raises(ValueError, match='NETCDF4'):
        cube.to_netcdf(again, format='NETCDF3_64BIT', compress=True)


def test_delay_cube_on_the_device_and_a_compressible_size(torch_cuda, tmp_path):
    """A smooth cube held as device tensors: the compressed file is smaller, and reads back bit for bit."""
    from raider_amd.delay import DelayCube
    z, y, x = np.meshgrid(np.linspace(0, 9000, 12), np.linspace(34, 33, 50), np.linspace(-118, -117, 61), indexing='ij')
    wet = 0.3 * np.exp(-z / 2000.0) * (1 + 0.05 * np.sin(8 * x) * np.cos(9 * y)); hydro = 2.3 * np.exp(-z / 8000.0) + 0 * x
    v = {'wet': torch_cuda.from_numpy(wet).cuda(), 'hydro': torch_cuda.from_numpy(hydro).cuda(), 'z': z[:, 0, 0], 'y': y[0, :, 0], 'x': x[0, 0, :]}
    cube = DelayCube(v, {'description': 'RAiDER geo cube - ray tracing'})
    p, q = tmp_path / 'dev.nc', tmp_path / 'plain.nc'
    cube.to_netcdf(p, compress=True)
    cube.to_netcdf(q)
    _check_file(p, {'wet': wet, 'hydro': hydro}, h5names=('z', 'y', 'x'))
    assert p.stat().st_size < 0.8 * q.stat().st_size, (p.stat().st_size, q.stat().st_size)


def test_gunw_write_delays_slc(torch_cuda, tmp_path):
    import datetime as dt
    from raider_amd import gunw
    a, b = _delay_cube(), _delay_cube()
    b.variables['wet'] = b.variables['wet'] * 1.1
    ds = gunw.compute_delays_slc({dt.datetime(2020, 1, 3): a, dt.datetime(2020, 1, 15): b}, 0.0556)
    p = tmp_path / 'slc.nc'
    gunw.write_delays_slc(ds, p)
    want = {k: np.asarray(ds.variables[k], dtype=np.float32) for k in ds.variables}
    assert sorted(want) == sorted(['heightsMeta', 'latitudeMeta', 'longitudeMeta'] + [f'{k}_{n}' for k in ('reference', 'secondary') for n in gunw.TROPO_NAMES])
    f = _check_file(p, want, h5names=tuple(gunw.DIM_NAMES))
    lay = f['reference_troposphereWet']
    assert lay.attrs['units'] == 'radians' and lay.attrs['long_name'] == 'troposphereWet' and float(np.asarray(lay.attrs['_FillValue']).ravel()[0]) == 0.0
    assert lay.attrs['scene_center_time'] == '2020-01-03T00:00:00' and lay.read().dtype == np.float32


@pytest.mark.parametrize('name', ['int16_3x5', 'dem_uint16', 'f32_short_last_strip'])
def test_tifflite_write_on_the_device(torch_cuda, tmp_path, name):
    from raider_amd import tifflite
    from tests.test_deflate_host import GT, _bits, pillow_array, rasters
    a = rasters()[name]
    p = tmp_path / 'dev.tif'
    src = torch_cuda.from_numpy(a).cuda() if name == 'f32_short_last_strip' else a          # a device tensor is taken as it is
    tifflite.write(p, src, transform=GT, crs=4326, nodata=-9999.0, compress='deflate', predictor=2, encoder='device')
    info = tifflite.TiffInfo(p)
    assert info.predictor == 2 and info.compression == 8
    back, prof = tifflite.read(p)
    assert back.dtype == a.dtype and np.array_equal(_bits(back), _bits(a))
    assert prof['transform'] == GT and prof['crs'] == 4326 and prof['nodata'] == -9999.0
    dev, _ = tifflite.read(p, device='cuda')
    assert dev.is_cuda and np.array_equal(_bits(dev.cpu().numpy()), _bits(a))
    got = pillow_array(p)
    if got is not None:
        assert got.shape == a.shape and np.array_equal(got, a)
    # the host encoder writes the same tags and pixels; without a predictor the device encoder is served too
    q = tmp_path / 'host.tif'
    tifflite.write(q, a, transform=GT, crs=4326, nodata=-9999.0, compress='deflate', predictor=2, encoder='host')
    hinfo = tifflite.TiffInfo(q)
    assert (hinfo.tile_h, len(hinfo.offsets), hinfo.profile()['transform']) == (info.tile_h, len(info.offsets), prof['transform'])
    tifflite.write(q, a, compress='deflate', encoder='device')
    assert tifflite.TiffInfo(q).predictor == 1 and np.array_equal(_bits(tifflite.read(q)[0]), _bits(a))


def test_write_delays_takes_the_device_route_and_gives_the_host_routes_pixels(torch_cuda, tmp_path, monkeypatch):
    from raider_amd import tifflite, utilFcns
    rng = np.random.default_rng(2)
    y, x = np.mgrid[0:70, 0:300]
    w = 0.2 + 0.1 * np.sin(x / 40.0) * np.cos(y / 9.0) + rng.normal(0, 1e-4, (70, 300)); h = 2.1 + 0.001 * y + 0 * x
    w[2, 3] = np.nan; w[60:] = np.nan
    aoi = type('R', (), dict(type=lambda self: 'radar_rasters', projection=lambda self: 'EPSG:4326', geotransform=lambda self: (-118.0, 0.01, 0.0, 34.0, 0.0, -0.01)))()
    utilFcns.writeDelays(aoi, w.copy(), h.copy(), tmp_path / 'wet.tif', tmp_path / 'hydro.tif', outformat='GTiff', ndv=-9999.0)
    monkeypatch.setattr(utilFcns, '_gpu_visible', lambda: False)
    utilFcns.writeDelays(aoi, w.copy(), h.copy(), tmp_path / 'wet_host.tif', tmp_path / 'hydro_host.tif', outformat='GTiff', ndv=-9999.0)
    for name in ('wet', 'hydro'):
        d, hst = tifflite.TiffInfo(tmp_path / f'{name}.tif'), tifflite.TiffInfo(tmp_path / f'{name}_host.tif')
        assert (d.predictor, hst.predictor) == (2, 1) and d.compression == hst.compression == 8 and len(d.offsets) == len(hst.offsets) == 2
        a, pa = utilFcns.rio_open(tmp_path / f'{name}.tif')
        b, pb = utilFcns.rio_open(tmp_path / f'{name}_host.tif')
        assert a.dtype == np.float32 and a.tobytes() == b.tobytes()
        assert {k: pa[k] for k in ('transform', 'crs', 'nodata', 'width', 'height', 'dtype')} == {k: pb[k] for k in ('transform', 'crs', 'nodata', 'width', 'height', 'dtype')}
    assert utilFcns.rio_open(tmp_path / 'wet.tif')[0][2, 3] == -9999.0
