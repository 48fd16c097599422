"""GPU: zlib streams decoded on the device - rdr_inflate_decode (one wave per stream, the history a ring in LDS, lane 0 decoding tokens
through inflate_next) and rdr_h5_unchunk - through raider_amd.deflate.inflate_segments, the deflate route of tifflite.read and
h5lite.Dataset.read_device.  The judge is zlib: status == 0 exactly when zlib.decompress accepts a stream and its output fits the
slot, and then the bytes are zlib's.  The damaged set is the one tools/probes/inflate_host_check ran on the CPU under the sanitizers
(tests/test_inflate_host.py): a robustness check of streams whose handling is already known, not a search for a fault."""
import struct
import zlib

import numpy as np
import pytest

from raider_amd import _lib as L
from raider_amd import deflate, h5lite, h5write, tifflite
from raider_amd.deflate import inflate_segments
from tests import deflate_craft as D
from tests import tiff_codec as T

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

SENTINEL = 0xA5


def _dev():
    return torch.device('cuda', 0)


def _pack(streams, rng, first=1):
    """One buffer holding the streams at odd byte offsets with gaps of 1 .. 7 sentinel bytes between them."""
    parts, offs, pos = [bytes([SENTINEL]) * first], [], first
    for s in streams:
        offs.append(pos)
        gap = int(rng.integers(1, 8))
        if (pos + len(s) + gap) % 2 == 0:
            gap += 1                                             # the next stream starts at an odd offset
        parts += [bytes(s), bytes([SENTINEL]) * gap]
        pos += len(s) + gap
    return np.frombuffer(b''.join(parts), dtype=np.uint8), np.array(offs, dtype=np.int64)


def _decode(streams, caps, stride, rng, tensor=True):
    """(slots as a (n, stride) NumPy array, status, produced) of one call; slots pre-filled with the sentinel."""
    buf, offs = _pack(streams, rng)
    sizes = np.array([len(s) for s in streams], dtype=np.int64)
    n = len(streams)
    if tensor:
        out = torch.full((n * stride,), SENTINEL, dtype=torch.uint8, device=_dev())
        out, status, produced = inflate_segments(torch.from_numpy(buf.copy()).to(_dev()), offs, sizes, caps, out_stride=stride, out=out)
        return out.cpu().numpy().reshape(n, stride), status.cpu().numpy(), produced.cpu().numpy()
    out = np.full(n * stride, SENTINEL, dtype=np.uint8)
    out, status, produced = inflate_segments(buf, offs, sizes, caps, out_stride=stride, out=out)
    return out.reshape(n, stride), status, produced


def _check(slots, status, produced, streams, caps, labels):
    """The status rule, slot by slot; returns how many streams zlib accepted."""
    ok = 0
    for k, s in enumerate(streams):
        want = D.judge(s, int(caps[k]))
        if want is None:
            assert 1 <= status[k] <= 4, (labels[k], status[k])
            assert 0 <= produced[k] <= caps[k]
        else:
            ok += 1
            assert status[k] == 0 and produced[k] == len(want), (labels[k], status[k], produced[k], len(want))
            assert slots[k, :len(want)].tobytes() == want, labels[k]
            assert np.all(slots[k, len(want):] == SENTINEL), labels[k]
        assert np.all(slots[k, int(caps[k]):] == SENTINEL), labels[k]      # nothing beyond the slot, whatever the stream is
    return ok


@pytest.mark.parametrize('tensor', [True, False])
def test_corpus_in_one_call(tensor):
    names, streams = zip(*D.corpus())
    want = [zlib.decompress(s) for s in streams]
    caps = np.array([len(w) for w in want], dtype=np.int64)
    stride = (int(caps.max()) + 37 + 15) // 16 * 16              # a tail of sentinel bytes behind the largest slot too
    slots, status, produced = _decode(streams, caps, stride, np.random.default_rng(21), tensor)
    assert _check(slots, status, produced, streams, caps, names) == len(streams)
    assert 'crafted-far' in names and 'dyn-single-distance' in names and 'stored-65535' in names


def test_many_unequal_segments():
    rng = np.random.default_rng(22)
    base = np.frombuffer(D.delay_like(12000, seed=5) + D.text_like(20000, seed=6), dtype=np.uint8)
    sizes = np.concatenate([[1, 2, 3, 40000], rng.choice(np.arange(4, 40000), 296, replace=False)])
    rng.shuffle(sizes)
    assert sizes.size == 300 and sizes.min() == 1 and sizes.max() == 40000
    data = [base[int(o):int(o) + int(n)].tobytes() for o, n in zip(rng.integers(0, base.size - 40000, 300), sizes)]
    streams = [zlib.compress(d, int(rng.integers(1, 10))) for d in data]
    slots, status, produced = _decode(streams, sizes.astype(np.int64), 40000 + 16, rng)
    assert np.all(status == 0) and np.array_equal(produced, sizes)
    for k, d in enumerate(data):
        assert slots[k, :len(d)].tobytes() == d
        assert np.all(slots[k, len(d):] == SENTINEL)


def test_slot_size():
    c = dict(D.corpus())
    streams = [c['text-l6'], c['text-l6'], c['zeros-l9'], c['zeros-l9'], c['random-l0'], c['random-l0'], c['empty-l6'], c['one-l6'], c['one-l6']]
    full = [len(zlib.decompress(s)) for s in streams]
    caps = np.array([full[0] - 1, full[1], full[2] - 1, full[3], full[4] - 1, full[5], 0, 0, 1], dtype=np.int64)
    slots, status, produced = _decode(streams, caps, 100000 + 64, np.random.default_rng(23))
    assert list(status) == [2, 0, 2, 0, 2, 0, 0, 2, 0], status
    _check(slots, status, produced, streams, caps, list(range(len(streams))))


@pytest.mark.parametrize('tables', ['fixed', 'dynamic'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_round_trip_through_the_device_encoder(tables, dtype):
    raw = np.frombuffer(D.delay_like(100 * 1024 // np.dtype(dtype).itemsize, dtype=dtype, seed=8), dtype=np.uint8)
    src = torch.from_numpy(raw.copy()).to(_dev())
    cuts = np.array([0, 1, 33000, 33001, 70001, raw.size], dtype=np.int64)          # unequal ranges, one of a single byte
    packed, oo = deflate.deflate_segments(src, cuts[:-1], np.diff(cuts), tables=tables)
    sizes = np.diff(cuts)
    out, status, produced = inflate_segments(packed, oo[:-1], np.diff(oo), sizes)
    stride = out.numel() // sizes.size
    assert np.all(status.cpu().numpy() == 0) and np.array_equal(produced.cpu().numpy(), sizes)
    back = out.cpu().numpy().reshape(sizes.size, stride)
    for k in range(sizes.size):
        assert np.array_equal(back[k, :sizes[k]], raw[cuts[k]:cuts[k + 1]])
        assert zlib.decompress(packed[int(oo[k]):int(oo[k + 1])].cpu().numpy().tobytes()) == raw[cuts[k]:cuts[k + 1]].tobytes()


def test_damaged_streams_follow_zlib():
    """Every damaged variant sits between two valid streams of the same call, which must decode as if it were not there."""
    corpus = D.corpus()
    neighbour = dict(corpus)['syncflush']
    nb = zlib.decompress(neighbour)
    rng = np.random.default_rng(24)
    groups = [(name, D.damaged(name, s)) for name, s in corpus] + [('specials', D.specials())]
    accepted = rejected = 0
    for name, variants in groups:
        labels, streams = [], []
        for label, s in variants:
            labels += ['neighbour', label]
            streams += [neighbour, s]
        labels.append('neighbour'); streams.append(neighbour)
        good = [D.judge(s) for s in streams]
        caps = np.array([len(g) if g is not None else 70000 for g in good], dtype=np.int64)
        stride = (int(caps.max()) + 15) // 16 * 16 + 16
        slots, status, produced = _decode(streams, caps, stride, rng)
        ok = _check(slots, status, produced, streams, caps, labels)
        n_nb = (len(streams) + 1) // 2
        assert np.all(status[0::2] == 0) and all(slots[k, :len(nb)].tobytes() == nb for k in range(0, len(streams), 2))
        accepted += ok - n_nb
        rejected += len(streams) - ok
    by = {}
    labels, streams = zip(*D.specials())
    caps = np.full(len(streams), 4000, dtype=np.int64)
    _, status, _ = _decode(streams, caps, 4096, rng)
    by = dict(zip(labels, status))
    assert by['preset-dictionary'] == L.RDR_INFL_INVALID and by['block-type-3'] == L.RDR_INFL_INVALID and by['len-nlen'] == L.RDR_INFL_INVALID
    assert by['too-far-back'] == L.RDR_INFL_INVALID and by['wrong-adler'] == L.RDR_INFL_CHECKSUM and by['trailing-bytes'] == L.RDR_INFL_OK
    assert rejected > 1000 and accepted > 0                      # (a flipped bit behind the Adler-32, or in a bit zlib does not read, is accepted)


def test_abi_errors():
    ctx = L.Context.default()
    src = torch.zeros(64, dtype=torch.uint8, device=_dev())
    out = torch.zeros(256, dtype=torch.uint8, device=_dev())
    status = torch.zeros(2, dtype=torch.int32, device=_dev())
    i64 = lambda *v: np.array(v, dtype=np.int64)

    def call(src=src, nsrc=64, so=i64(0, 8), sb=i64(8, 8), n=2, cap=i64(128, 128), out=out, stride=128, status=status, loc=L.RDR_DEVICE):
        return ctx.lib.rdr_inflate_decode(ctx.handle, L.ptr(src), nsrc, L.ptr(so), L.ptr(sb), n, L.ptr(cap), L.ptr(out), stride, L.ptr(status), None, loc)

    assert call() == L.RDR_OK                                    # (two streams of zeros: bad headers, a status each)
    assert list(status.cpu().numpy()) == [L.RDR_INFL_INVALID] * 2
    for kw in (dict(src=None), dict(so=None), dict(sb=None), dict(cap=None), dict(out=None), dict(status=None), dict(nsrc=0), dict(n=0), dict(stride=0),
               dict(stride=-16), dict(so=i64(0, 60)), dict(so=i64(-1, 8)), dict(sb=i64(8, -1)), dict(sb=i64(8, 100)), dict(cap=i64(128, 129)),
               dict(cap=i64(-1, 128)), dict(stride=1 << 31, cap=i64(1, 1)), dict(loc=7)):
        assert call(**kw) == L.RDR_ERR_INVALID, kw
    with pytest.raises(ValueError):
        inflate_segments(src, [0], [8, 8], [16])
    with pytest.raises(ValueError):
        inflate_segments(src, [], [], [])
    with pytest.raises(TypeError):
        inflate_segments(src.cpu(), [0], [8], [16])


# ---- tifflite ------------------------------------------------------------------------------------------------------------------------
def _raster(dtype, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:150, 0:130]
    a = np.stack([1000 + 3 * y + 2 * x + rng.integers(0, 5, (150, 130)), 20000 - y * x // 7 + rng.integers(0, 3, (150, 130))])
    return (a / 7.0).astype(dtype) if np.dtype(dtype).kind == 'f' else a.astype(dtype)


@pytest.mark.parametrize('dtype', [np.uint16, np.float32, np.float64])
@pytest.mark.parametrize('layout', ['strips', 'tiles'])
@pytest.mark.parametrize('predictor', [1, 2])
@pytest.mark.parametrize('planar', [1, 2])
def test_tifflite_device_route_equals_host_route(tmp_path, dtype, layout, predictor, planar):
    a = _raster(dtype, 31)
    kw = dict(rows_per_strip=32) if layout == 'strips' else dict(tile=(64, 64))      # a short last strip; tiles with padded edges
    p = tmp_path / 'a.tif'
    p.write_bytes(T.make_tiff(a, compression=8, predictor=predictor, planar=planar, **kw))
    host, prof = tifflite.read(p)
    assert np.array_equal(host, a)
    dev, prof_d = tifflite.read(p, device=_dev(), inflate='device')
    assert dev.is_cuda and prof_d == prof
    assert dev.cpu().numpy().tobytes() == host.tobytes() and tuple(dev.shape) == host.shape
    down, _ = tifflite.read(p, inflate='device')                # device=None: the result is downloaded
    assert isinstance(down, np.ndarray) and down.tobytes() == host.tobytes()
    one, _ = tifflite.read(p, band=2, device=_dev(), inflate='device')
    assert one.cpu().numpy().tobytes() == host[1].tobytes()
    same, _ = tifflite.read(p, device=_dev(), inflate='host')
    assert same.cpu().numpy().tobytes() == host.tobytes()


def test_tifflite_written_by_the_device_encoder(tmp_path):
    a = _raster(np.float32, 32)[0]
    p = tmp_path / 'w.tif'
    tifflite.write(p, a, compress='deflate', rows_per_strip=16, predictor=2, encoder='device')
    host, _ = tifflite.read(p)
    dev, _ = tifflite.read(p, device=_dev(), inflate='device')
    assert dev.cpu().numpy().tobytes() == host.tobytes() == a.tobytes()


def _patch_counts(data, counts, k, new):
    """The file with segment k's byte count set to `new` (the counts lie out of line, as one run of uint32)."""
    old = struct.pack(f'<{len(counts)}I', *counts)
    assert data.count(old) == 1
    i = data.index(old)
    counts = list(counts); counts[k] = new
    return data[:i] + struct.pack(f'<{len(counts)}I', *counts) + data[i + len(old):]


def test_tifflite_truncated_and_overlong_segments(tmp_path):
    a = _raster(np.uint16, 33)[0]
    data = T.make_tiff(a, compression=8, predictor=2, rows_per_strip=32)
    p = tmp_path / 'cut.tif'
    p.write_bytes(data)
    info = tifflite.TiffInfo(p)
    counts = [int(c) for c in info.bytecounts]
    p.write_bytes(_patch_counts(data, counts, 2, counts[2] // 2))
    msgs = []
    for kw in (dict(), dict(device=_dev(), inflate='host'), dict(device=_dev(), inflate='device'), dict(inflate='device')):
        with pytest.raises(tifflite.NotATIFF, match='segment 2: deflate stream is damaged') as e:
            tifflite.read(p, **kw)
        msgs.append(str(e.value))
    assert len(set(msgs)) == 1
    # a last strip that holds all 32 rows where 22 are needed: ImageLength 160 -> 150 in a file of five strips
    tall = np.concatenate([a, a[:10]])
    data = bytearray(T.make_tiff(tall, compression=8, predictor=2, rows_per_strip=32))
    entry = struct.pack('<HHII', 257, 4, 1, 160)
    assert data.count(entry) == 1
    i = data.index(entry)
    data[i:i + 12] = struct.pack('<HHII', 257, 4, 1, 150)
    q = tmp_path / 'long.tif'
    q.write_bytes(bytes(data))
    host, _ = tifflite.read(q)
    assert np.array_equal(host, a)
    dev, _ = tifflite.read(q, device=_dev(), inflate='device')
    assert dev.cpu().numpy().tobytes() == host.tobytes()


# ---- h5lite --------------------------------------------------------------------------------------------------------------------------
SHAPE, CHUNK = (5, 37, 41), (2, 16, 16)


def _cube(dtype, seed):
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(np.linspace(0, 9000, SHAPE[0]), np.linspace(34, 33, SHAPE[1]), np.linspace(-118, -117, SHAPE[2]), indexing='ij')
    return (2.3 * np.exp(-z / 8000.0) * (1 + 0.05 * np.sin(8 * x) * np.cos(9 * y)) + 1e-5 * rng.standard_normal(SHAPE)).astype(dtype)


def _host_chunked(a, file_dtype, shuffle, fletcher, level=6):
    """h5write.ChunkedData of `a` with zlib chunks made on the host, stored as file_dtype (either byte order)."""
    stored = a.astype(file_dtype)
    raw = deflate.h5_chunks_host(stored, CHUNK, 0, shuffle=shuffle)
    n = int(np.prod(deflate.chunk_grid(SHAPE, CHUNK)))
    cb = raw.size // n
    parts = [zlib.compress(raw[k * cb:(k + 1) * cb].tobytes(), level) + (struct.pack('<I', 0xdeadbeef) if fletcher else b'') for k in range(n)]
    filters = (('shuffle',) if shuffle else ()) + ('deflate',) + (('fletcher32',) if fletcher else ())
    return h5write.ChunkedData(SHAPE, file_dtype, CHUNK, b''.join(parts), np.cumsum([0] + [len(p) for p in parts]), filters=filters, level=level)


def _bits(a):
    return np.ascontiguousarray(a).view(f'u{a.dtype.itemsize}')


@pytest.mark.parametrize('dtype', ['<f4', '<f8', '>f4', '>f8'])
@pytest.mark.parametrize('shuffle,fletcher', [(True, False), (False, False), (True, True), (False, True)])
def test_h5lite_read_device_equals_read(tmp_path, dtype, shuffle, fletcher):
    a = _cube(np.dtype(dtype).newbyteorder('='), 41)
    a[0, 1, 2] = np.nan
    p = tmp_path / 'c.h5'
    h5write.write_hdf5(p, [('wet', _host_chunked(a, np.dtype(dtype), shuffle, fletcher), [('units', 'm')], None)])
    ds = h5lite.File(p)['wet']
    host = ds.read()
    assert host.dtype.isnative and np.array_equal(_bits(host), _bits(a))
    dev = ds.read_device(inflate='device')
    assert dev is not None and dev.is_cuda and tuple(dev.shape) == SHAPE
    got = dev.cpu().numpy()
    assert got.dtype == host.dtype and np.array_equal(_bits(got), _bits(host))
    assert ds.read_device(inflate='host') is None
    with pytest.raises(ValueError, match='inflate must be'):
        ds.read_device(inflate='gpu')


def test_h5lite_candidates_and_a_damaged_chunk(tmp_path):
    a = _cube(np.float32, 42)
    plain = a.copy()
    no_filter = h5write.ChunkedData(SHAPE, a.dtype, CHUNK, deflate.h5_chunks_host(a, CHUNK, 0, shuffle=False).tobytes(),
                                    np.arange(28) * (2 * 16 * 16 * 4), filters=())
    good = _host_chunked(a, np.dtype('<f4'), True, False)
    p = tmp_path / 'k.h5'
    h5write.write_hdf5(p, [('plain', plain, [], None), ('nofilter', no_filter, [], None), ('good', good, [], None)])
    f = h5lite.File(p)
    assert f['plain'].read_device(inflate='device') is None      # contiguous: raw() serves it
    assert f['nofilter'].read_device(inflate='device') is None   # chunked, no deflate
    assert np.array_equal(f['nofilter'].read(), a)
    assert np.array_equal(f['good'].read_device(inflate='device').cpu().numpy(), a)
    # one chunk with a flipped bit in its deflate body: both routes raise zlib's error
    packed = bytearray(good.packed.tobytes())
    packed[int(good.offsets[5]) + 40] ^= 0x10
    bad = h5write.ChunkedData(SHAPE, a.dtype, CHUNK, bytes(packed), good.offsets, filters=good.filters, level=6)
    q = tmp_path / 'bad.h5'
    h5write.write_hdf5(q, [('wet', bad, [], None)])
    ds = h5lite.File(q)['wet']
    with pytest.raises(zlib.error) as e_host:
        ds.read()
    with pytest.raises(zlib.error) as e_dev:
        ds.read_device(inflate='device')
    assert str(e_host.value) == str(e_dev.value)


@pytest.mark.parametrize('tables', ['fixed', 'dynamic'])
def test_delay_cube_file_through_getInterpolators(tmp_path, monkeypatch, tables):
    from raider_amd.delay import DelayCube
    from raider_amd.delayFcns import clear_file_cache, getInterpolators
    wet, hydro = 0.1 * _cube(np.float64, 43), _cube(np.float64, 44)
    wet[0, 1, 2] = np.nan
    v = {'wet': wet, 'hydro': hydro, 'z': np.linspace(0.0, 9000.0, SHAPE[0]), 'y': np.linspace(34.0, 33.0, SHAPE[1]), 'x': np.linspace(-118.0, -117.0, SHAPE[2])}
    cube = DelayCube(v, {'description': 'RAiDER geo cube - ray tracing'})
    packed, plain = tmp_path / 'packed.nc', tmp_path / 'plain.nc'
    cube.to_netcdf(packed, compress=True, chunks=CHUNK, tables=tables)
    cube.to_netcdf(plain)
    f = h5lite.File(packed)
    for name, want in (('wet', wet), ('hydro', hydro)):
        assert f[name].raw() is None
        dev = f[name].read_device(inflate='device')
        assert np.array_equal(_bits(dev.cpu().numpy()), _bits(f[name].read())) and np.array_equal(_bits(dev.cpu().numpy()), _bits(want))
    calls = []
    real = h5lite.Dataset.read_device
    monkeypatch.setattr(h5lite, '_INFLATE_MIN_CHUNKS', 1)
    monkeypatch.setattr(h5lite.Dataset, 'read_device', lambda self, *a, **k: calls.append(self.name) or real(self, *a, **k))
    clear_file_cache()
    rng = np.random.default_rng(45)
    pts = np.stack([rng.uniform(32.9, 34.1, 1000), rng.uniform(-118.1, -116.9, 1000), rng.uniform(-100.0, 9100.0, 1000)], axis=-1)
    got = [i(pts) for i in getInterpolators(str(packed))]
    assert len(calls) == 2                                       # both fields came through the device route
    want = [i(pts) for i in getInterpolators(str(plain))]
    assert len(calls) == 2                                       # the contiguous file is served by raw()
    for g, w in zip(got, want):
        assert np.array_equal(_bits(g), _bits(w)) and np.isfinite(w).sum() > 500
    clear_file_cache()


# ---- the input window, the routing rule, the chunk table -----------------------------------------------------------------------------
def test_empty_stored_block_in_the_last_window_at_every_alignment():
    """The stored-block header hands the bit buffer's whole bytes back; when that ends a batch in the stream's last input window the
    position lies before a window staged for that batch.  Every such stream, at each of the four source alignments, in one call."""
    streams, want = [], []
    for n, m in D.SYNC_TAILS:
        s, d = D.crafted_sync_tail(n, m)
        assert zlib.decompress(s) == d
        streams.append(s); want.append(d)
    enc = deflate.deflate_segments(torch.from_numpy(np.frombuffer(D.delay_like(9000, seed=3), dtype=np.uint8).copy()).to(_dev()), [0], [36000])
    own = enc[0].cpu().numpy().tobytes()                          # the device encoder's stream: an empty stored block behind each 32 KiB
    streams.append(own); want.append(zlib.decompress(own))
    parts, offs, pos = [], [], 0
    for a in range(4):
        for s in streams:
            pad = (a - pos) % 4 + 4
            parts += [bytes([SENTINEL]) * pad, s]
            offs.append(pos + pad)
            pos += pad + len(s)
    assert sorted(set(o % 4 for o in offs)) == [0, 1, 2, 3]
    buf = torch.from_numpy(np.frombuffer(b''.join(parts), dtype=np.uint8).copy()).to(_dev())
    assert buf.data_ptr() % 4 == 0
    sizes = [len(s) for s in streams] * 4
    caps = np.array([len(w) for w in want] * 4, dtype=np.int64)
    out, status, produced = inflate_segments(buf, offs, sizes, caps)
    stride = out.numel() // len(offs)
    assert list(status.cpu().numpy()) == [0] * len(offs), status
    back, produced = out.cpu().numpy().reshape(len(offs), stride), produced.cpu().numpy()
    for k in range(len(offs)):
        w = want[k % len(streams)]
        assert produced[k] == len(w) and back[k, :len(w)].tobytes() == w, (k, offs[k] % 4)


def test_tifflite_auto_takes_the_device_route_from_the_threshold(tmp_path, monkeypatch):
    calls = []
    real = deflate.inflate_segments
    monkeypatch.setattr(deflate, 'inflate_segments', lambda *a, **k: calls.append(len(a[1])) or real(*a, **k))
    n = tifflite._INFLATE_MIN_SEGMENTS
    for rows, routed in ((n - 1, False), (n, True), (n + 1, True)):
        a = np.arange(rows * 24, dtype=np.uint16).reshape(rows, 24)
        p = tmp_path / f'{rows}.tif'
        p.write_bytes(T.make_tiff(a, compression=8, predictor=2, rows_per_strip=1))
        assert len(tifflite.TiffInfo(p).offsets) == rows
        calls.clear()
        t, _ = tifflite.read(p, device=_dev())                   # 'auto' with a device: by segment count
        assert np.array_equal(t.cpu().numpy(), a) and calls == ([rows] if routed else [])
        calls.clear()
        h, _ = tifflite.read(p)                                  # 'auto' without one: NumPy all the way
        assert isinstance(h, np.ndarray) and np.array_equal(h, a) and calls == []
        tifflite.read(p, device=_dev(), inflate='host')
        assert calls == []
        tifflite.read(p, device=_dev(), inflate='device')
        assert calls == [rows]


def test_h5lite_auto_threshold(tmp_path, monkeypatch):
    a = _cube(np.float32, 46)
    p = tmp_path / 't.h5'
    h5write.write_hdf5(p, [('wet', _host_chunked(a, np.dtype('<f4'), True, False), [], None)])
    ds = h5lite.File(p)['wet']
    monkeypatch.setattr(h5lite, '_INFLATE_MIN_CHUNKS', 28)
    assert ds.read_device() is None                              # 27 chunks: one short of the threshold
    monkeypatch.setattr(h5lite, '_INFLATE_MIN_CHUNKS', 27)
    assert np.array_equal(ds.read_device().cpu().numpy(), a)


@pytest.mark.parametrize('dtype', ['u1', 'i2', 'f4', 'f8'])
@pytest.mark.parametrize('shape,chunk', [((37,), (16,)), ((9, 21), (4, 8)), ((5, 37, 41), (2, 16, 16)), ((3, 5, 9, 11), (2, 2, 4, 8))])
@pytest.mark.parametrize('tensor', [True, False])
def test_unchunk_on_the_device_equals_its_restatement(shape, chunk, dtype, tensor):
    """rdr_h5_unchunk itself: chunks in another order at a stride beyond the chunk, one chunk absent (the zero fill), both byte orders,
    with and without the shuffle - against deflate.h5_unchunk_host, which the host test holds against the cutter."""
    rng = np.random.default_rng(len(shape) * 10 + np.dtype(dtype).itemsize)
    a = rng.integers(1, 250, size=shape).astype(dtype)
    n = int(np.prod(deflate.chunk_grid(shape, chunk)))
    for shuffle, swap in ((True, False), (False, True), (True, True)):
        src = a.astype(np.dtype(dtype).newbyteorder('S')) if swap else a
        raw = deflate.h5_chunks_host(src, chunk, 0, shuffle=shuffle).reshape(n, -1)
        cb = raw.shape[1]
        order = np.delete(rng.permutation(n), 0)                 # every chunk but one, shuffled
        padded = np.full((order.size, cb + 24), SENTINEL, dtype=np.uint8)
        padded[:, :cb] = raw[order]
        want = deflate.h5_unchunk_host(padded, cb + 24, order, dtype, shape, chunk, shuffle=shuffle, swap=swap)
        assert not np.array_equal(want, a) and (want == 0).any()
        buf = torch.from_numpy(padded.reshape(-1).copy()).to(_dev()) if tensor else padded.reshape(-1)
        got = deflate.h5_unchunk(buf, cb + 24, order, dtype, shape, chunk, shuffle=shuffle, swap=swap)
        got = got.cpu().numpy() if tensor else got
        assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes()
        full = deflate.h5_unchunk(torch.from_numpy(raw.reshape(-1).copy()).to(_dev()), cb, np.arange(n), dtype, shape, chunk, shuffle=shuffle, swap=swap)
        assert full.cpu().numpy().tobytes() == a.tobytes()
    ctx = L.Context.default()
    i64 = lambda *v: np.array(v, dtype=np.int64)
    one, dst = torch.zeros(64, dtype=torch.uint8, device=_dev()), torch.zeros(40, dtype=torch.uint8, device=_dev())
    call = lambda idx, npresent: ctx.lib.rdr_h5_unchunk(ctx.handle, L.ptr(one), 16, L.ptr(idx), npresent, 1, 1, L.ptr(i64(40)), L.ptr(i64(16)), 0, 0, L.ptr(dst), L.RDR_DEVICE)
    assert call(i64(0, 2), 2) == L.RDR_OK
    assert call(i64(0, 0), 2) == L.RDR_ERR_INVALID and call(i64(0, 3), 2) == L.RDR_ERR_INVALID and call(i64(-1, 1), 2) == L.RDR_ERR_INVALID
    assert call(i64(0, 1, 2, 2), 4) == L.RDR_ERR_INVALID
