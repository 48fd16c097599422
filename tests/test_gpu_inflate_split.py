"""GPU: rdr_inflate_decode_split - long zlib streams cut at their flush points and decoded by many waves - through
raider_amd.deflate.inflate_segments(..., split=True) and the two readers.  The contract is the serial call: for every stream, good or
bad, out (the guard bytes around the slots included), status and produced are those of inflate_segments(...) without the keyword, for
the same pre-filled buffer; accepted streams are zlib's bytes.  The streams with true, history-keeping and false flush points are the
ones tests/test_inflate_split_host.py ran on the CPU under the sanitizers, where their premises are asserted with zlib alone."""
import struct
import zlib

import numpy as np
import pytest

from raider_amd import _lib as L
from raider_amd import deflate, h5lite, tifflite
from raider_amd.deflate import inflate_segments
from tests import deflate_craft as D
from tests import test_inflate_split_host as H

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

SENTINEL = 0xA5
GUARD = 64
BOTH = pytest.mark.parametrize('tensor', [True, False], ids=['tensor', 'numpy'])


def _dev():
    return torch.device('cuda', 0)


def _pack(streams):
    """One buffer with stream k at an offset congruent to k mod 4, sentinel bytes between."""
    parts, offs, pos = [], [], 0
    for k, s in enumerate(streams):
        pad = (k - pos) % 4 + 4
        parts += [bytes([SENTINEL]) * pad, bytes(s)]
        offs.append(pos + pad)
        pos += pad + len(s)
    parts.append(bytes([SENTINEL]) * 8)
    return np.frombuffer(b''.join(parts), dtype=np.uint8).copy(), np.array(offs, dtype=np.int64)


def _both(streams, caps, tensor, odd=0):
    """The serial and the split call on the same streams and the same pre-filled slots: (slots (n, stride), status, produced, pieces) of the
    split call, after asserting that the two calls agree in every byte.  The streams are repeated until there are four, so that the
    offsets take every value mod 4; GUARD sentinel bytes lie in front of the first slot and behind every slot (odd: added to the
    stride, so that the slots' addresses take every value mod 4 too)."""
    reps = -(-4 // len(streams))
    n0 = len(streams)
    streams, caps = list(streams) * reps, np.array(list(caps) * reps, dtype=np.int64)
    buf, offs = _pack(streams)
    assert sorted(set(int(o) % 4 for o in offs)) == [0, 1, 2, 3]
    sizes = np.array([len(s) for s in streams], dtype=np.int64)
    n = len(streams)
    stride = (int(caps.max()) + GUARD + 3) // 4 * 4 + odd
    got = []
    for split in (False, True):
        if tensor:
            whole = torch.full((GUARD + n * stride,), SENTINEL, dtype=torch.uint8, device=_dev())
            _, status, produced = inflate_segments(torch.from_numpy(buf).to(_dev()), offs, sizes, caps, out_stride=stride, out=whole[GUARD:], split=split)
            got.append((whole.cpu().numpy(), status.cpu().numpy(), produced.cpu().numpy()))
        else:
            whole = np.full(GUARD + n * stride, SENTINEL, dtype=np.uint8)
            _, status, produced = inflate_segments(buf, offs, sizes, caps, out_stride=stride, out=whole[GUARD:], split=split)
            got.append((whole, status, produced))
    (a, sa, pa), (b, sb, pb) = got
    assert np.array_equal(sa, sb), (sa, sb)
    assert np.array_equal(pa, pb), (pa, pb)
    assert np.array_equal(a, b), np.nonzero(a != b)[0][:8]
    pieces = deflate.last_pieces()
    assert pieces.shape == (n,) and np.all(pieces >= 1)
    assert np.all(a[:GUARD] == SENTINEL)
    slots = a[GUARD:].reshape(n, stride)
    for k, s in enumerate(streams):
        want = D.judge(s, int(caps[k]))
        assert np.all(slots[k, int(caps[k]):] == SENTINEL), k
        if want is None:
            assert 1 <= sb[k] <= 4, (k, sb[k])
        else:
            assert sb[k] == 0 and pb[k] == len(want) and slots[k, :len(want)].tobytes() == want, (k, sb[k], pb[k])
            assert np.all(slots[k, len(want):] == SENTINEL), k
        assert pieces[k] == pieces[k % n0], (k, pieces)           # the same stream at another alignment: the same plan
    return slots, sb, pb, pieces


def _own(data, sizes, tables):
    """The device encoder's streams of consecutive ranges of `data`."""
    src = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(_dev())
    cuts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    packed, oo = deflate.deflate_segments(src, cuts[:-1], np.diff(cuts), tables=tables)
    packed = packed.cpu().numpy().tobytes()
    return [packed[int(oo[k]):int(oo[k + 1])] for k in range(len(sizes))]


LENGTHS = [1, 32768, 32769, 100000, 5 * 32768 + 17]


@BOTH
@pytest.mark.parametrize('tables', ['fixed', 'dynamic'])
def test_own_encoder(tensor, tables):
    rnd = np.random.default_rng(53)
    kinds = {'delay': b''.join(D.delay_like(n // 4 + 1, seed=51)[:n] for n in LENGTHS),      # every range a shuffled array of its own
             'text': b''.join(D.text_like(n, seed=52) for n in LENGTHS), 'random': rnd.integers(0, 256, sum(LENGTHS), dtype=np.uint8).tobytes()}
    streams, labels = [], []
    for name, data in kinds.items():
        streams += _own(data, LENGTHS, tables)
        labels += [(name, n) for n in LENGTHS]
    assert deflate.last_block_counts()[0] == sum(-(-n // 32768) for n in LENGTHS)          # the random input: every sub-block stored
    caps = [n for _, n in labels]
    assert all(len(zlib.decompress(s)) == c for s, c in zip(streams, caps))
    _, status, _, pieces = _both(streams, caps, tensor, odd=1)
    assert np.all(status == 0)
    for k, (name, n) in enumerate(labels):
        if n == 1 or name == 'random':
            assert H.candidates(streams[k]) == [], (name, n)     # (stored sub-blocks carry no marker; the one in front of a trailer is none)
            assert pieces[k] == 1, (name, n, pieces[k])
        elif n > 32768:
            assert pieces[k] >= 2, (name, n, pieces[k])
            assert pieces[k] <= -(-n // 32768), (name, n, pieces[k])


@BOTH
def test_full_flush(tensor):
    full, points = H.full_stream()
    _, status, _, pieces = _both([full], [60000], tensor)
    # twelve flush points, each the only marker of its 1024-byte window and none by chance: twelve candidates, thirteen pieces in the
    # chain, of which the empty final block behind the last flush point joins the twelfth
    assert len(H.candidates(full)) == 12
    assert np.all(status == 0) and list(pieces) == [12] * 4


@BOTH
def test_sync_flush_keeps_the_history(tensor):
    (s1, _), (s2, _) = H.sync_streams()
    _, status, _, pieces = _both([s1, s2], [60000, 60000], tensor)
    assert np.all(status == 0) and list(pieces) == [1] * 4       # every piece reaches back; in s2 across two predecessors


@BOTH
def test_mixed_flushes(tensor):
    mixed, points = H.mixed_stream()
    _, status, _, pieces = _both([mixed], [100000], tensor)
    assert np.all(status == 0) and 2 <= pieces[0] < len(points)


@BOTH
def test_false_candidates(tensor):
    stored, payload = H.stored_false()
    crafted, data = H.crafted_false()
    assert H.candidates(stored) and H.candidates(crafted)
    _, status, _, pieces = _both([stored, crafted], [len(payload), len(data)], tensor)
    assert np.all(status == 0) and list(pieces) == [1] * 4


@BOTH
def test_bad_streams(tensor):
    n = 5 * 32768
    own = _own(D.text_like(n, seed=54), [n], 'fixed')[0]
    cands = H.candidates(own)
    assert len(cands) == 4
    cut = own[:(cands[1] + cands[2]) // 2]                        # inside piece 3
    flip = bytearray(own); flip[(cands[0] + cands[1]) // 2] ^= 0x40   # inside piece 2
    adler = own[:-4] + struct.pack('>I', (zlib.adler32(zlib.decompress(own)) + 1) & 0xffffffff)
    sp = dict(D.specials())
    streams = [own, cut, bytes(flip), adler, own, sp['len-nlen'], sp['too-far-back'], b'']
    caps = [n, n, n, n, n - 1, 4000, 4000, 4000]
    slots, status, produced, pieces = _both(streams, caps, tensor)
    assert pieces[0] == 5 and status[0] == 0
    assert status[1] == L.RDR_INFL_SHORT and status[4] == L.RDR_INFL_OVERFLOW and status[3] == L.RDR_INFL_CHECKSUM
    assert status[2] != 0 and D.judge(bytes(flip)) is None        # (whichever status the serial call gives the flipped byte)
    assert status[5] == L.RDR_INFL_INVALID and status[6] == L.RDR_INFL_INVALID and status[7] == L.RDR_INFL_SHORT
    assert list(pieces[[1, 4, 5, 6, 7]]) == [1] * 5               # not clean: through the serial kernel
    assert 0 < produced[1] < n and np.all(slots[1, produced[1]:] == SENTINEL)       # the bytes the serial call leaves stay
    assert produced[7] == 0 and np.all(slots[7] == SENTINEL)


def test_abi_errors():
    ctx = L.Context.default()
    assert hasattr(ctx.lib, 'rdr_inflate_decode_split')
    src = torch.zeros(64, dtype=torch.uint8, device=_dev())
    out = torch.full((256,), SENTINEL, dtype=torch.uint8, device=_dev())
    status = torch.full((2,), -7, dtype=torch.int32, device=_dev())
    pieces = np.full(2, -7, dtype=np.int64)
    i64 = lambda *v: np.array(v, dtype=np.int64)

    def call(src=src, nsrc=64, so=i64(0, 8), sb=i64(8, 8), n=2, cap=i64(128, 128), out=out, stride=128, status=status, pieces=pieces, loc=L.RDR_DEVICE):
        return ctx.lib.rdr_inflate_decode_split(ctx.handle, L.ptr(src), nsrc, L.ptr(so), L.ptr(sb), n, L.ptr(cap), L.ptr(out), stride, L.ptr(status), None,
                                                None if pieces is None else L.ptr(pieces), loc)

    for kw in (dict(src=None), dict(so=None), dict(sb=None), dict(cap=None), dict(out=None), dict(status=None), dict(nsrc=0), dict(n=0), dict(n=-1), dict(stride=0),
               dict(stride=-16), dict(so=i64(0, 60)), dict(so=i64(-1, 8)), dict(sb=i64(8, -1)), dict(sb=i64(8, 100)), dict(cap=i64(128, 129)),
               dict(cap=i64(-1, 128)), dict(stride=1 << 31, cap=i64(1, 1)), dict(loc=7)):
        assert call(**kw) == L.RDR_ERR_INVALID, kw
    assert np.all(out.cpu().numpy() == SENTINEL) and list(status.cpu().numpy()) == [-7, -7] and list(pieces) == [-7, -7]
    assert call(pieces=None) == L.RDR_OK                         # (two streams of zeros: bad headers, a status each)
    assert list(status.cpu().numpy()) == [L.RDR_INFL_INVALID] * 2 and np.all(out.cpu().numpy() == SENTINEL)
    assert call() == L.RDR_OK and list(pieces) == [1, 1]
    with pytest.raises(ValueError):
        inflate_segments(src, [0], [8, 8], [16], split=True)


# ---- the readers ---------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(f'u{a.dtype.itemsize}')


def _cube_file(tmp_path):
    from raider_amd.delay import DelayCube
    rng = np.random.default_rng(55)
    z, y, x = np.meshgrid(np.linspace(0, 9000, 20), np.linspace(34, 33, 48), np.linspace(-118, -117, 48), indexing='ij')
    wet = (0.23 * np.exp(-z / 8000.0) * (1 + 0.05 * np.sin(8 * x) * np.cos(9 * y)) + 1e-5 * rng.standard_normal(z.shape)).astype(np.float32)
    v = {'wet': wet, 'hydro': (10 * wet).astype(np.float32), 'z': np.linspace(0.0, 9000.0, 20), 'y': np.linspace(34.0, 33.0, 48), 'x': np.linspace(-118.0, -117.0, 48)}
    p = tmp_path / 'cube.nc'
    DelayCube(v, {'description': 'RAiDER geo cube - ray tracing'}).to_netcdf(p, compress=True)
    return p


def test_delay_cube_file_both_routes(tmp_path):
    f = h5lite.File(_cube_file(tmp_path))
    for name in ('wet', 'hydro'):
        dev = f[name].read_device(inflate='device')
        assert dev is not None and dev.is_cuda
        assert f[name].read_device(inflate='host') is None
        assert np.array_equal(_bits(dev.cpu().numpy()), _bits(f[name].read()))


def test_h5lite_auto_counts_flush_points(tmp_path, monkeypatch):
    ds = h5lite.File(_cube_file(tmp_path))['wet']
    chunk, entries = ds._chunks(ds.layout, ds.shape)
    entries = list(entries)
    buf = np.frombuffer(ds.file.buf, dtype=np.uint8)
    marks = sum(deflate.flush_points(bytes(buf[ds.file.base + addr:ds.file.base + addr + size])) for _, size, _, addr, _ in entries)
    assert len(entries) == 9 and marks >= 1
    monkeypatch.setattr(h5lite, '_INFLATE_MIN_PIECES', len(entries) + marks - 1)
    got = ds.read_device()
    assert got is not None and np.array_equal(_bits(got.cpu().numpy()), _bits(ds.read()))
    monkeypatch.setattr(h5lite, '_INFLATE_MIN_PIECES', len(entries) + marks + 1)
    assert ds.read_device() is None


def test_tifflite_strips_from_the_device_encoder(tmp_path, monkeypatch):
    rng = np.random.default_rng(56)
    y, x = np.mgrid[0:96, 0:1024]
    a = (1000 + 3 * y + 2 * x + rng.integers(0, 5, (96, 1024)) / 7.0).astype(np.float32)
    p = tmp_path / 'w.tif'
    tifflite.write(p, a, compress='deflate', rows_per_strip=32, predictor=2, encoder='device')
    host, _ = tifflite.read(p)
    dev, _ = tifflite.read(p, device=_dev(), inflate='device')
    assert dev.cpu().numpy().tobytes() == host.tobytes() == a.tobytes()
    assert np.all(deflate.last_pieces() >= 2)                    # strips of 128 KiB: four sub-blocks each
    calls = []
    real = deflate.inflate_segments
    monkeypatch.setattr(deflate, 'inflate_segments', lambda *k, **kw: calls.append(len(k[1])) or real(*k, **kw))
    units = tifflite._inflate_units(tifflite.TiffInfo(p))
    assert units > 3
    monkeypatch.setattr(tifflite, '_INFLATE_MIN_PIECES', units)
    auto, _ = tifflite.read(p, device=_dev())
    assert calls == [3] and auto.cpu().numpy().tobytes() == a.tobytes()
    monkeypatch.setattr(tifflite, '_INFLATE_MIN_PIECES', units + 1)
    tifflite.read(p, device=_dev())
    assert calls == [3]


@pytest.mark.parametrize('split', [False, True], ids=['serial', 'split'])
@pytest.mark.parametrize('shift', [1, 2, 3])
def test_literal_then_stored_block_into_an_unaligned_slot(shift, split):
    """One literal, then a stored block, into a slot whose address is `shift` mod 4: in front of the stored copy the decoder flushes up
    to the last word boundary of the global address, and with address + produced < 4 there is none (the offset must not wrap)."""
    rng = np.random.default_rng(57)
    streams, want = [], []
    for n in (10, 9000):                                         # (9000: the stored copy flushes on its way, past 8192 bytes)
        payload = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        w = D.BitWriter()
        D.fixed_block(w, [65], final=False)
        D.stored_block(w, payload)
        data = b'A' + payload
        streams.append(D.zlib_wrap(w.out, data)); want.append(data)
        assert zlib.decompress(streams[-1]) == data
    buf, offs = _pack(streams)
    stride = 9064
    whole = torch.full((GUARD + shift + 2 * stride,), SENTINEL, dtype=torch.uint8, device=_dev())
    assert whole.data_ptr() % 4 == 0 and stride % 4 == 0        # both slots at `shift` mod 4
    caps = [len(w) for w in want]
    _, status, produced = inflate_segments(torch.from_numpy(buf).to(_dev()), offs, [len(s) for s in streams], caps, out_stride=stride, out=whole[GUARD + shift:],
                                           split=split)
    got = whole.cpu().numpy()
    assert list(status.cpu().numpy()) == [0, 0] and list(produced.cpu().numpy()) == caps
    assert np.all(got[:GUARD + shift] == SENTINEL)
    for k, w in enumerate(want):
        slot = got[GUARD + shift + k * stride:GUARD + shift + (k + 1) * stride]
        assert slot[:len(w)].tobytes() == w and np.all(slot[len(w):] == SENTINEL), k
