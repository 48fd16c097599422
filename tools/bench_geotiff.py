"""GeoTIFF DEM from path to device: raider_amd.tifflite (LZW tiles decoded on the GPU; deflate tiles inflated by zlib on the host, predictor
undone on the GPU) against Pillow's libtiff decode on the host plus the upload - Pillow standing in for what rasterio does in the reference.

Synthesises one N x N int16 DEM (smooth terrain plus noise, so the codecs have something to find) twice - 256 x 256 LZW tiles, and
256 x 256 deflate tiles with predictor 2 - with an encoder of its own, checks that both readers give the same pixels, then times,
per file and per side, (a) path -> device tensor and (b) path -> heights sampled at M device points (interpolate_elevation's rule).
Every timing is a host clock around work that ends in a device synchronise; `warmup` untimed calls first (page cache, workspace
allocations), then `reps` calls with the two sides alternated; median, minimum, maximum.  The yardstick is recorded, not asserted.

    python tools/bench_geotiff.py [--size 4000] [--points 16000000] [--reps 9] [--warmup 2] --out profiles/r19_geotiff.json
"""
import argparse
import json
import os
import statistics
import struct
import sys
import tempfile
import time
import zlib
from concurrent.futures import ProcessPoolExecutor
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def lzw_encode(data):
    """TIFF-flavoured LZW (MSB-first, Clear 256, EOI 257, early change) of a bytes object; integer-keyed table, bits packed by NumPy."""
    codes, widths = [256], [9]
    table = {}
    nxt, width = 258, 9
    w = -1
    for b in data:
        if w < 0:
            w = b
            continue
        key = (w << 8) | b
        c = table.get(key)
        if c is not None:
            w = c
            continue
        codes.append(w); widths.append(width)
        table[key] = nxt; nxt += 1
        if nxt > 4094:
            codes.append(256); widths.append(width)
            table = {}; nxt = 258; width = 9
        elif nxt >= (1 << width) and width < 12:
            width += 1
        w = b
    if w >= 0:
        codes.append(w); widths.append(width)
        nxt += 1
        if nxt >= (1 << width) and width < 12:
            width += 1
    codes.append(257); widths.append(width)
    c = np.asarray(codes, dtype=np.uint32); wd = np.asarray(widths, dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(wd)[:-1]])
    nbits = int(wd.sum())
    bits = np.zeros((nbits + 7) // 8 * 8, dtype=np.uint8)
    for k in range(12):                                   # bit k (from the top) of every code at least k + 1 wide
        m = wd > k
        bits[start[m] + k] = (c[m] >> (wd[m] - 1 - k)) & 1
    return np.packbits(bits).tobytes()


def _encode_tile(args):
    kind, tile = args
    if kind == 'lzw':
        return lzw_encode(tile.tobytes())
    u = tile.view(np.uint16).copy()
    u[:, 1:] = u[:, 1:] - u[:, :-1]
    return zlib.compress(u.tobytes(), 6)


def write_tiled(path, dem, kind, gt, pool):
    """A classic little-endian GeoTIFF of int16 `dem` in 256 x 256 tiles, kind 'lzw' or 'deflate_pred2', EPSG:4326."""
    H, W = dem.shape
    T = 256
    tiles = []
    for y in range(0, H, T):
        for x in range(0, W, T):
            t = np.zeros((T, T), dtype=np.int16)
            blk = dem[y:y + T, x:x + T]
            t[:blk.shape[0], :blk.shape[1]] = blk
            tiles.append((kind, t))
    segs = list(pool.map(_encode_tile, tiles, chunksize=4))
    pos, offs = 8, []
    for s in segs:
        offs.append(pos); pos += len(s) + (len(s) & 1)
    ent = [(256, 4, [W]), (257, 4, [H]), (258, 3, [16]), (259, 3, [5 if kind == 'lzw' else 8]), (262, 3, [1]), (277, 3, [1]), (284, 3, [1]),
           (317, 3, [1 if kind == 'lzw' else 2]), (322, 4, [T]), (323, 4, [T]), (324, 4, offs), (325, 4, [len(s) for s in segs]), (339, 3, [2]),
           (33550, 12, [gt[1], -gt[5], 0.0]), (33922, 12, [0.0, 0.0, 0.0, gt[0], gt[3], 0.0]),
           (34735, 3, [1, 1, 0, 3, 1024, 0, 1, 2, 1025, 0, 1, 1, 2048, 0, 1, 4326]), (42113, 2, b'-32768\x00')]
    fmt = {3: 'H', 4: 'I', 12: 'd'}
    extra_pos = pos + 2 + 12 * len(ent) + 4
    ifd, blob = bytearray(struct.pack('<H', len(ent))), bytearray()
    for tag, typ, vals in ent:
        payload = vals if typ == 2 else struct.pack('<' + fmt[typ] * len(vals), *vals)
        ifd += struct.pack('<HHI', tag, typ, len(vals))
        if len(payload) <= 4:
            ifd += payload + bytes(4 - len(payload))
        else:
            ifd += struct.pack('<I', extra_pos + len(blob)); blob += payload + bytes(len(payload) & 1)
    ifd += struct.pack('<I', 0)
    with open(path, 'wb') as f:
        f.write(struct.pack('<2sHI', b'II', 42, pos))
        for s in segs:
            f.write(s + bytes(len(s) & 1))
        f.write(ifd); f.write(blob)
    return sum(len(s) for s in segs)


def _summary(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), repeats_ms=[round(v, 3) for v in ms])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4000)
    ap.add_argument('--points', type=int, default=16_000_000)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    N = a.size
    rng = np.random.default_rng(19)
    yy, xx = np.meshgrid(np.arange(N), np.arange(N), indexing='ij')
    dem = (1500 + 900 * np.sin(xx / 310.0) * np.cos(yy / 270.0) + 300 * np.sin((xx + 2 * yy) / 47.0) + rng.normal(0, 3, (N, N))).astype(np.int16)
    del yy, xx
    gt = (-118.0, 1.0 / 3600, 0.0, 35.0, 0.0, -1.0 / 3600)
    tmp = Path(tempfile.mkdtemp(prefix='bench_geotiff_'))
    files = {}
    with ProcessPoolExecutor(min(16, os.cpu_count() or 1)) as pool:           # (before anything touches the GPU)
        for kind in ('lzw', 'deflate_pred2'):
            p = tmp / f'dem_{kind}.tif'
            t0 = time.perf_counter()
            nbytes = write_tiled(p, dem, kind, gt, pool)
            files[kind] = dict(path=p, compressed_bytes=nbytes, encode_s=round(time.perf_counter() - t0, 2))

    import torch
    from PIL import Image
    from raider_amd import _lib, tifflite
    from raider_amd.interpolator import interpolate_elevation, raster_sample
    Image.MAX_IMAGE_PIXELS = None
    dev = torch.device('cuda:0')
    M = a.points
    g = torch.Generator(device=dev); g.manual_seed(5)
    xt = gt[0] + torch.rand(M, dtype=torch.float64, device=dev, generator=g) * (N * gt[1])
    yt = gt[3] + torch.rand(M, dtype=torch.float64, device=dev, generator=g) * (N * gt[5])

    def ours_tensor(p):
        return tifflite.read(p, band=1, device=dev)[0]

    def ours_heights(p):
        return interpolate_elevation(p, xt, yt)

    def pillow_tensor(p):
        with Image.open(p) as im:
            return torch.from_numpy(np.array(im)).to(dev)

    def pillow_heights(p):
        return raster_sample(pillow_tensor(p), gt, xt, yt, 'nearest')

    def clock(fn, p):
        t0 = time.perf_counter()
        r = fn(p)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    name, cus, _ = _lib.Context.default().device_info()
    out = dict(tool='bench_geotiff', device=name, compute_units=cus, source_hash=_lib.load().rdr_source_hash().decode(), size=N, dtype='int16', tile=256,
               points=M, reps=a.reps, warmup=a.warmup, pillow=__import__('PIL').__version__, torch=torch.__version__,
               timing='host clock around calls that end in torch.cuda.synchronize(); the two sides alternate call by call', files={})
    for kind, f in files.items():
        p = f['path']
        ref = np.array(Image.open(p))
        mine = ours_tensor(p).cpu().numpy()
        same = bool(np.array_equal(mine, ref) and np.array_equal(ref, dem))
        hs = bool(torch.equal(ours_heights(p), pillow_heights(p)))
        rec = dict(compression=kind, file_bytes=p.stat().st_size, raster_bytes=int(dem.nbytes), encode_s=f['encode_s'], pixels_identical_to_pillow=same,
                   heights_identical=hs)
        for label, mine_fn, their_fn in (('path_to_device_tensor', ours_tensor, pillow_tensor), ('path_to_sampled_heights', ours_heights, pillow_heights)):
            for _ in range(a.warmup):
                clock(mine_fn, p); clock(their_fn, p)
            tm, tp = [], []
            for _ in range(a.reps):
                tm.append(clock(mine_fn, p)[0]); tp.append(clock(their_fn, p)[0])
            rec[label] = dict(tifflite=_summary(tm), pillow_plus_upload=_summary(tp))
        out['files'][kind] = rec
        p.unlink()
    tmp.rmdir()
    line = json.dumps(out)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
