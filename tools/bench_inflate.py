"""Device inflate against host inflate: rdr_inflate_decode alone, and the two routes of tifflite.read / h5lite.Dataset.read_device
from path to device tensor, in one process.

1. Kernel alone: `--mb` MB of int16 DEM bytes (predictor-2 differences, as a GeoTIFF holds them) as 1, 4, 16, 64, 256 and 1024 equal
   zlib streams (level 6), decoded by one inflate_segments call on device tensors; GB/s of output and microseconds per token on lane
   0 (the tokens are counted by tools/probes/inflate_host_check, built without sanitizers; a wave decodes ceil(streams / grid) streams).
2. Path -> device tensor, inflate='host' against inflate='device', alternated call by call: the N x N int16 DEM in deflate tiles with
   predictor 2 at tile sizes that give 1 .. 1024 segments (256 x 256 is tools/bench_geotiff.py's deflate file; inflate='host' is that
   tool's route, unchanged); an N x N float32 delay raster as tifflite.write(encoder='device') writes it; 20 x M x M float32 and
   float64 cubes written chunked + shuffle + deflate by the device encoder in 4, 16 and 64 chunks (host: read() plus the upload).
   Every route's result is compared bit for bit before it is timed.
The crossover recorded per class is the smallest segment count from which on the device route's whole span (its maximum) lies below
the host route's minimum; None when it never does.  Host clocks around work that ends in a device synchronise; medians with spans.

    python tools/bench_inflate.py [--size 4000] [--cube 1000] [--mb 32] [--reps 5] [--warmup 1] --out profiles/r24_inflate.json
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
import zlib
from concurrent.futures import ProcessPoolExecutor
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / 'tools'))


def _summary(ms):
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), repeats_ms=[round(v, 3) for v in ms])


def _note(*what):
    print('[bench_inflate]', *what, file=sys.stderr, flush=True)


def _z6(b):
    return zlib.compress(b, 6)


def _encode_tile(t):
    u = t.view(np.uint16).copy()
    u[:, 1:] = u[:, 1:] - u[:, :-1]
    return zlib.compress(u.tobytes(), 6)


def write_deflate_tiles(path, dem, T, pool):
    """bench_geotiff.write_tiled's deflate + predictor-2 file with T x T tiles."""
    import struct
    H, W = dem.shape
    tiles = []
    for y in range(0, H, T):
        for x in range(0, W, T):
            t = np.zeros((T, T), dtype=np.int16)
            blk = dem[y:y + T, x:x + T]
            t[:blk.shape[0], :blk.shape[1]] = blk
            tiles.append(t)
    segs = list(pool.map(_encode_tile, tiles))
    pos, offs = 8, []
    for s in segs:
        offs.append(pos); pos += len(s) + (len(s) & 1)
    ent = [(256, 4, [W]), (257, 4, [H]), (258, 3, [16]), (259, 3, [8]), (262, 3, [1]), (277, 3, [1]), (284, 3, [1]), (317, 3, [2]), (322, 4, [T]), (323, 4, [T]),
           (324, 4, offs), (325, 4, [len(s) for s in segs]), (339, 3, [2])]
    fmt = {3: 'H', 4: 'I'}
    extra_pos = pos + 2 + 12 * len(ent) + 4
    ifd, blob = bytearray(struct.pack('<H', len(ent))), bytearray()
    for tag, typ, vals in ent:
        payload = struct.pack('<' + fmt[typ] * len(vals), *vals)
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
    return len(segs)


def build_probe(tmp):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    exe = tmp / 'inflate_host_check'
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O2', str(REPO / 'tools' / 'probes' / 'inflate_host_check.cpp'), '-o', str(exe)], check=True)
    return exe


def count_tokens(probe, tmp, streams, cap):
    import struct
    p = tmp / 'streams.bin'
    with open(p, 'wb') as f:
        f.write(struct.pack('<I', len(streams)))
        for s in streams:
            f.write(struct.pack('<II', len(s), cap)); f.write(s)
    r = subprocess.run([str(probe), str(p)], capture_output=True, text=True, check=True)
    p.unlink()
    rows = [l.split() for l in r.stdout.split('\n')[:-1]]
    assert len(rows) == len(streams) and all(row[0] == '0' for row in rows)
    return sum(int(row[3]) for row in rows)


def crossover(rows):
    """rows: [(segments, host summary, device summary)] in rising segment order."""
    best = None
    for n, h, d in reversed(rows):
        if d['max_ms'] < h['min_ms']:
            best = n
        else:
            break
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4000)
    ap.add_argument('--cube', type=int, default=1000)
    ap.add_argument('--mb', type=int, default=32)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--probe', default=None, help='a built tools/probes/inflate_host_check (built here when not given)')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    N, M = a.size, a.cube
    rng = np.random.default_rng(19)
    yy, xx = np.meshgrid(np.arange(N), np.arange(N), indexing='ij')
    dem = (1500 + 900 * np.sin(xx / 310.0) * np.cos(yy / 270.0) + 300 * np.sin((xx + 2 * yy) / 47.0) + rng.normal(0, 3, (N, N))).astype(np.int16)
    del yy, xx
    tmp = Path(tempfile.mkdtemp(prefix='bench_inflate_'))
    probe = Path(a.probe) if a.probe else build_probe(tmp)
    # ---- everything the host encodes, before anything touches the GPU
    u = dem.view(np.uint16).copy()
    u[:, 1:] = u[:, 1:] - u[:, :-1]
    flat = u.tobytes()[:a.mb << 20]
    kernel_sets, tiff_files = {}, {}
    with ProcessPoolExecutor(min(16, os.cpu_count() or 1)) as pool:
        for nseg in (1, 4, 16, 64, 256, 1024):
            cb = len(flat) // nseg
            kernel_sets[nseg] = (cb, list(pool.map(_z6, [flat[k * cb:(k + 1) * cb] for k in range(nseg)])))
        for T in (N, -(-N // 2), -(-N // 4 // 16) * 16, 512, 256, 128):
            p = tmp / f'dem_{T}.tif'
            n = write_deflate_tiles(p, dem, T, pool)
            if n in tiff_files:
                p.unlink()                                       # (a small --size: two tile sizes give one count)
            else:
                tiff_files[n] = p

    _note('encoded on the host')
    import torch
    from raider_amd import _lib, deflate, h5lite, h5write, tifflite
    dev = torch.device('cuda:0')
    name, cus, _ = _lib.Context.default().device_info()
    grid = 3 * cus

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def alternate(host_fn, dev_fn):
        for _ in range(a.warmup):
            clock(host_fn); clock(dev_fn)
        th, td = [], []
        for _ in range(a.reps):
            th.append(clock(host_fn)[0]); td.append(clock(dev_fn)[0])
        return _summary(th), _summary(td)

    out = dict(tool='bench_inflate', device=name, compute_units=cus, source_hash=_lib.load().rdr_source_hash().decode(), zlib=zlib.ZLIB_RUNTIME_VERSION,
               torch=torch.__version__, size=N, cube=[20, M, M], reps=a.reps, warmup=a.warmup,
               timing='host clock around calls that end in torch.cuda.synchronize(); the two routes alternate call by call',
               host_route="inflate='host' is the parent commit's route, the same code: zlib.decompress segment by segment, then the upload")
    # ---- 1. the kernel alone
    rows = []
    for nseg, (cb, streams) in kernel_sets.items():
        tokens = count_tokens(probe, tmp, streams, cb)
        sizes = np.array([len(s) for s in streams], dtype=np.int64)
        offs = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        src = torch.from_numpy(np.frombuffer(b''.join(streams), dtype=np.uint8).copy()).to(dev)
        caps = np.full(nseg, cb, dtype=np.int64)
        call = lambda: deflate.inflate_segments(src, offs, sizes, caps)
        o, status, produced = call()
        got = o.cpu().numpy().reshape(nseg, -1)[:, :cb].tobytes()
        assert bool((status == 0).all()) and got == flat[:cb * nseg]
        for _ in range(a.warmup):
            clock(call)
        s = _summary([clock(call)[0] for _ in range(a.reps)])
        per_wave = tokens / nseg * -(-nseg // grid)
        rows.append(dict(segments=nseg, decoded_bytes=cb * nseg, compressed_bytes=int(sizes.sum()), tokens=tokens, call=s,
                         output_GB_per_s=round(cb * nseg / s['median_ms'] / 1e6, 3), us_per_token_lane0=round(s['median_ms'] * 1e3 / per_wave, 4)))
        _note('kernel', rows[-1])
        del src, o
    out['kernel'] = rows
    # ---- 2a. the DEM, by segment count
    rows, pairs = [], []
    for nseg, p in sorted(tiff_files.items()):
        host_fn = lambda: tifflite.read(p, band=1, device=dev, inflate='host')[0]
        dev_fn = lambda: tifflite.read(p, band=1, device=dev, inflate='device')[0]
        same = bool(torch.equal(host_fn(), dev_fn())) and bool(np.array_equal(dev_fn().cpu().numpy(), dem))
        h, d = alternate(host_fn, dev_fn)
        rows.append(dict(segments=nseg, file_bytes=p.stat().st_size, identical=same, host=h, device=d))
        pairs.append((nseg, h, d))
        _note('dem', nseg, 'host', h['median_ms'], 'device', d['median_ms'])
        p.unlink()
    out['dem_int16_deflate_pred2'] = dict(rows=rows, crossover_segments=crossover(pairs))
    # ---- 2b. a float32 delay raster as the device encoder writes it
    yy, xx = np.meshgrid(np.linspace(0, 6, N), np.linspace(0, 5, N), indexing='ij')
    delay = (2.3 + 0.2 * np.sin(xx) * np.cos(yy) + 1e-4 * rng.standard_normal((N, N))).astype(np.float32)
    del yy, xx
    p = tmp / 'delay.tif'
    tifflite.write(p, delay, compress='deflate', rows_per_strip=4, predictor=2, encoder='device')
    host_fn = lambda: tifflite.read(p, band=1, device=dev, inflate='host')[0]
    dev_fn = lambda: tifflite.read(p, band=1, device=dev, inflate='device')[0]
    same = bool(torch.equal(host_fn(), dev_fn())) and dev_fn().cpu().numpy().tobytes() == delay.tobytes()
    h, d = alternate(host_fn, dev_fn)
    out['delay_float32_device_written'] = dict(segments=len(tifflite.TiffInfo(p).offsets), file_bytes=p.stat().st_size, identical=same, host=h, device=d)
    _note('delay raster', 'host', h['median_ms'], 'device', d['median_ms'])
    p.unlink()
    del delay
    # ---- 2c. cubes
    z, y, x = np.meshgrid(np.linspace(0, 9000, 20), np.linspace(34, 33, M), np.linspace(-118, -117, M), indexing='ij')
    cube64 = 2.3 * np.exp(-z / 8000.0) * (1 + 0.05 * np.sin(8 * x) * np.cos(9 * y)) + 1e-5 * rng.standard_normal(z.shape)
    del z, y, x
    out['cubes'] = {}
    for dt in (np.float32, np.float64):
        cube = cube64.astype(dt)
        t = torch.from_numpy(cube).to(dev)
        rows, pairs = [], []
        for div in (2, 4, 8):
            chunks = (20, -(-M // div), -(-M // div))
            packed, offsets = deflate.compress_chunks(t, chunks, np.nan, shuffle=True)
            p = tmp / 'cube.h5'
            h5write.write_hdf5(p, [('wet', h5write.ChunkedData(cube.shape, cube.dtype, chunks, packed, offsets), [('units', 'm')], None)])

            def host_fn():
                f = h5lite.File(p)
                return torch.from_numpy(f['wet'].read()).to(dev)

            def dev_fn():
                f = h5lite.File(p)
                return f['wet'].read_device(device=dev, inflate='device')
            same = bool(torch.equal(host_fn(), dev_fn())) and dev_fn().cpu().numpy().tobytes() == cube.tobytes()
            h, d = alternate(host_fn, dev_fn)
            rows.append(dict(chunks=div * div, file_bytes=p.stat().st_size, decoded_bytes=int(cube.nbytes), identical=same, host=h, device=d))
            pairs.append((div * div, h, d))
            _note('cube', np.dtype(dt).name, div * div, 'host', h['median_ms'], 'device', d['median_ms'])
            p.unlink()
        out['cubes'][np.dtype(dt).name] = dict(rows=rows, crossover_chunks=crossover(pairs))
        del t
    if not a.probe:
        probe.unlink()
    tmp.rmdir()
    print(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
