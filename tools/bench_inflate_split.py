"""The split inflater against the serial kernel and host zlib, from path (or host bytes) to device tensor, in one process.

Three routes per input, alternated call by call: 'host' (zlib.decompress stream by stream, then the upload - inflate='host'), 'serial'
(the device route with split=False: rdr_inflate_decode, one wave per stream) and 'split' (the device route as the readers take it:
rdr_inflate_decode_split).  The serial route is the readers' own code with deflate.inflate_segments wrapped so that the keyword is
dropped.  Every route's result is compared bit for bit before it is timed; host clocks around work that ends in a device synchronise;
warm-up calls, then `--reps` alternated repeats; medians with spans.  `ahead_of_host` is true when the split route's median lies below
the host route's by more than both spans (max - min of either route's repeats).  No process is started once the device is open: the
DEM tiles are compressed by a process pool in front of `import torch`, chunks compressed later by threads (zlib releases the GIL).

Inputs: 20 x M x M float32 and float64 cubes chunked as DelayCube.to_netcdf(compress=True) chunks them (delay.gunw_chunks: a third
of each horizontal axis), tables fixed and dynamic; one stream of `--mb` MB from the device encoder; an N x N float32 raster in 16 deflate strips from the
device encoder; and the many-stream inputs of tools/bench_inflate.py (the int16 DEM in 256 host-zlib tiles, the float32 raster in N / 4
device-written strips, the float32 cube in 64 host-zlib chunks), which show what the split route costs where there is little to split;
and three small files around the readers' 'auto' thresholds: a 20 x 150 x 150 float32 cube in nine device-written chunks (about 64
chunks + flush points), the same cube in nine host-zlib chunks with a Z_SYNC_FLUSH every 32 KiB (the same count, but every piece
depends on the one before: measure pass, then the serial kernel) and float32 rasters of 8 to 48 MB in 8 or 16 device-written strips
(about 256, 500, 750, 1000 and 1500).

    python tools/bench_inflate_split.py [--size 4000] [--cube 1000] [--mb 32] [--reps 3] [--warmup 1] --out profiles/r28_inflate_split.json
    python tools/bench_inflate_split.py --trace-only     # the float32 cube through the split route alone, for a kernel trace
"""
import argparse
import json
import statistics
import sys
import tempfile
import time
import zlib
from concurrent.futures import ProcessPoolExecutor, ThreadPoolExecutor
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / 'tools'))


def _summary(ms):
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), repeats_ms=[round(v, 3) for v in ms])


def _note(*what):
    print('[bench_inflate_split]', *what, file=sys.stderr, flush=True)


def _z6(b):
    return zlib.compress(b, 6)


def _z6_sync(b, step=32768):
    """zlib level 6 with a Z_SYNC_FLUSH every `step` bytes: the marker, and the history kept across it"""
    c = zlib.compressobj(6)
    return b''.join(c.compress(b[o:o + step]) + c.flush(zlib.Z_SYNC_FLUSH) for o in range(0, len(b), step)) + c.flush()


def _ahead(a, b):
    """route a is ahead of route b: its median is lower by more than both spans"""
    return b['median_ms'] - a['median_ms'] > max(a['max_ms'] - a['min_ms'], b['max_ms'] - b['min_ms'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=4000)
    ap.add_argument('--cube', type=int, default=1000)
    ap.add_argument('--mb', type=int, default=32)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--trace-only', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    N, M = a.size, a.cube
    rng = np.random.default_rng(19)
    tmp = Path(tempfile.mkdtemp(prefix='bench_inflate_split_'))
    z, y, x = np.meshgrid(np.linspace(0, 9000, 20), np.linspace(34, 33, M), np.linspace(-118, -117, M), indexing='ij')
    cube64 = 2.3 * np.exp(-z / 8000.0) * (1 + 0.05 * np.sin(8 * x) * np.cos(9 * y)) + 1e-5 * rng.standard_normal(z.shape)
    del z, y, x
    dem_file = None
    if not a.trace_only:                                          # everything the host encodes, before anything touches the GPU
        from bench_inflate import write_deflate_tiles
        yy, xx = np.meshgrid(np.arange(N), np.arange(N), indexing='ij')
        dem = (1500 + 900 * np.sin(xx / 310.0) * np.cos(yy / 270.0) + 300 * np.sin((xx + 2 * yy) / 47.0) + rng.normal(0, 3, (N, N))).astype(np.int16)
        del yy, xx
        dem_file = tmp / 'dem.tif'
        with ProcessPoolExecutor(16) as pool:
            ntiles = write_deflate_tiles(dem_file, dem, 256, pool)

    import torch
    from raider_amd import _lib, deflate, h5lite, h5write, tifflite
    from raider_amd.delay import gunw_chunks
    dev = torch.device('cuda:0')
    name, cus, _ = _lib.Context.default().device_info()
    real = deflate.inflate_segments
    rows = []

    def serially(fn):
        """fn with the device route's decode forced to split=False"""
        def run():
            deflate.inflate_segments = lambda *k, **kw: real(*k, **{**kw, 'split': False})
            try:
                return fn()
            finally:
                deflate.inflate_segments = real
        return run

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def three(label, host_fn, dev_fn, want, **info):
        routes = dict(host=host_fn, serial=serially(dev_fn), split=dev_fn)
        got = {k: f() for k, f in routes.items()}
        p = deflate.last_pieces()
        same = all(g.cpu().numpy().tobytes() == want for g in got.values())
        del got
        for _ in range(a.warmup):
            for f in routes.values():
                clock(f)
        ms = {k: [] for k in routes}
        for _ in range(a.reps):
            for k, f in routes.items():
                ms[k].append(clock(f)[0])
        row = dict(input=label, identical=same, streams=int(p.size), pieces_min=int(p.min()), pieces_max=int(p.max()), pieces_total=int(p.sum()),
                   **info, **{k: _summary(v) for k, v in ms.items()})
        row['ahead_of_host'] = _ahead(row['split'], row['host'])
        row['ahead_of_serial'] = _ahead(row['split'], row['serial'])
        _note(label, 'pieces', row['pieces_total'], *(f"{k} {row[k]['median_ms']}" for k in routes), 'identical', same)
        rows.append(row)
        if a.out:                                                 # (row by row: a run that is cut short leaves what it measured)
            Path(a.out).parent.mkdir(parents=True, exist_ok=True)
            Path(a.out).write_text(json.dumps(dict(out, rows=rows), indent=1) + '\n')

    def cube_routes(cube, chunks, tables, host_zlib=None):
        p = tmp / 'cube.h5'
        if host_zlib:
            raw = deflate.h5_chunks_host(cube, chunks, np.nan, shuffle=True)
            n = int(np.prod(deflate.chunk_grid(cube.shape, chunks)))
            cb = raw.size // n
            with ThreadPoolExecutor(16) as pool:                  # (threads: the device is open, no process is started from here on)
                parts = list(pool.map(host_zlib, [raw[k * cb:(k + 1) * cb].tobytes() for k in range(n)]))
            packed, offsets = np.frombuffer(b''.join(parts), dtype=np.uint8), np.cumsum([0] + [len(s) for s in parts])
        else:
            packed, offsets = deflate.compress_chunks(torch.from_numpy(cube).to(dev), chunks, np.nan, shuffle=True, tables=tables)
        h5write.write_hdf5(p, [('wet', h5write.ChunkedData(cube.shape, cube.dtype, chunks, packed, offsets), [('units', 'm')], None)])
        host_fn = lambda: torch.from_numpy(h5lite.File(p)['wet'].read()).to(dev)
        dev_fn = lambda: h5lite.File(p)['wet'].read_device(device=dev, inflate='device')
        return p, host_fn, dev_fn

    if a.trace_only:
        cube = cube64.astype(np.float32)
        p, _, dev_fn = cube_routes(cube, gunw_chunks(cube.shape), 'fixed')
        for _ in range(3):
            clock(dev_fn)
        p.unlink(); tmp.rmdir()
        return

    out = dict(tool='bench_inflate_split', device=name, compute_units=cus, source_hash=_lib.load().rdr_source_hash().decode(), zlib=zlib.ZLIB_RUNTIME_VERSION,
               torch=torch.__version__, size=N, cube=[20, M, M], mb=a.mb, reps=a.reps, warmup=a.warmup,
               timing='host clock around calls that end in torch.cuda.synchronize(); the three routes alternate call by call',
               routes="host: inflate='host' (zlib, then the upload); serial: the device route with split=False (rdr_inflate_decode); split: the device route "
                      "(rdr_inflate_decode_split)")
    # ---- the cubes in their GUNW chunks
    for dt in (np.float32, np.float64):
        cube = cube64.astype(dt)
        for tables in ('fixed', 'dynamic'):
            p, host_fn, dev_fn = cube_routes(cube, gunw_chunks(cube.shape), tables)
            three(f'cube {np.dtype(dt).name} GUNW chunks, {tables}', host_fn, dev_fn, cube.tobytes(), file_bytes=p.stat().st_size, decoded_bytes=int(cube.nbytes))
            p.unlink()
    # ---- one long stream from the device encoder
    flat = np.ascontiguousarray(cube64.astype(np.float32)).view(np.uint8).reshape(-1)[:a.mb << 20]
    flat = np.ascontiguousarray(flat.reshape(-1, 4).T).reshape(-1)                   # shuffled, as a chunk is
    packed, oo = deflate.deflate_segments(torch.from_numpy(flat).to(dev), [0], [flat.size])
    stream = packed.cpu().numpy()
    sbytes = stream.tobytes()
    host_fn = lambda: torch.from_numpy(np.frombuffer(zlib.decompress(sbytes), dtype=np.uint8)).to(dev)
    dev_fn = lambda: deflate.inflate_segments(torch.from_numpy(stream).to(dev), [0], [stream.size], [flat.size], split=True)[0][:flat.size]
    three(f'one stream of {a.mb} MB from the device encoder', host_fn, dev_fn, flat.tobytes(), compressed_bytes=int(stream.size), decoded_bytes=int(flat.size))
    # ---- rasters from the device encoder: 16 strips, and N / 4
    yy, xx = np.meshgrid(np.linspace(0, 6, N), np.linspace(0, 5, N), indexing='ij')
    delay = (2.3 + 0.2 * np.sin(xx) * np.cos(yy) + 1e-4 * rng.standard_normal((N, N))).astype(np.float32)
    del yy, xx
    for rps in (-(-N // 16), 4):
        p = tmp / 'delay.tif'
        tifflite.write(p, delay, compress='deflate', rows_per_strip=rps, predictor=2, encoder='device')
        host_fn = lambda: tifflite.read(p, band=1, device=dev, inflate='host')[0]
        dev_fn = lambda: tifflite.read(p, band=1, device=dev, inflate='device')[0]
        three(f'raster float32 in {len(tifflite.TiffInfo(p).offsets)} strips from the device encoder', host_fn, dev_fn, delay.tobytes(), file_bytes=p.stat().st_size)
        p.unlink()
    # ---- host-zlib files: nothing to split
    host_fn = lambda: tifflite.read(dem_file, band=1, device=dev, inflate='host')[0]
    dev_fn = lambda: tifflite.read(dem_file, band=1, device=dev, inflate='device')[0]
    three(f'DEM int16 in {ntiles} host-zlib tiles', host_fn, dev_fn, dem.tobytes(), file_bytes=dem_file.stat().st_size)
    dem_file.unlink()
    cube = cube64.astype(np.float32)
    p, host_fn, dev_fn = cube_routes(cube, (20, -(-M // 8), -(-M // 8)), 'fixed', host_zlib=_z6)
    three('cube float32 in 64 host-zlib chunks', host_fn, dev_fn, cube.tobytes(), file_bytes=p.stat().st_size)
    p.unlink()
    # ---- around the readers' thresholds: chunks / segments + flush points near 64 and 256
    small = np.ascontiguousarray(cube[:, :150, :150])
    for label, kw in (('nine device-written chunks', {}), ('nine host-zlib chunks, Z_SYNC_FLUSH every 32 KiB', dict(host_zlib=_z6_sync))):
        p, host_fn, dev_fn = cube_routes(small, gunw_chunks(small.shape), 'fixed', **kw)
        ds = h5lite.File(p)['wet']
        units = sum(1 + deflate.flush_points(bytes(ds.file.buf[ds.file.base + addr:ds.file.base + addr + size])) for _, size, _, addr, _ in ds._chunks(ds.layout, ds.shape)[1])
        three(f'cube float32 20 x 150 x 150 in {label}', host_fn, dev_fn, small.tobytes(), file_bytes=p.stat().st_size, units=units)
        p.unlink()
    for rows_, cols, nstrips in ((2048, 1000, 8), (1024, 4000, 16), (1536, 4000, 16), (2048, 4000, 16), (3072, 4000, 16)):
        strip = np.ascontiguousarray(delay[:rows_, :cols])
        p = tmp / 'strip.tif'
        tifflite.write(p, strip, compress='deflate', rows_per_strip=rows_ // nstrips, predictor=2, encoder='device')
        host_fn = lambda: tifflite.read(p, band=1, device=dev, inflate='host')[0]
        dev_fn = lambda: tifflite.read(p, band=1, device=dev, inflate='device')[0]
        three(f'raster float32 {rows_} x {cols} in {nstrips} strips from the device encoder', host_fn, dev_fn, strip.tobytes(), file_bytes=p.stat().st_size,
              units=tifflite._inflate_units(tifflite.TiffInfo(p)))
        p.unlink()
    tmp.rmdir()
    out['rows'] = rows
    print(json.dumps(out))


if __name__ == '__main__':
    main()
