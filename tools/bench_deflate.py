"""Delay rasters and cubes deflated on the device (rdr_deflate_encode) against the host route (zlib level 6, what writeDelays used
before and still uses without a GPU).

Three measurements, each a host clock around work that ends with the file on disk or in a device synchronise; `warmup` untimed calls
first, then `reps` calls with the two sides alternated; median, minimum, maximum:
  1. two N x N float32 delay rasters through utilFcns._write_delay_raster: the device route (predictor 2, one encode call per raster)
     and the host route (utilFcns._gpu_visible patched to False: byte for byte the parent commit's path); seconds and file bytes;
  2. the encoder alone, device tensor to device tensor, in GB/s of input: the rasters' predictor-2 strips and the shuffled chunks of
     a (20, M, M) float64 cube; for each input the size ratio against zlib level 1 and against zlib's fixed-table encoder (Z_FIXED)
     in the same 32 KiB sub-blocks;
  3. DelayCube.to_netcdf of that cube with and without compress.
It also records the encoder's size excess over zlib Z_FIXED on the three inputs of tests/test_gpu_deflate.py's ratio test: the test's
margin is that excess plus 0.05.  The yardstick is recorded, not asserted.

    python tools/bench_deflate.py [--size 4000] [--cube 1000] [--reps 5] [--warmup 1] --out profiles/r22_deflate.json

--tables runs another study in place of the three above: the encoder's dynamic-table mode (tables='dynamic') against its fixed mode.
For the four inputs of DESIGN.md 7 at workload size (predictor-2 and plain float32 raster strips, shuffled float32 and float64 cube
chunks) and the inputs of tests/test_gpu_deflate_dynamic.py's ratio test: the device's bytes in both modes, zlib Z_FIXED and zlib
level 1 (default strategy) in 32 KiB sub-blocks, zlib level 1 on whole segments, the block counts, and the encoder's GB/s in both
modes (device tensor to device tensor, the two modes alternated).  With --ab-parent-lib (the library built from the parent commit) it
also alternates the two libraries, three times, one fresh process per turn, on rdr_deflate_encode (the default, fixed path), and records
medians and spans: the default path's median must lie inside the parent's span.

    python tools/bench_deflate.py --tables [--ab-parent-lib parent/libraider_hip.so] --out profiles/r23_deflate_dynamic.json
"""
import argparse
import json
import statistics
import sys
import tempfile
import time
import zlib
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
SUB = 32768


def _summary(s):
    return dict(median_s=statistics.median(s), min_s=min(s), max_s=max(s), repeats_s=[round(v, 5) for v in s])


def zfixed_size(data):
    """zlib's fixed-table encoder at level 1 over independent 32 KiB sub-blocks, each stored when that is smaller."""
    total = 6
    for o in range(0, len(data), SUB):
        part = data[o:o + SUB]
        co = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
        total += min(len(co.compress(part) + co.flush(zlib.Z_SYNC_FLUSH)), len(part) + 5)
    return total


def ratios(segs, device_bytes):
    """Input bytes over output bytes for the device encoder, zlib level 1 and zlib Z_FIXED in sub-blocks, over a sample of `segs`."""
    n = sum(len(s) for s in segs)
    z1 = sum(len(zlib.compress(s, 1)) for s in segs)
    zf = sum(zfixed_size(s) for s in segs)
    return dict(input_bytes=n, device_bytes=device_bytes, zlib1_bytes=z1, zlib_fixed_bytes=zf, ratio_device=n / device_bytes, ratio_zlib1=n / z1,
                ratio_zlib_fixed=n / zf, device_over_zlib1=device_bytes / z1, device_over_zlib_fixed=device_bytes / zf)


def zlib1_size(data):
    """zlib level 1, default strategy, over independent 32 KiB sub-blocks closed with Z_SYNC_FLUSH, each stored when that is smaller."""
    total = 6
    for o in range(0, len(data), SUB):
        part = data[o:o + SUB]
        co = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY)
        total += min(len(co.compress(part) + co.flush(zlib.Z_SYNC_FLUSH)), len(part) + 5)
    return total


def _workload_inputs(N, M):
    """{label: (bytes as a NumPy uint8 array, offsets, sizes)}: the four inputs of DESIGN.md 7."""
    from raider_amd import deflate
    from raider_amd.delay import gunw_chunks
    yy, xx = np.meshgrid(np.arange(N, dtype=np.float32), np.arange(N, dtype=np.float32), indexing='ij')
    wet = (0.15 + 0.1 * np.sin(xx / 310.0) * np.cos(yy / 270.0) + 0.02 * np.sin((xx + 2 * yy) / 47.0)).astype(np.float32)
    wet[:N // 16] = 0.0
    del yy, xx
    row = N * 4
    rps = max(1, (1 << 16) // row)
    offs = np.arange(0, N, rps, dtype=np.int64) * row
    sizes = np.minimum(rps, N - np.arange(0, N, rps, dtype=np.int64)) * row
    p2 = wet.view(np.uint32).copy()
    p2[:, 1:] -= wet.view(np.uint32)[:, :-1]
    out = {'raster_f32_predictor2_strips': (p2.reshape(-1).view(np.uint8), offs, sizes), 'raster_f32_plain_strips': (wet.reshape(-1).view(np.uint8), offs, sizes)}
    z, y, x = np.meshgrid(np.linspace(0, 15000, 20), np.arange(M, dtype=np.float64), np.arange(M, dtype=np.float64), indexing='ij')
    cw = 0.3 * np.exp(-z / 2000.0) * (1 + 0.05 * np.sin(x / 90.0) * np.cos(y / 70.0))
    del z, y, x
    chunks = gunw_chunks(cw.shape)
    n = int(np.prod(deflate.chunk_grid(cw.shape, chunks)))
    for label, arr in (('cube_f32_shuffled_chunks', cw.astype(np.float32)), ('cube_f64_shuffled_chunks', cw)):
        raw = deflate.h5_chunks_host(arr, chunks, np.nan, True)
        cb = raw.size // n
        out[label] = (raw, np.arange(n, dtype=np.int64) * cb, np.full(n, cb, dtype=np.int64))
    return out


def ab_child(a):
    """One turn of the A/B: rdr_deflate_encode of the library at --ab-child (device tensor to device tensor) through ctypes alone, so
    that a library without the newer entry points loads; one JSON line."""
    import ctypes as C
    import hashlib
    import torch
    lib = C.CDLL(a.ab_child)
    VP, I64 = C.c_void_p, C.c_int64
    lib.rdr_create.argtypes = [C.c_int, C.POINTER(VP)]
    lib.rdr_deflate_bound.restype = I64; lib.rdr_deflate_bound.argtypes = [I64]
    lib.rdr_deflate_encode.argtypes = [VP, VP, I64, VP, VP, I64, VP, I64, VP, C.c_int]
    lib.rdr_destroy.argtypes = [VP]
    ctx = VP()
    assert lib.rdr_create(0, C.byref(ctx)) == 0
    res = {}
    for label, (buf, offs, sizes) in _workload_inputs(a.size, a.cube).items():
        if label not in ('raster_f32_predictor2_strips', 'cube_f64_shuffled_chunks'):
            continue
        src = torch.from_numpy(buf).cuda()
        cap = int(sum(lib.rdr_deflate_bound(int(v)) * int(c) for v, c in zip(*np.unique(sizes, return_counts=True))))
        out = torch.empty(cap, dtype=torch.uint8, device='cuda')
        oo = np.zeros(offs.size + 1, dtype=np.int64)
        ts = []
        for k in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc = lib.rdr_deflate_encode(ctx, src.data_ptr(), buf.size, offs.ctypes.data, sizes.ctypes.data, offs.size, out.data_ptr(), cap, oo.ctypes.data, 1)
            torch.cuda.synchronize()
            assert rc == 0
            if k >= a.warmup:
                ts.append(time.perf_counter() - t0)
        res[label] = dict(input_bytes=int(buf.size), output_bytes=int(oo[-1]), sha256=hashlib.sha256(out[:int(oo[-1])].cpu().numpy().tobytes()).hexdigest(), **_summary(ts))
    lib.rdr_destroy(ctx)
    print(json.dumps(res))


def tables_study(a):
    import subprocess
    import torch
    from raider_amd import _lib, deflate
    from tests import test_gpu_deflate_dynamic as T
    name, cus, _ = _lib.Context.default().device_info()
    out = dict(tool='bench_deflate --tables', device=name, compute_units=cus, source_hash=_lib.load().rdr_source_hash().decode(), torch=torch.__version__,
               zlib=zlib.ZLIB_VERSION, reps=a.reps, warmup=a.warmup,
               timing='host clock around deflate_segments, device tensor to device tensor, ended by torch.cuda.synchronize(); the two modes alternate call by call',
               sizes='zlib figures of the workload inputs are over a sample of at most 64 segments, with the device bytes of the same segments beside them')

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r

    def study(buf, offs, sizes, timed):
        src = torch.from_numpy(np.ascontiguousarray(buf)).cuda()
        ts, got = {'fixed': [], 'dynamic': []}, {}
        for k in range((a.warmup + a.reps) if timed else 1):
            for mode in ('fixed', 'dynamic'):
                s, (packed, oo) = clock(lambda: deflate.deflate_segments(src, offs, sizes, tables=mode))
                if k >= a.warmup or not timed:
                    ts[mode].append(s)
                got[mode] = (oo.copy(), deflate.last_block_counts(), packed)
        pick = list(range(0, len(offs), max(1, len(offs) // 64)))[:64]
        segs = [buf[offs[i]:offs[i] + sizes[i]].tobytes() for i in pick]
        r = dict(input_bytes=int(buf.size), segments=int(len(offs)), sample_segments=len(pick), sample_input_bytes=sum(len(s) for s in segs),
                 sample_zlib_fixed_bytes=sum(zfixed_size(s) for s in segs), sample_zlib1_sub_block_bytes=sum(zlib1_size(s) for s in segs),
                 sample_zlib1_whole_segment_bytes=sum(len(zlib.compress(s, 1)) for s in segs))
        for mode in ('fixed', 'dynamic'):
            oo, counts, packed = got[mode]
            r[f'device_{mode}_bytes'] = int(oo[-1])
            r[f'sample_device_{mode}_bytes'] = int(sum(oo[i + 1] - oo[i] for i in pick))
            r[f'blocks_stored_fixed_dynamic_{mode}'] = list(counts)
            if timed:
                r[f'gb_per_s_median_{mode}'] = buf.size / statistics.median(ts[mode]) / 1e9
                r[f'time_{mode}'] = _summary(ts[mode])
        host = got['dynamic'][2].cpu().numpy(); oo = got['dynamic'][0]
        r['dynamic_sample_decodes'] = all(zlib.decompress(host[oo[i]:oo[i + 1]].tobytes()) == s for i, s in zip(pick, segs))
        r['ratio_device_fixed'] = r['sample_input_bytes'] / r['sample_device_fixed_bytes']
        r['ratio_device_dynamic'] = r['sample_input_bytes'] / r['sample_device_dynamic_bytes']
        r['ratio_zlib_fixed'] = r['sample_input_bytes'] / r['sample_zlib_fixed_bytes']
        r['ratio_zlib1_sub_block'] = r['sample_input_bytes'] / r['sample_zlib1_sub_block_bytes']
        r['dynamic_excess_over_zlib1_sub_block'] = r['sample_device_dynamic_bytes'] / r['sample_zlib1_sub_block_bytes'] - 1.0
        return r

    out['workload_inputs'] = {label: study(buf, offs, sizes, True) for label, (buf, offs, sizes) in _workload_inputs(a.size, a.cube).items()}
    table = {}
    for which in ('cube_f32', 'cube_f64', 'raster_p2', 'alpha4'):
        segs = T._ratio_input(which)
        buf = np.frombuffer(b''.join(segs), dtype=np.uint8)
        sz = np.array([len(s) for s in segs], dtype=np.int64)
        table[which] = study(buf, np.cumsum(np.concatenate([[0], sz[:-1]])).astype(np.int64), sz, False)
    out['ratio_test_inputs'] = table
    # the files: a float32 delay raster (predictor 2) and a float64 delay cube written with either tables, the modes alternated
    import tempfile as _tf
    from raider_amd import tifflite
    from raider_amd.delay import DelayCube
    tmp = Path(_tf.mkdtemp(prefix='bench_deflate_tables_'))
    N, M = a.size, a.cube
    yy, xx = np.meshgrid(np.arange(N, dtype=np.float32), np.arange(N, dtype=np.float32), indexing='ij')
    wet = (0.15 + 0.1 * np.sin(xx / 310.0) * np.cos(yy / 270.0) + 0.02 * np.sin((xx + 2 * yy) / 47.0)).astype(np.float32)
    wet[:N // 16] = 0.0
    del yy, xx
    z, y, x = np.meshgrid(np.linspace(0, 15000, 20), np.arange(M, dtype=np.float64), np.arange(M, dtype=np.float64), indexing='ij')
    cube = DelayCube({'wet': 0.3 * np.exp(-z / 2000.0) * (1 + 0.05 * np.sin(x / 90.0) * np.cos(y / 70.0)), 'hydro': 2.3 * np.exp(-z / 8000.0) * (1 + 0.001 * np.sin(x / 300.0)),
                      'z': np.linspace(0, 15000, 20), 'y': np.linspace(35, 33, M), 'x': np.linspace(-118, -116, M)}, {'description': 'RAiDER geo cube - ray tracing'})
    del z, y, x
    writers = {'delay_raster_f32_predictor2_tif': lambda mode: tifflite.write(tmp / 'r.tif', wet, compress='deflate', predictor=2, encoder='device', tables=mode),
               'delay_cube_f64_netcdf': lambda mode: cube.to_netcdf(tmp / 'c.nc', compress=True, tables=mode)}
    files = {}
    for label, fn in writers.items():
        ts, size = {'fixed': [], 'dynamic': []}, {}
        for k in range(a.warmup + a.reps):
            for mode in ('fixed', 'dynamic'):
                s, _ = clock(lambda: fn(mode))
                if k >= a.warmup:
                    ts[mode].append(s)
                size[mode] = (tmp / ('r.tif' if 'tif' in label else 'c.nc')).stat().st_size
        files[label] = {mode: dict(file_bytes=size[mode], **_summary(ts[mode])) for mode in ('fixed', 'dynamic')}
    files['delay_raster_f32_predictor2_tif']['shape'] = [N, N]; files['delay_cube_f64_netcdf']['shape'] = [20, M, M]
    out['files'] = files
    for p in tmp.iterdir():
        p.unlink()
    tmp.rmdir()
    del wet, cube
    if a.ab_parent_lib:
        turns = {'parent': [], 'new': []}
        for _ in range(3):
            for side, lib in (('parent', a.ab_parent_lib), ('new', str(_lib.LIB_PATH))):
                r = subprocess.run([sys.executable, __file__, '--ab-child', lib, '--size', str(a.size), '--cube', str(a.cube), '--reps', str(a.reps), '--warmup', str(a.warmup)],
                                   capture_output=True, text=True, check=True)
                turns[side].append(json.loads(r.stdout.strip().splitlines()[-1]))
        ab = {}
        for label in turns['new'][0]:
            e = {}
            for side in ('parent', 'new'):
                med = [t[label]['median_s'] for t in turns[side]]
                e[side] = dict(turn_medians_s=med, median_s=statistics.median(med), span_s=[min(t[label]['min_s'] for t in turns[side]), max(t[label]['max_s'] for t in turns[side])],
                               span_of_turn_medians_s=[min(med), max(med)], output_bytes=turns[side][0][label]['output_bytes'], sha256=turns[side][0][label]['sha256'])
            e['same_bytes'] = e['parent']['sha256'] == e['new']['sha256']
            e['new_median_inside_parent_span'] = e['parent']['span_s'][0] <= e['new']['median_s'] <= e['parent']['span_s'][1]
            e['new_over_parent_median'] = e['new']['median_s'] / e['parent']['median_s']
            ab[label] = e
        out['ab_default_path_against_parent_library'] = dict(entry='rdr_deflate_encode', alternations=3, process='a fresh process per turn', **ab)
    print(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tables', action='store_true', help='the dynamic-table study in place of the three measurements')
    ap.add_argument('--ab-parent-lib', default=None, help='with --tables: the library built from the parent commit, for the A/B of the default path')
    ap.add_argument('--ab-child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--size', type=int, default=4000)
    ap.add_argument('--cube', type=int, default=1000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    if a.ab_child:
        return ab_child(a)
    if a.tables:
        return tables_study(a)
    import torch
    from raider_amd import _lib, deflate, tifflite, utilFcns
    from raider_amd.delay import DelayCube, gunw_chunks
    from tests import test_gpu_deflate as T
    dev = torch.device('cuda:0')
    N, M = a.size, a.cube
    yy, xx = np.meshgrid(np.arange(N, dtype=np.float32), np.arange(N, dtype=np.float32), indexing='ij')
    wet = (0.15 + 0.1 * np.sin(xx / 310.0) * np.cos(yy / 270.0) + 0.02 * np.sin((xx + 2 * yy) / 47.0)).astype(np.float32)
    hyd = (2.2 + 0.1 * np.cos(xx / 900.0) + 0.05 * np.sin(yy / 700.0)).astype(np.float32)
    wet[:N // 16] = 0.0; hyd[:N // 16] = 0.0                      # the no-data band
    del yy, xx
    tmp = Path(tempfile.mkdtemp(prefix='bench_deflate_'))
    gt = (-118.0, 1.0 / 3600, 0.0, 35.0, 0.0, -1.0 / 3600)
    name, cus, _ = _lib.Context.default().device_info()
    out = dict(tool='bench_deflate', device=name, compute_units=cus, source_hash=_lib.load().rdr_source_hash().decode(), torch=torch.__version__, zlib=zlib.ZLIB_VERSION,
               reps=a.reps, warmup=a.warmup, timing='host clock around calls that end with the file written / torch.cuda.synchronize(); the two sides alternate call by call')

    # ---- 1. the raster route
    def route(device):
        vis = utilFcns._gpu_visible
        utilFcns._gpu_visible = (lambda: True) if device else (lambda: False)
        try:
            t0 = time.perf_counter()
            utilFcns._write_delay_raster(wet, tmp / 'wet.tif', 0.0, 'GTiff', 'EPSG:4326', gt)
            utilFcns._write_delay_raster(hyd, tmp / 'hydro.tif', 0.0, 'GTiff', 'EPSG:4326', gt)
            return time.perf_counter() - t0, (tmp / 'wet.tif').stat().st_size + (tmp / 'hydro.tif').stat().st_size
        finally:
            utilFcns._gpu_visible = vis
    for _ in range(a.warmup):
        route(True)
    td, th, size_d, size_h = [], [], 0, 0
    for k in range(a.reps):
        s, size_d = route(True); td.append(s)
        same = bool(np.array_equal(tifflite.read(tmp / 'wet.tif')[0], wet) and np.array_equal(tifflite.read(tmp / 'hydro.tif')[0], hyd)) if k == 0 else same
        if k < max(2, a.reps // 2):                                # (the host route takes seconds per call)
            s, size_h = route(False); th.append(s)
    out['write_delay_rasters'] = dict(rasters=2, shape=[N, N], dtype='float32', raster_bytes=int(wet.nbytes + hyd.nbytes), pixels_read_back_identical=same,
                                      device_route=dict(file_bytes=size_d, **_summary(td)), host_route_as_parent_commit=dict(file_bytes=size_h, **_summary(th)),
                                      speedup_median=statistics.median(th) / statistics.median(td))

    # ---- 2. the encoder alone
    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, r
    ctx = _lib.Context.default()
    row = N * 4
    rps = max(1, (1 << 16) // row)
    offs = np.arange(0, N, rps, dtype=np.int64) * row
    sizes = np.minimum(rps, N - np.arange(0, N, rps, dtype=np.int64)) * row
    enc = {}
    for label, arr in (('wet_raster_predictor2_strips', wet), ('hydro_raster_predictor2_strips', hyd)):
        t = torch.from_numpy(arr).to(dev).reshape(-1).view(torch.uint8)
        d = torch.empty_like(t)
        _lib.check(ctx.lib.rdr_tiff_predict(ctx.handle, _lib.ptr(t), 4, N, N, _lib.ptr(d), _lib.RDR_DEVICE), ctx.handle)
        for _ in range(a.warmup):
            clock(lambda: deflate.deflate_segments(d, offs, sizes))
        ts = []
        for _ in range(a.reps):
            s, (packed, oo) = clock(lambda: deflate.deflate_segments(d, offs, sizes)); ts.append(s)
        host = d.cpu().numpy()
        pick = list(range(0, offs.size, max(1, offs.size // 64)))                 # the ratios over a sample of 64 strips
        segs = [host[offs[i]:offs[i] + sizes[i]].tobytes() for i in pick]
        dev_bytes = int(sum(oo[i + 1] - oo[i] for i in pick))
        enc[label] = dict(input_bytes=int(t.numel()), output_bytes=int(oo[-1]), segments=int(offs.size), gb_per_s_median=t.numel() / statistics.median(ts) / 1e9,
                          ratio_whole_input=t.numel() / int(oo[-1]), sample_of_strips=ratios(segs, dev_bytes), **_summary(ts))
    z, y, x = np.meshgrid(np.linspace(0, 15000, 20), np.arange(M, dtype=np.float64), np.arange(M, dtype=np.float64), indexing='ij')
    cw = 0.3 * np.exp(-z / 2000.0) * (1 + 0.05 * np.sin(x / 90.0) * np.cos(y / 70.0))
    ch = 2.3 * np.exp(-z / 8000.0) * (1 + 0.001 * np.sin(x / 300.0))
    del z, y, x
    chunks = gunw_chunks(cw.shape)
    raw = deflate.h5_chunks(torch.from_numpy(cw).to(dev), chunks, np.nan, True)
    nchunk = int(np.prod(deflate.chunk_grid(cw.shape, chunks)))
    cb = raw.numel() // nchunk
    coffs, csizes = np.arange(nchunk, dtype=np.int64) * cb, np.full(nchunk, cb, dtype=np.int64)
    for _ in range(a.warmup):
        clock(lambda: deflate.deflate_segments(raw, coffs, csizes))
    ts = []
    for _ in range(a.reps):
        s, (packed, oo) = clock(lambda: deflate.deflate_segments(raw, coffs, csizes)); ts.append(s)
    seg0 = raw[:cb].cpu().numpy().tobytes()
    enc['f64_cube_shuffled_chunks'] = dict(input_bytes=int(raw.numel()), output_bytes=int(oo[-1]), segments=nchunk, chunks=list(chunks),
                                           gb_per_s_median=raw.numel() / statistics.median(ts) / 1e9, ratio_whole_input=raw.numel() / int(oo[-1]),
                                           first_chunk=ratios([seg0], int(oo[1] - oo[0])), **_summary(ts))
    del raw
    out['encoder_only'] = enc

    # ---- 3. the cube file
    cube = DelayCube({'wet': cw, 'hydro': ch, 'z': np.linspace(0, 15000, 20), 'y': np.linspace(35, 33, M), 'x': np.linspace(-118, -116, M)},
                     {'description': 'RAiDER geo cube - ray tracing'})

    def cube_file(compress):
        t0 = time.perf_counter()
        cube.to_netcdf(tmp / 'cube.nc', compress=compress)
        return time.perf_counter() - t0, (tmp / 'cube.nc').stat().st_size
    for _ in range(a.warmup):
        cube_file(True); cube_file(False)
    tc, tu = [], []
    for _ in range(a.reps):
        s, size_c = cube_file(True); tc.append(s)
        s, size_u = cube_file(False); tu.append(s)
    out['delay_cube_to_netcdf'] = dict(shape=list(cw.shape), dtype='float64', chunks=list(chunks), compressed=dict(file_bytes=size_c, **_summary(tc)),
                                       uncompressed=dict(file_bytes=size_u, **_summary(tu)))

    # ---- the inputs of the ratio test: the excess its margin is taken from
    excess = {}
    for which in ('cube_f32', 'cube_f64', 'raster_p2'):
        segs = T.ratio_segments(which)
        buf = np.frombuffer(b''.join(segs), dtype=np.uint8)
        sz = [len(s) for s in segs]
        packed, oo = deflate.deflate_segments(buf, np.cumsum([0] + sz[:-1]), sz)
        excess[which] = dict(excess_over_zlib_fixed=packed.size / sum(zfixed_size(s) for s in segs) - 1.0, **ratios(segs, int(packed.size)))
    out['ratio_test_inputs'] = excess
    for p in tmp.iterdir():
        p.unlink()
    tmp.rmdir()
    print(json.dumps(out))
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + '\n')


if __name__ == '__main__':
    main()
