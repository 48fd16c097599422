"""GPU: the boundary layer of the library - the entry points that stage their arguments into scratch slots, launch, download and
synchronise through one helper (the host ABI).  Every one of them is called through ctx.lib with host arrays and with device
tensors: the two routes must agree bit for bit, across a slot that grows (1 element, then 8193 - the first size beyond a slot's 64 KiB
minimum - then 3, read out of a slot that still holds the larger call's bytes); optional arguments may be absent; and the text and
code of every argument error are pinned."""
import ctypes as C
import zlib

import numpy as np
import pytest

from raider_amd import _lib as L
from raider_amd import deflate
from raider_amd.engine import Cube
from tests import tiff_codec as T

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

SENTINEL = 0xA5
SIZES = (1, 8193, 3)
LCC = np.array([6371229.0, 0.0, 38.5, 38.5, 38.5, -97.5, 0.0, 0.0])
TM = np.array([6378137.0, 0.00669438, 0.0, -117.0, 0.9996, 500000.0, 0.0])


def sent(nbytes):
    """An output buffer before the call: `nbytes` sentinel bytes."""
    return np.full(int(nbytes), SENTINEL, dtype=np.uint8)


class Case:
    """One call of one entry point: `ins` and `outs` follow `loc` (NumPy arrays; outs hold what the buffer holds before the call),
    `tab` holds the arrays that are host arrays whatever `loc` says, `s` the scalars.  call(lib, handle, p, s, loc) makes the call;
    p(name) is the pointer of a buffer, NULL for the names in `null`."""

    def __init__(self, call, ins, outs, tab=None, **scalars):
        self.call, self.ins, self.outs, self.tab, self.s, self.null = call, ins, outs, tab or {}, scalars, set()

    def run(self, ctx, tensor):
        """(rc, {name: bytes of the output after the call}) over the host route or the device route."""
        if tensor:
            bufs = {k: torch.from_numpy(np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy()).to('cuda:0') for k, v in {**self.ins, **self.outs}.items()}
            ctx.adopt_torch_stream(next(iter(bufs.values())))
        else:
            bufs = {k: np.ascontiguousarray(v).copy() for k, v in {**self.ins, **self.outs}.items()}
        self.bufs = bufs

        def p(name):
            if name in self.null:
                return None
            return L.ptr(bufs[name]) if name in bufs else L.ptr(self.tab[name])
        rc = self.call(ctx.lib, ctx.handle, p, self.s, L.RDR_DEVICE if tensor else L.RDR_HOST)
        if tensor:
            torch.cuda.synchronize()
            return rc, {k: bufs[k].cpu().numpy() for k in self.outs}
        return rc, {k: bufs[k].reshape(-1).view(np.uint8) for k in self.outs}


def _ground(n, rng):
    """(lat, lon, h, xyz, los): n points near 33 N 117 W, their rough ECEF positions and unit look vectors some 35 degrees off the vertical."""
    lat, lon, h = rng.uniform(31, 35, n), rng.uniform(-119, -115, n), rng.uniform(0, 2000, n)
    la, lo = np.radians(lat), np.radians(lon)
    up = np.stack([np.cos(la) * np.cos(lo), np.cos(la) * np.sin(lo), np.sin(la)], axis=1)
    east = np.stack([-np.sin(lo), np.cos(lo), 0 * lo], axis=1)
    los = np.cos(np.radians(35)) * up + np.sin(np.radians(35)) * east
    return lat, lon, h, np.ascontiguousarray(up * (6371e3 + h[:, None])), np.ascontiguousarray(los)


# ---- the entry points: name -> builder(n, rng, ctx) of a Case ---------------------------------------------------------------------
def b_transform_cone(n, rng, ctx):
    call = lambda lib, h, p, s, loc: lib.rdr_transform_cone(h, L.RDR_PROJ_LCC, p('par'), 8, 0, p('a'), p('b'), s['n'], p('oa'), p('ob'), loc)
    return Case(call, dict(a=rng.uniform(-120, -70, n), b=rng.uniform(25, 50, n)), dict(oa=sent(8 * n), ob=sent(8 * n)), dict(par=LCC), n=n)


_cubes = {}


def _lcc_cube(ctx):
    """A small cube on a Lambert grid, made once per context (rdr_project_points takes the projection from it)."""
    if ctx.serial not in _cubes:
        _cubes.clear()
        rng = np.random.default_rng(1)
        q = Cube(np.arange(4.0) * 3e3, np.arange(5.0) * 3e3, np.arange(6.0) * 1e3, rng.random((4, 5, 6)), rng.random((4, 5, 6)), ctx=ctx)
        q.set_projection_lcc(38.5, 38.5, 38.5, -97.5)
        _cubes[ctx.serial] = q
    return _cubes[ctx.serial]


def b_project_points(n, rng, ctx):
    q = _lcc_cube(ctx)
    call = lambda lib, h, p, s, loc: lib.rdr_project_points(h, q.handle, p('lat'), p('lon'), s['n'], p('y'), p('x'), loc)
    return Case(call, dict(lat=rng.uniform(25, 50, n), lon=rng.uniform(-120, -70, n)), dict(y=sent(8 * n), x=sent(8 * n)), n=n)


def b_transform_tm(n, rng, ctx):
    call = lambda lib, h, p, s, loc: lib.rdr_transform_tm(h, p('par'), 7, 0, p('a'), p('b'), s['n'], p('oa'), p('ob'), loc)
    return Case(call, dict(a=rng.uniform(-119, -115, n), b=rng.uniform(31, 35, n)), dict(oa=sent(8 * n), ob=sent(8 * n)), dict(par=TM), n=n)


def b_grid_geodetic(n, rng, ctx):
    call = lambda lib, h, p, s, loc: lib.rdr_grid_geodetic(h, L.RDR_GRID_TM, p('par'), 7, p('x'), s['nx'], p('y'), 2, p('lat'), p('lon'), loc)
    return Case(call, dict(x=np.sort(rng.uniform(4e5, 6e5, n)), y=np.array([3.5e6, 3.6e6])), dict(lat=sent(16 * n), lon=sent(16 * n)), dict(par=TM), nx=n)


def b_inverse_time_weights(n, rng, ctx):
    call = lambda lib, h, p, s, loc: lib.rdr_inverse_time_weights(h, p('az'), s['n'], p('dates'), 3, -1.0, 1e-6, p('w'), loc)
    return Case(call, dict(az=rng.uniform(0, 7200, n)), dict(w=sent(24 * n)), dict(dates=np.array([0.0, 3600.0, 7200.0])), n=n)


def b_delays_to_phase(n, rng, ctx):
    call = lambda lib, h, p, s, loc: lib.rdr_delays_to_phase(h, p('wet'), p('hyd'), s['n'], L.RDR_F64, 0.056, p('ow'), p('oh'), loc)
    return Case(call, dict(wet=rng.random(n), hyd=rng.random(n) + 2), dict(ow=sent(8 * n), oh=sent(8 * n)), n=n)


def _b_project(entry):
    def build(n, rng, ctx):
        call = lambda lib, h, p, s, loc: getattr(lib, entry)(h, p('wet'), p('hyd'), p('proj'), s['n'], loc)
        return Case(call, dict(proj=rng.uniform(20, 45, n)), dict(wet=rng.random(n), hyd=rng.random(n) + 2), n=n)     # (divided in place)
    return build


def b_top_of_atmosphere(n, rng, ctx):
    _, _, _, xyz, los = _ground(n, rng)
    call = lambda lib, h, p, s, loc: lib.rdr_top_of_atmosphere(h, p('xyz'), p('los'), s['n'], 30000.0, p('factor'), p('pos'), loc)
    return Case(call, dict(xyz=xyz, los=los, factor=rng.uniform(0.7, 1.0, n)), dict(pos=sent(24 * n)), n=n)


def b_build_ray(n, rng, ctx):
    _, _, _, xyz, los = _ground(n, rng)
    zs = np.linspace(0.0, 40000.0, 12)
    K = C.c_int32()
    assert ctx.lib.rdr_build_ray(ctx.handle, L.ptr(zs), zs.size, 0.0, L.ptr(xyz), L.ptr(los), n, 30000.0, C.byref(K), None, None, None, L.RDR_HOST) == 0
    k = K.value
    assert k >= 8
    call = lambda lib, h, p, s, loc: lib.rdr_build_ray(h, p('zs'), zs.size, 0.0, p('xyz'), p('los'), s['n'], 30000.0, C.byref(K), p('len'), p('lo'), p('hi'), loc)
    return Case(call, dict(xyz=xyz, los=los), dict(len=sent(8 * k * n), lo=sent(24 * k * n), hi=sent(24 * k * n)), dict(zs=zs), n=n)


def b_lla2ecef(n, rng, ctx):
    lat, lon, h, _, _ = _ground(n, rng)
    call = lambda lib, hd, p, s, loc: lib.rdr_lla2ecef(hd, p('lat'), p('lon'), p('h'), s['n'], p('xyz'), loc)
    return Case(call, dict(lat=lat, lon=lon, h=h), dict(xyz=sent(24 * n)), n=n)


def b_ecef2lla(n, rng, ctx):
    xyz = _ground(n, rng)[3]
    call = lambda lib, h, p, s, loc: lib.rdr_ecef2lla(h, p('xyz'), s['n'], p('lon'), p('lat'), p('h'), loc)
    return Case(call, dict(xyz=xyz), dict(lon=sent(8 * n), lat=sent(8 * n), h=sent(8 * n)), n=n)


def b_look_vectors(n, rng, ctx):
    lat, lon, _, _, _ = _ground(n, rng)

    def call(lib, h, p, s, loc):
        addr = lambda k: getattr(p(k), 'value', None)
        r = L.RdrRays(n=s['n'], origin_mode=L.ORIGIN_LLH, los_mode=L.LOS_INC_HD, lat=addr('lat'), lon=addr('lon'), inc=addr('inc'), hd=addr('hd'), loc=loc)
        return lib.rdr_look_vectors(h, C.byref(r), 0.0, p('los'))
    return Case(call, dict(lat=lat, lon=lon, inc=rng.uniform(20, 45, n), hd=rng.uniform(-170, -160, n)), dict(los=sent(24 * n)), n=n)


def b_ecmwf_model_levels(n, rng, ctx):
    nlev, ny, nx = 3, 2, n
    ins = dict(z=rng.uniform(0, 5000, (ny, nx)).astype(np.float32), lnsp=rng.uniform(11.2, 11.6, (ny, nx)).astype(np.float32),
               t=rng.uniform(220, 290, (nlev, ny, nx)).astype(np.float32), q=rng.uniform(1e-4, 1e-2, (nlev, ny, nx)).astype(np.float32))
    tab = dict(lats=np.array([33.0, 34.0], dtype=np.float32), a=np.array([0.0, 2000.0, 8000.0, 0.0]), b=np.array([0.0, 0.1, 0.6, 1.0]))
    call = lambda lib, h, p, s, loc: lib.rdr_ecmwf_model_levels(h, p('z'), p('lnsp'), p('t'), p('q'), p('lats'), p('a'), p('b'), s['nlev'], ny, nx, 287.06,
                                                                p('p'), p('zs'), loc)
    return Case(call, ins, dict(p=sent(8 * nlev * ny * nx), zs=sent(8 * nlev * ny * nx)), tab, nlev=nlev)


def b_pressure_level_state(n, rng, ctx, out_loc=None):
    nlev, ny, nx = 3, 2, n
    ins = dict(height=np.sort(rng.uniform(0, 30000, (nlev, ny, nx)), axis=0), p=np.array([100000.0, 50000.0, 10000.0]), t=rng.uniform(220, 290, (nlev, ny, nx)),
               hum=rng.uniform(0, 100, (nlev, ny, nx)), lats=np.array([33.0, 34.0]))
    nb = 8 * nlev * ny * nx

    def call(lib, h, p, s, loc):
        return lib.rdr_pressure_level_state(h, p('height'), 1, p('p'), 1, p('t'), p('hum'), p('lats'), 1, s['nlev'], ny, nx, 0, 1, 0, p('ozs'), p('op'), p('ot'),
                                            p('oh'), loc, loc if s['out_loc'] is None else s['out_loc'])
    return Case(call, ins, dict(ozs=sent(nb), op=sent(nb), ot=sent(nb), oh=sent(nb)), nlev=nlev, out_loc=out_loc)


def b_orbit_look_vectors(n, rng, ctx):
    t = np.arange(6.0) * 10.0
    r, w = 7071e3, 7.5e3 / 7071e3                                    # a circular orbit over 33 N 117 W, heading north
    lo = np.radians(-117.0)
    e1 = np.array([np.cos(lo), np.sin(lo), 0.0]); e2 = np.array([0.0, 0.0, 1.0])
    ang = np.radians(33.0) + w * (t - 25.0)
    pos = r * (np.cos(ang)[:, None] * e1 + np.sin(ang)[:, None] * e2)
    vel = r * w * (-np.sin(ang)[:, None] * e1 + np.cos(ang)[:, None] * e2)
    la, ln = np.radians(rng.uniform(32.5, 33.5, n)), np.radians(rng.uniform(-121, -119, n))
    xyz = 6371e3 * np.stack([np.cos(la) * np.cos(ln), np.cos(la) * np.sin(ln), np.sin(la)], axis=1)
    call = lambda lib, h, p, s, loc: lib.rdr_orbit_look_vectors(h, p('t'), p('pos'), p('vel'), 6, p('xyz'), s['n'], 1e-8, 51, p('los'), p('az'), p('sr'), loc)
    return Case(call, dict(xyz=np.ascontiguousarray(xyz)), dict(los=sent(24 * n), az=sent(8 * n), sr=sent(8 * n)),
                dict(t=t, pos=np.ascontiguousarray(pos), vel=np.ascontiguousarray(vel)), n=n)


def b_interp_nd(n, rng, ctx):
    ax0, ax1 = np.linspace(0.0, 4.0, 5), np.linspace(-3.0, 3.0, 7)
    lens = np.array([5, 7], dtype=np.int64)

    def call(lib, h, p, s, loc):
        axes = (C.c_void_p * 2)(getattr(p('ax0'), 'value', None), getattr(p('ax1'), 'value', None))   # (the axes follow `loc`)
        return lib.rdr_interp_nd(h, 2, axes, lens.ctypes.data_as(L.c_lp), p('v'), p('q'), s['n'], 1, -9.0, p('out'), loc)
    q = np.stack([rng.uniform(-0.5, 4.5, n), rng.uniform(-3.5, 3.5, n)], axis=1)
    return Case(call, dict(ax0=ax0, ax1=ax1, v=rng.random((5, 7)), q=np.ascontiguousarray(q)), dict(out=sent(8 * n)), n=n)


def b_interp_along_axis(n, rng, ctx):
    pts = np.cumsum(rng.uniform(0.5, 1.5, (n, 4)), axis=1)
    call = lambda lib, h, p, s, loc: lib.rdr_interp_along_axis(h, p('pts'), p('v'), s['ncol'], 4, p('q'), 2, 1, -9.0, p('out'), loc)
    return Case(call, dict(pts=pts, v=rng.random((n, 4)), q=rng.uniform(0.0, 6.0, (n, 2))), dict(out=sent(16 * n)), ncol=n)


def b_make_points(n, rng, ctx):
    _, _, _, xyz, los = _ground(n, rng)
    npts = int(L.load().rdr_make_points_count(10.0, 3.0))
    assert npts == 4
    call = lambda lib, h, p, s, loc: lib.rdr_make_points(h, 10.0, p('sp'), p('slv'), s['n'], 3.0, p('out'), loc)
    return Case(call, dict(sp=xyz, slv=los), dict(out=sent(8 * 3 * npts * n)), n=n)


def b_raster_sample(n, rng, ctx):
    gt = np.array([0.0, 1.0, 0.0, 5.0, 0.0, -1.0])
    call = lambda lib, h, p, s, loc: lib.rdr_raster_sample(h, p('r'), L.RDR_F32, 5, 7, p('gt'), p('x'), p('y'), s['n'], L.RASTER_LINEAR, 0, 0.0, p('out'), loc)
    return Case(call, dict(r=rng.random((5, 7), dtype=np.float32), x=rng.uniform(-0.5, 7.5, n), y=rng.uniform(-0.5, 5.5, n)), dict(out=sent(8 * n)), dict(gt=gt), n=n)


def b_raster_bounds(n, rng, ctx):
    call = lambda lib, h, p, s, loc: lib.rdr_raster_bounds(h, p('a'), p('b'), L.RDR_F64, s['n'], 1, -1.0, p('out'), loc)
    a, b = rng.random(n), rng.random(n) + 3
    if n > 2:
        a[1] = -1.0                                                  # (a no-data element)
    return Case(call, dict(a=a, b=b), dict(out=sent(48)), n=n)


def _streams(n, rng, codec):
    """(buffer, offsets, sizes, caps, stride, the decoded data): four streams of 8 n random bytes (so the coded buffer grows with n too)
    in one buffer, at odd offsets; the third decodes to a third of that, so it ends well short of its slot."""
    data = [rng.integers(0, 256, 8 * n if k != 2 else 8 * n // 3, dtype=np.uint8).tobytes() for k in range(4)]
    enc = [codec(d) for d in data]
    parts, offs, pos = [b'\xa5'], [], 1
    for e in enc:
        offs.append(pos)
        gap = 1 + (pos + len(e)) % 2
        parts += [e, b'\xa5' * gap]
        pos += len(e) + gap
    caps = np.array([len(d) for d in data], dtype=np.int64)
    return (np.frombuffer(b''.join(parts), dtype=np.uint8), np.array(offs, dtype=np.int64), np.array([len(e) for e in enc], dtype=np.int64), caps,
            (int(caps.max()) + 16 + 15) // 16 * 16, data)


def b_tiff_lzw_decode(n, rng, ctx):
    buf, offs, sizes, caps, stride, data = _streams(n, rng, T.lzw_encode)
    call = lambda lib, h, p, s, loc: lib.rdr_tiff_lzw_decode(h, p('src'), buf.size, p('offs'), p('sizes'), s['nseg'], p('caps'), p('out'), s['stride'], p('status'), loc)
    c = Case(call, dict(src=buf), dict(out=sent(4 * stride), status=sent(16)), dict(offs=offs, sizes=sizes, caps=caps), nseg=4, stride=stride)
    c.data = data
    return c


def b_inflate_decode(n, rng, ctx):
    buf, offs, sizes, caps, stride, data = _streams(n, rng, lambda d: zlib.compress(d, 6))
    call = lambda lib, h, p, s, loc: lib.rdr_inflate_decode(h, p('src'), buf.size, p('offs'), p('sizes'), s['nseg'], p('caps'), p('out'), s['stride'], p('status'),
                                                            p('produced'), loc)
    c = Case(call, dict(src=buf), dict(out=sent(4 * stride), status=sent(16), produced=sent(32)), dict(offs=offs, sizes=sizes, caps=caps), nseg=4, stride=stride)
    c.data = data
    return c


def _raster_shape(n):
    """5 x 7 (an edge tile on both axes with 4 x 4 tiles) for the small calls, 131 x 129 in 16 x 16 tiles for the one that grows the slots."""
    return (5, 7, 4) if n < 100 else (131, 129, 16)


def b_tiff_assemble(n, rng, ctx):
    hgt, wid, tile = _raster_shape(n)
    nseg = -(-hgt // tile) * -(-wid // tile)
    stride = tile * tile * 4
    call = lambda lib, h, p, s, loc: lib.rdr_tiff_assemble(h, p('segs'), stride, s['height'], wid, tile, tile, 2, 0, 4, 1, 1, -1, p('out'), loc)
    return Case(call, dict(segs=rng.integers(0, 256, nseg * stride, dtype=np.uint8)), dict(out=sent(hgt * wid * 4)), height=hgt)


def b_tiff_predict(n, rng, ctx):
    hgt, wid, _ = _raster_shape(n)
    call = lambda lib, h, p, s, loc: lib.rdr_tiff_predict(h, p('in'), 4, s['height'], wid, p('out'), loc)
    return Case(call, {'in': rng.integers(0, 1 << 32, (hgt, wid), dtype=np.uint32)}, dict(out=sent(hgt * wid * 4)), height=hgt)


def _array_shape(n):
    """3 x 5 x 7 in 2 x 4 x 4 chunks (an edge chunk on every axis) for the small calls, 9 x 33 x 37 in 4 x 16 x 16 chunks for the large one."""
    return ((3, 5, 7), (2, 4, 4)) if n < 100 else ((9, 33, 37), (4, 16, 16))


def b_h5_chunks(n, rng, ctx):
    shape, chunk = _array_shape(n)
    nb = int(np.prod(deflate.chunk_grid(shape, chunk)) * np.prod(chunk)) * 8
    tab = dict(shape=np.array(shape, dtype=np.int64), chunk=np.array(chunk, dtype=np.int64), fill=np.array([np.nan]))
    call = lambda lib, h, p, s, loc: lib.rdr_h5_chunks(h, p('a'), 8, s['ndim'], p('shape'), p('chunk'), p('fill'), 1, p('out'), loc)
    return Case(call, dict(a=rng.random(shape)), dict(out=sent(nb)), tab, ndim=3)


def b_h5_unchunk(n, rng, ctx):
    shape, chunk = _array_shape(n)
    raw = deflate.h5_chunks_host(rng.random(shape), chunk, np.nan, True)
    nchunks = int(np.prod(deflate.chunk_grid(shape, chunk)))
    stride = raw.size // nchunks
    index = rng.permutation(nchunks)[:nchunks - 1].astype(np.int64)       # one chunk absent: its elements read as 0
    chunks = np.concatenate([raw[k * stride:(k + 1) * stride] for k in index])
    tab = dict(index=index, shape=np.array(shape, dtype=np.int64), chunk=np.array(chunk, dtype=np.int64))
    call = lambda lib, h, p, s, loc: lib.rdr_h5_unchunk(h, p('chunks'), stride, p('index'), s['npresent'], s['es'], 3, p('shape'), p('chunk'), 1, 0, p('out'), loc)
    return Case(call, dict(chunks=chunks), dict(out=sent(int(np.prod(shape)) * 8)), tab, npresent=index.size, es=8)


def b_deflate_encode_tables(n, rng, ctx):
    src = np.frombuffer((b'slant delay ' * (n + 1))[:8 * n], dtype=np.uint8)
    cut = max(1, 3 * n)
    tab = dict(offs=np.array([0, cut], dtype=np.int64), sizes=np.array([cut, 8 * n - cut], dtype=np.int64), oo=np.zeros(3, dtype=np.int64),
               kinds=np.zeros(3, dtype=np.int64))
    cap = int(sum(deflate.bound(int(v)) for v in tab['sizes']))
    call = lambda lib, h, p, s, loc: lib.rdr_deflate_encode_tables(h, p('src'), src.size, p('offs'), p('sizes'), s['nseg'], L.RDR_DEFL_DYNAMIC, p('out'), cap, p('oo'),
                                                                   p('kinds'), loc)
    return Case(call, dict(src=src), dict(out=sent(cap)), tab, nseg=2)


ENTRIES = {
    'rdr_transform_cone': b_transform_cone, 'rdr_project_points': b_project_points, 'rdr_transform_tm': b_transform_tm,
    'rdr_grid_geodetic': b_grid_geodetic, 'rdr_inverse_time_weights': b_inverse_time_weights, 'rdr_delays_to_phase': b_delays_to_phase,
    'rdr_project_cosinc': _b_project('rdr_project_cosinc'), 'rdr_project_divide': _b_project('rdr_project_divide'),
    'rdr_top_of_atmosphere': b_top_of_atmosphere, 'rdr_build_ray': b_build_ray, 'rdr_lla2ecef': b_lla2ecef, 'rdr_ecef2lla': b_ecef2lla,
    'rdr_look_vectors': b_look_vectors, 'rdr_ecmwf_model_levels': b_ecmwf_model_levels, 'rdr_pressure_level_state': b_pressure_level_state,
    'rdr_orbit_look_vectors': b_orbit_look_vectors, 'rdr_interp_nd': b_interp_nd, 'rdr_interp_along_axis': b_interp_along_axis,
    'rdr_make_points': b_make_points, 'rdr_raster_sample': b_raster_sample, 'rdr_raster_bounds': b_raster_bounds,
    'rdr_tiff_lzw_decode': b_tiff_lzw_decode, 'rdr_tiff_assemble': b_tiff_assemble, 'rdr_tiff_predict': b_tiff_predict,
    'rdr_h5_chunks': b_h5_chunks, 'rdr_h5_unchunk': b_h5_unchunk, 'rdr_deflate_encode_tables': b_deflate_encode_tables,
    'rdr_inflate_decode': b_inflate_decode,
}


def _both(ctx, case):
    """{name: bytes} of the host route, after checking that the device route gave the same bytes."""
    rc, host = case.run(ctx, False)
    assert rc == 0, L.last_error(ctx.handle)
    tabs = {k: v.tobytes() for k, v in case.tab.items()}
    rc, dev = case.run(ctx, True)
    assert rc == 0, L.last_error(ctx.handle)
    for k in case.outs:
        assert np.array_equal(host[k], dev[k]), k
    for k, v in case.tab.items():                                   # (tables the library writes - stream offsets, block counts - agree too)
        assert tabs[k] == v.tobytes(), k
    return host


# ---- host and device routes agree, across slot growth -----------------------------------------------------------------------------
@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_routes_agree_across_slot_growth(entry):
    ctx = L.Context()                                               # one context for the six calls: every slot starts empty and grows once
    rng = np.random.default_rng(sorted(ENTRIES).index(entry))
    for n in SIZES:
        case = ENTRIES[entry](n, rng, ctx)
        host = _both(ctx, case)
        assert any(np.any(v != SENTINEL) for v in host.values()), n          # the call wrote something
        if entry in ('rdr_tiff_lzw_decode', 'rdr_inflate_decode'):
            slots = host['out'].reshape(4, case.s['stride'])
            assert np.all(host['status'].view(np.int32) == 0)
            for k, d in enumerate(case.data):
                assert slots[k, :len(d)].tobytes() == d, (n, k)
                assert np.all(slots[k, len(d):] == SENTINEL), (n, k)         # bytes the stream does not reach keep their value
            assert len(case.data[2]) + 5 <= len(case.data[0])
            if entry == 'rdr_inflate_decode':
                assert list(host['produced'].view(np.int64)) == [len(d) for d in case.data]
        if entry == 'rdr_deflate_encode_tables':
            oo = case.tab['oo']
            for k in range(2):
                o, m = int(case.tab['offs'][k]), int(case.tab['sizes'][k])
                assert zlib.decompress(host['out'][oo[k]:oo[k + 1]].tobytes()) == case.ins['src'][o:o + m].tobytes()
            assert np.all(host['out'][oo[2]:] == SENTINEL)


# ---- optional arguments -----------------------------------------------------------------------------------------------------------
def _optional(entry, absent, same, n=37, **kw):
    """The call without the buffers in `absent`, on both routes: the outputs in `same` equal the all-arguments call's, a host buffer that
    was not asked for keeps its sentinel.  Returns (outputs of the full call, outputs without)."""
    ctx = L.Context()
    full = ENTRIES[entry](n, np.random.default_rng(5), ctx, **kw)
    want = _both(ctx, full)
    part = ENTRIES[entry](n, np.random.default_rng(5), ctx, **kw)
    part.null = set(absent)
    got = _both(ctx, part)
    for k in same:
        assert np.array_equal(got[k], want[k]), k
    for k in set(absent) & set(part.outs):
        assert np.array_equal(got[k], np.ascontiguousarray(part.outs[k]).reshape(-1).view(np.uint8)), k
    return want, got


def test_top_of_atmosphere_without_factor():
    want, got = _optional('rdr_top_of_atmosphere', ['factor'], [])
    assert np.all(np.isfinite(got['pos'].view(np.float64)))


@pytest.mark.parametrize('absent', [['az'], ['sr'], ['az', 'sr']])
def test_orbit_look_vectors_optional_outputs(absent):
    _optional('rdr_orbit_look_vectors', absent, {'los', 'az', 'sr'} - set(absent))


def test_raster_bounds_without_b():
    want, got = _optional('rdr_raster_bounds', ['b'], [])
    a, b = want['out'].view(np.float64), got['out'].view(np.float64)
    assert np.array_equal(a[:3], b[:3]) and a[2] == 36 and a[5] == 37
    assert np.isnan(b[3]) and np.isnan(b[4]) and b[5] == 0          # no second raster: no valid element


@pytest.mark.parametrize('absent', ['hyd', 'wet'])
def test_project_cosinc_one_delay(absent):
    _optional('rdr_project_cosinc', [absent], {'wet', 'hyd'} - {absent})


def test_inflate_decode_without_produced():
    _optional('rdr_inflate_decode', ['produced'], ['out', 'status'], n=300)


@pytest.mark.parametrize('loc,out_loc', [(L.RDR_HOST, L.RDR_DEVICE), (L.RDR_DEVICE, L.RDR_HOST)])
def test_pressure_level_state_mixed_locations(loc, out_loc):
    ctx = L.Context()
    want = _both(ctx, b_pressure_level_state(37, np.random.default_rng(6), ctx))
    case = b_pressure_level_state(37, np.random.default_rng(6), ctx, out_loc=out_loc)
    ins = {k: np.ascontiguousarray(v) for k, v in case.ins.items()}
    outs = {k: v.copy() for k, v in case.outs.items()}
    if loc == L.RDR_DEVICE:
        ins = {k: torch.from_numpy(v).to('cuda:0') for k, v in ins.items()}
    else:
        outs = {k: torch.from_numpy(v).to('cuda:0') for k, v in outs.items()}
    ctx.adopt_torch_stream(next(iter((ins if loc == L.RDR_DEVICE else outs).values())))
    p = lambda k: L.ptr(ins[k] if k in ins else outs[k])
    assert case.call(ctx.lib, ctx.handle, p, case.s, loc) == 0, L.last_error(ctx.handle)
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert np.array_equal(v.cpu().numpy() if out_loc == L.RDR_DEVICE else v, want[k]), k


# ---- error texts and codes ----------------------------------------------------------------------------------------------------------
def _bad_offset(c):
    c.tab['offs'] = c.tab['offs'].copy(); c.tab['offs'][1] = 1 << 40


def _bad_cap(c):
    c.tab['caps'] = c.tab['caps'].copy(); c.tab['caps'][2] = c.s['stride'] + 1


def _bad_shape(c):
    c.tab['shape'] = c.tab['shape'].copy(); c.tab['shape'][1] = 0


# (entry, what to change in a valid call of 3 elements, the error text): every one is RDR_ERR_INVALID
ERRORS = [(e, dict(null=a), f'{e}: NULL argument') for e, a in [
    ('rdr_transform_cone', 'a'), ('rdr_project_points', 'lat'), ('rdr_grid_geodetic', 'lat'), ('rdr_inverse_time_weights', 'w'),
    ('rdr_delays_to_phase', 'hyd'), ('rdr_project_cosinc', 'proj'), ('rdr_project_divide', 'proj'), ('rdr_top_of_atmosphere', 'pos'),
    ('rdr_build_ray', 'xyz'), ('rdr_lla2ecef', 'h'), ('rdr_ecef2lla', 'lat'), ('rdr_look_vectors', 'los'), ('rdr_ecmwf_model_levels', 'b'),
    ('rdr_pressure_level_state', 'oh'), ('rdr_orbit_look_vectors', 'vel'), ('rdr_interp_nd', 'v'), ('rdr_interp_along_axis', 'q'),
    ('rdr_make_points', 'slv'), ('rdr_raster_sample', 'gt'), ('rdr_raster_bounds', 'out'), ('rdr_tiff_lzw_decode', 'caps'),
    ('rdr_tiff_assemble', 'segs'), ('rdr_tiff_predict', 'out'), ('rdr_h5_chunks', 'fill'), ('rdr_h5_unchunk', 'index'), ('rdr_inflate_decode', 'status')]]
ERRORS += [(e, dict(n=-1), f'{e}: negative count') for e in [
    'rdr_transform_cone', 'rdr_project_points', 'rdr_transform_tm', 'rdr_inverse_time_weights', 'rdr_delays_to_phase', 'rdr_project_cosinc',
    'rdr_project_divide', 'rdr_top_of_atmosphere', 'rdr_build_ray', 'rdr_lla2ecef', 'rdr_ecef2lla', 'rdr_orbit_look_vectors', 'rdr_interp_nd',
    'rdr_make_points']]
ERRORS += [
    ('rdr_transform_tm', dict(null='ob'), 'rdr_transform_tm: NULL argument / 7 parameters (a, es, lat_0, lon_0, k_0, x_0, y_0)'),
    ('rdr_deflate_encode_tables', dict(null='oo'), 'rdr_deflate_encode: NULL argument'),
    ('rdr_grid_geodetic', dict(nx=-1), 'rdr_grid_geodetic: negative count'),
    ('rdr_interp_along_axis', dict(ncol=-1), 'rdr_interp_along_axis: negative count'),
    ('rdr_look_vectors', dict(n=-1), 'rays->n negative'),
    ('rdr_ecmwf_model_levels', dict(nlev=0), 'rdr_ecmwf_model_levels: empty grid'),
    ('rdr_pressure_level_state', dict(nlev=0), 'rdr_pressure_level_state: empty grid'),
    ('rdr_raster_sample', dict(n=0), 'rdr_raster_sample: the point count must be positive'),
    ('rdr_raster_bounds', dict(n=0), 'rdr_raster_bounds: the element count must be positive (at most 2^40)'),
    ('rdr_tiff_assemble', dict(height=0), 'rdr_tiff_assemble: raster and segment sizes must be positive (below 2^31)'),
    ('rdr_tiff_predict', dict(height=0), 'rdr_tiff_predict: raster sizes must be positive, at most 2^36 samples'),
    ('rdr_tiff_lzw_decode', dict(nseg=0), 'rdr_tiff_lzw_decode: need a non-empty buffer and 1 .. 2^24 segments'),
    ('rdr_inflate_decode', dict(nseg=0), 'rdr_inflate_decode: need a non-empty buffer and 1 .. 2^24 segments'),
    ('rdr_deflate_encode_tables', dict(nseg=0), 'rdr_deflate_encode: need a non-empty buffer (at most 2^40 bytes) and 1 .. 2^24 segments'),
    ('rdr_h5_chunks', dict(ndim=0), 'rdr_h5_chunks: 1 .. 4 dimensions'),
    ('rdr_h5_unchunk', dict(npresent=0), 'rdr_h5_unchunk: 1 .. 8 chunks may be present'),
    # a table or shape error each, for the entries that share their validation
    ('rdr_tiff_lzw_decode', dict(change=_bad_offset), 'rdr_tiff_lzw_decode: segment 1 does not lie inside the source buffer'),
    ('rdr_tiff_lzw_decode', dict(stride=0), 'rdr_tiff_lzw_decode: out_stride must be positive and below 2 GiB (at most 2^40 bytes in all)'),
    ('rdr_inflate_decode', dict(change=_bad_offset), 'rdr_inflate_decode: segment 1 does not lie inside the source buffer'),
    ('rdr_inflate_decode', dict(change=_bad_cap), 'rdr_inflate_decode: segment 2 would write beyond its slot of out_stride bytes'),
    ('rdr_deflate_encode_tables', dict(change=_bad_offset), 'rdr_deflate_encode: segment 1 does not lie inside the source buffer'),
    ('rdr_h5_chunks', dict(change=_bad_shape), 'rdr_h5_chunks: shape and chunk sizes must be positive (below 2^31)'),
    ('rdr_h5_unchunk', dict(change=_bad_shape), 'rdr_h5_unchunk: shape and chunk sizes must be positive (below 2^31)'),
    ('rdr_h5_unchunk', dict(es=3), 'rdr_h5_unchunk: elements of 1, 2, 4 or 8 bytes'),
]


@pytest.fixture(scope='module')
def error_ctx():
    return L.Context()


@pytest.mark.parametrize('entry,change,text', ERRORS, ids=[f'{e}-{"-".join(sorted(c))}-{i}' for i, (e, c, _) in enumerate(ERRORS)])
def test_error_texts_and_codes(error_ctx, entry, change, text):
    case = ENTRIES[entry](3, np.random.default_rng(7), error_ctx)
    for k, v in change.items():
        if k == 'null':
            case.null = {v}
        elif k == 'change':
            v(case)
        else:
            assert k in case.s, k
            case.s[k] = v
    rc, out = case.run(error_ctx, False)
    assert rc == L.RDR_ERR_INVALID
    assert L.last_error(error_ctx.handle) == text
    for k, v in out.items():                                        # refused before anything was written
        assert np.array_equal(v, np.ascontiguousarray(case.outs[k]).reshape(-1).view(np.uint8)), k
