"""GPU: the host drivers of the ray and point entries (raider_hip.hip: RayCall, partition_reset / partition_read, prepass_records,
march_on_records, grow, gather_staged).  Nothing here is new behaviour: the routes through the drivers are compared with each other, bit
for bit, so the file needs no tolerance of its own - the one comparison with the C oracle takes bound and helper from test_gpu_tile_body.

  a. three routes, one answer: raytrace | ray_prepass -> nparts -> ray_march | ray_prepass_device -> ray_march_device, for host and for
     device arrays, with the stored records reused (the same device pointers), with the reuse defeated (a fresh copy of one array) and
     with a workspace too small for the batch (the chunked store-only pass 1); f32 and f64 cubes, one slice height and per-ray heights;
  b. scratch that grows and is reused: small, 78 x larger, small again on one context; 1, 7, 1 slices;
  c. early exits of the five ray entries, called as C: no contributing level, an empty batch;
  d. rdr_ray_kernel_attributes for which = 0..7;
  e. a date series at 300 points against one call per date, and what it says it copied up.

Scene: a 12 x 14 x 9 lon/lat cube, a 70 x 50 ray grid (5 x 4 tiles, padded both ways) in the middle of it, incidence 20 .. 40 degrees."""
import ctypes as C

import numpy as np
import pytest

from oracle import raider_oracle as O
from oracle import oracle_c as OC
from tests.test_gpu_tile_body import _against

pytestmark = pytest.mark.gpu

NY, NX = 50, 70
HD = -167.9
HT = 0.0
NO_LEVELS = 'no weather-model interval contributes to the ray integral (build_ray -> None)'

_S = {}


def _scene():
    if not _S:
        c = O.synthetic_cube(12, 14, 9, seed=27)
        xs, ys = np.asarray(c['xs']), np.asarray(c['ys'])
        fx = lambda f: xs.min() + f * (xs.max() - xs.min())
        fy = lambda f: ys.min() + f * (ys.max() - ys.min())
        xp, yp = np.linspace(fx(0.3), fx(0.7), NX), np.linspace(fy(0.7), fy(0.3), NY)
        xx, yy = np.meshgrid(xp, yp)
        inc = np.broadcast_to(20.0 + 20.0 * np.arange(NX) / (NX - 1), (NY, NX)).copy()
        los = np.ascontiguousarray(O.look_vectors_from_inc_hd(inc, np.full((NY, NX), HD), yy, xx, 0.0))
        hts = np.ascontiguousarray(400.0 + 350.0 * np.sin(xx * 3.0) * np.cos(yy * 2.0))          # per-ray origin heights, 50 .. 750 m
        _S.update(c=c, xp=xp, yp=yp, los=los, hts=hts, zref=float(np.asarray(c['zs'])[-1] - 1.0), cubes={}, ref={})
    return _S


def _cube(dtype, ctx=None):
    import raider_amd as R
    s = _scene()
    if ctx is not None or dtype not in s['cubes']:
        c = s['c']
        q = R.Cube(c['ys'], c['xs'], c['zs'], np.asarray(c['wet'], dtype=dtype), np.asarray(c['hydro'], dtype=dtype), order='zyx', ctx=ctx)
        if ctx is not None:
            return q
        s['cubes'][dtype] = q
    return s['cubes'][dtype]


def _rays(per_ray, device=False, rows=slice(None), cols=slice(None), fresh_los=False):
    """the batch (rows / cols: a block of it) on host arrays, or - whole - on ONE set of device tensors (fresh_los: but a copy of los)"""
    import raider_amd as R
    s = _scene()
    a = dict(xp=s['xp'][cols], yp=s['yp'][rows], los=np.ascontiguousarray(s['los'][rows, cols]), hts=np.ascontiguousarray(s['hts'][rows, cols]))
    if device:
        import torch
        if 'dev' not in s:
            s['dev'] = {k: torch.from_numpy(v).cuda() for k, v in a.items()}
        a = dict(s['dev'])
        if fresh_los:
            a['los'] = a['los'].clone()
    return R.Rays.grid(a['xp'], a['yp'], los=a['los'], hts=a['hts'] if per_ray else None)


def _host(a):
    return a.cpu().numpy() if hasattr(a, 'cpu') else np.asarray(a)


def _same(a, b):
    return np.array_equal(_host(a), _host(b), equal_nan=True)


def _reference(dtype, per_ray):
    """rdr_raytrace on host arrays, once per cube dtype and height form: (wet, hydro, nparts, flags)"""
    s = _scene()
    if (dtype, per_ray) not in s['ref']:
        w, h, npn, fl = _cube(dtype).raytrace(_rays(per_ray), None if per_ray else HT, s['zref'])
        assert np.isfinite(w).all() and np.isfinite(h).all() and w.min() > 0
        s['ref'][(dtype, per_ray)] = (np.array(w, copy=True), np.array(h, copy=True), npn, fl)
    return s['ref'][(dtype, per_ray)]


def _pass1_launches(ctx, call):
    """(result of call(), launches of the light pass-1 kernel it made)"""
    ctx.set_profiling(True)
    try:
        out = call()
        return out, ctx.profile_get(0)[0]
    finally:
        ctx.set_profiling(False)


def _check(what, got, ref):
    w, h, npn, fl = got
    assert np.array_equal(npn, ref[2]) and (fl & 15) == (ref[3] & 15), (what, npn, ref[2], fl, ref[3])
    assert _same(w, ref[0]) and _same(h, ref[1]), what


def _via_host_partition(cube, rays, march_rays, ht, zref):
    import raider_amd as R
    ml, fl = cube.ray_prepass(rays, ht, zref)
    npn = R.nparts_from_maxlen(ml, 1000.0)
    (w, h), launches = _pass1_launches(cube.ctx, lambda: cube.ray_march(march_rays, ht, zref, npn, fl))
    return (w, h, npn, fl), launches


def _via_device_partition(cube, rays, march_rays, ht, zref):
    import torch
    import raider_amd as R
    K = len(cube.ray_levels(rays.table_height(ht), zref)[0])
    part = torch.full((K + 4,), 7.0, dtype=torch.float64, device='cuda')
    cube.ray_prepass_device(rays, ht, zref, part)
    (w, h), launches = _pass1_launches(cube.ctx, lambda: cube.ray_march_device(march_rays, ht, zref, part))
    p = part.cpu().numpy()
    assert set(p[K:]) <= {0.0, 1.0}
    return (w, h, R.nparts_from_maxlen(p[:K], 1000.0), int(p[K] + 2 * p[K + 1] + 4 * p[K + 2] + 8 * p[K + 3])), launches


@pytest.mark.parametrize('per_ray', [False, True], ids=['slice', 'per_ray_heights'])
@pytest.mark.parametrize('dtype', [np.float32, np.float64], ids=['f32', 'f64'])
def test_three_routes_one_answer(dtype, per_ray):
    import raider_amd as R
    s = _scene()
    cube, zref, ht = _cube(dtype), s['zref'], None if per_ray else HT
    ref = _reference(dtype, per_ray)
    # host arrays: nothing is kept between the two calls (a host array may have been rewritten), the march runs its own store-only pass 1
    got, launches = _via_host_partition(cube, _rays(per_ray), _rays(per_ray), ht, zref)
    _check('host: prepass -> march', got, ref)
    assert launches == 1
    # device arrays
    rays = _rays(per_ray, device=True)
    _check('device: raytrace', cube.raytrace(rays, ht, zref), ref)
    for name, route in (('prepass -> march', _via_host_partition), ('prepass_device -> march_device', _via_device_partition)):
        got, launches = route(cube, rays, rays, ht, zref)
        _check(f'device, records reused: {name}', got, ref)
        assert launches == 0, name
        got, launches = route(cube, rays, _rays(per_ray, device=True, fresh_los=True), ht, zref)
        _check(f'device, another look-vector array: {name}', got, ref)
        assert launches == 1, name
        # 20 tiles of records do not fit 1 MiB (17): pass 1 keeps nothing, the march stores and integrates chunk by chunk
        ctx = R.Context.default()
        ctx.set_workspace_limit(1 << 20)
        try:
            got, launches = route(cube, rays, rays, ht, zref)
        finally:
            ctx.set_workspace_limit(48 << 30)
        _check(f'device, chunked: {name}', got, ref)
        assert launches >= 2, name


def test_one_route_against_the_oracle():
    s = _scene()
    w, h, npn, fl = _reference(np.float32, False)
    _against('ray drivers', w, h, npn, OC.build_cube_ray_slice(s['c'], s['xp'], s['yp'], HT, s['los'], s['zref']))


def test_scratch_grows_and_is_reused():
    """slots, record workspace, side buffer (and, for slices, the level table) of ONE context: small, large, small again"""
    from raider_amd import _lib as L
    s = _scene()
    ctx = L.Context()
    cube = _cube(np.float32, ctx)
    small = lambda: _rays(False, rows=slice(10, 15), cols=slice(20, 29))
    assert 75 < NY * NX / (5 * 9) < 85
    first = cube.raytrace(small(), HT, s['zref'])
    first = tuple(np.array(a, copy=True) for a in first[:3]) + (first[3],)
    _check('large after small', cube.raytrace(_rays(False), HT, s['zref']), _reference(np.float32, False))
    _check('small after large', cube.raytrace(small(), HT, s['zref']), first)
    # 1, 7, 1 slices
    hts7 = np.array([0.0, 120.0, 300.0, 650.0, 1500.0, 5000.0, 9000.0])
    one = cube.raytrace_slices(small(), hts7[:1], s['zref'])
    one = [np.array(a, copy=True) for a in one]
    seven = cube.raytrace_slices(small(), hts7, s['zref'])
    assert len(set(int(k) for k in seven[2])) > 1
    again = cube.raytrace_slices(small(), hts7[:1], s['zref'])
    for a, b, c7 in zip(one, again, seven):
        assert _same(a, b) and _same(a[0], c7[0])
    assert _same(one[0][0], first[0]) and _same(one[1][0], first[1])


def _entries(ctx, cube, rs, nz, dev):
    """the five one-batch ray entries on the rdr_rays `rs` as (name, call, wet, hydro, partition outputs); the outputs hold 7.0"""
    import torch
    lib, h, q, r = ctx.lib, ctx.handle, cube.handle, C.byref(rs)
    new = (lambda n: torch.full((n,), 7.0, dtype=torch.float64, device='cuda')) if dev else (lambda n: np.full(n, 7.0))
    p = lambda a: C.c_void_p(a.data_ptr()) if dev else C.c_void_p(a.ctypes.data)
    ml, fl, part = np.full(nz, 7.0), C.c_int32(7), torch.full((nz + 4,), 7.0, dtype=torch.float64, device='cuda')
    nparts, npo, flo = np.full(nz, 2, dtype=np.int32), np.zeros(nz, dtype=np.int32), C.c_int32(7)
    hp = lambda a: C.c_void_p(a.ctypes.data)
    w, hy = [new(4) for _ in range(5)], [new(4) for _ in range(5)]
    calls = (('rdr_ray_prepass', lambda ht, zref: lib.rdr_ray_prepass(h, q, r, ht, zref, hp(ml), C.byref(fl))),
             ('rdr_ray_prepass_device', lambda ht, zref: lib.rdr_ray_prepass_device(h, q, r, ht, zref, C.c_void_p(part.data_ptr()))),
             ('rdr_ray_march', lambda ht, zref: lib.rdr_ray_march(h, q, r, ht, zref, hp(nparts), 2, p(w[2]), p(hy[2]))),
             ('rdr_ray_march_device', lambda ht, zref: lib.rdr_ray_march_device(h, q, r, ht, zref, 1000.0, C.c_void_p(part.data_ptr()), p(w[3]), p(hy[3]))),
             ('rdr_raytrace', lambda ht, zref: lib.rdr_raytrace(h, q, r, ht, zref, 1000.0, p(w[4]), p(hy[4]), hp(npo), C.byref(flo))))
    torch.cuda.synchronize()
    return [(name, call, w[i], hy[i], dict(maxlen=ml, flags=fl, partition=part)) for i, (name, call) in enumerate(calls)]


def test_early_exits_of_the_five_entries():
    import torch
    import raider_amd as R
    from raider_amd import _lib as L
    s = _scene()
    cube = _cube(np.float64)
    ctx, nz = cube.ctx, cube.shape[2]
    K = len(cube.ray_levels(HT, s['zref'])[0])
    # no model interval between 50 km and the top of the model: the same code and text from all five, nothing launched, nothing written
    rays = _rays(False, device=True)
    rays.adopt_stream(ctx)
    for name, call, w, hy, _ in _entries(ctx, cube, rays.struct, nz, True):
        assert call(50000.0, s['zref']) == L.RDR_ERR_NO_LEVELS, name
        assert L.last_error() == NO_LEVELS, name
        assert (_host(w) == 7.0).all() and (_host(hy) == 7.0).all(), name
    with pytest.raises(R.NoLevels):
        cube.ray_levels(50000.0, s['zref'])
    # an empty batch (LLH origins, zenith rays, n = 0), device and host arrays
    ctx.set_stream(-1)
    for dev in (True, False):
        dummy = torch.zeros(1, dtype=torch.float64, device='cuda') if dev else np.zeros(1)
        rs = L.RdrRays()
        rs.n, rs.origin_mode, rs.los_mode, rs.loc = 0, L.ORIGIN_LLH, L.LOS_ZENITH, L.RDR_DEVICE if dev else L.RDR_HOST
        rs.lat = rs.lon = dummy.data_ptr() if dev else dummy.ctypes.data
        for name, call, w, hy, part in _entries(ctx, cube, rs, nz, dev):
            if not dev and name.endswith('_device'):
                assert call(HT, s['zref']) == L.RDR_ERR_INVALID and 'must be device arrays' in L.last_error(), name
                continue
            assert call(HT, s['zref']) == L.RDR_OK, (name, L.last_error())
            ctx.synchronize()
            assert (_host(w) == 7.0).all() and (_host(hy) == 7.0).all(), name
            if name == 'rdr_ray_prepass':
                assert not part['maxlen'][:K].any() and part['flags'].value == 0
            if name == 'rdr_ray_prepass_device':
                assert not _host(part['partition'])[:K + 4].any()


def test_kernel_attributes_of_both_dtypes():
    for dtype in (np.float32, np.float64):
        cube = _cube(dtype)
        attrs = [cube.ray_kernel_attributes(which) for which in range(8)]
        print('RAYDRIVERS vgpr', np.dtype(dtype).name, [a['vgpr'] for a in attrs])
        for which, a in enumerate(attrs):
            assert a['vgpr'] > 0 and a['max_threads'] > 0, (which, a)
            if which >= 4:                       # (test_stacked_kernels_are_loaded_without_scratch)
                assert a['scratch'] == 0, (which, a)
    with pytest.raises(ValueError):
        cube.ray_kernel_attributes(8)


@pytest.mark.parametrize('device', [False, True], ids=['host', 'device'])
def test_a_date_series_at_points_is_one_call_per_date(device):
    import raider_amd as R
    s = _scene()
    D, n = 3, 300
    cubes = []
    for e in range(D):
        c = O.synthetic_cube(12, 14, 9, seed=60 + e)
        cubes.append(R.Cube(c['ys'], c['xs'], c['zs'], c['wet_total'], c['hydro_total'], order='zyx'))
    ctx = cubes[0].ctx
    c, rng = s['c'], np.random.default_rng(5)
    lo, hi = np.array([c['ys'][0], c['xs'][0], c['zs'][0]]), np.array([c['ys'][-1], c['xs'][-1], c['zs'][-1]])
    y, x, z = (np.ascontiguousarray(rng.uniform(lo[k] - 0.02 * (hi[k] - lo[k]), hi[k] + 0.02 * (hi[k] - lo[k]), n)) for k in range(3))
    inc, div = rng.uniform(20.0, 46.0, (D, n)), rng.uniform(0.6, 0.95, (D, n))
    if device:
        import torch
        y, x, z, inc, div = (torch.from_numpy(a).cuda() for a in (y, x, z, inc, div))
    # proj_mode 0; 1 and 3 with one array for every date (stride 0) and with one per date (stride n)
    for kw, per_date, nproj in (({}, False, 0), ({'inc': inc[0]}, False, 1), ({'inc': inc}, True, D), ({'divisor': div[1]}, False, 1), ({'divisor': div}, True, D)):
        w, h = R.interp_project_epochs(cubes, y, x, z, **kw)
        assert ctx.point_upload_bytes() == (0 if device else (24 + 8 * nproj) * n), kw.keys()
        assert 0.8 < np.isfinite(_host(w[0])).mean() < 1.0
        for e, cb in enumerate(cubes):
            w1, h1 = cb.interp_project(y, x, z, **{k: (v[e] if per_date else v) for k, v in kw.items()})
            assert _same(w[e], w1) and _same(h[e], h1), (kw.keys(), e)
