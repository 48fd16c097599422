"""GPU: a time series of weather epochs through ONE ray batch with per-ray origin heights (rdr_raytrace_epochs,
raider_amd.raytrace_epochs) - a SAR scene on a DEM traced for every date.  Pass 1 runs once, pass 2 marches up to four epochs together
(the per-ray-height loop of march_epochs_kernel); pinned as
  * bit for bit what Cube.raytrace gives per epoch: every group pattern (D = 1 .. 6), f32 and f64 cubes, every input form, conic and
    polar-stereographic cubes, generic rays, the chunked workspace schedule, device arrays;
  * the oracle's per-pixel restatement (oracle_c.build_cube_ray_per_pixel) to 1e-9 m with the same partition.
Scene: 21 x 27 rays (three 256-lane tiles, the last one padded) on 40 x 44 x 24 cubes; the heights vary inside every wave over several
model intervals and include one below the cube's lowest level and one exactly on a level."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import raider_oracle as O
from oracle import oracle_c as OC

TIGHT = 1e-9          # metres: tests/test_gpu_perpixel.py's tolerance against the oracle
NY, NX = 21, 27
DMAX = 6


@pytest.fixture(scope='module')
def R():
    import raider_amd
    return raider_amd


def _fields(D, ny=40, nx=44, nz=24, seed0=10, **kw):
    """D epochs on one grid with distinct fields: seeds and a per-epoch scale (float32, as the cubes hold them)"""
    out = []
    for e in range(D):
        c = O.synthetic_cube(ny, nx, nz, seed=seed0 + e, **kw)
        s = 1.0 + 0.03 * e
        out.append(dict(c, wet=(c['wet'] * s).astype(np.float32), hydro=(c['hydro'] * s).astype(np.float32)))
    return out


def _cubes(R, cs, dtype=np.float32, proj=None):
    cubes = [R.Cube(c['ys'], c['xs'], c['zs'], c['wet'].astype(dtype), c['hydro'].astype(dtype), order='zyx') for c in cs]
    if proj is not None:
        for cb in cubes:
            proj(cb)
    return cubes


def _heights(ny, nx, lo, hi, zs=None, seed=5):
    """a ramp along the columns (a 16-column tile row crosses several model intervals) plus a seeded ripple, clipped to [lo, hi]"""
    rng = np.random.default_rng(seed)
    h = lo + (hi - lo) * (np.arange(nx) / (nx - 1.0))[None, :] + 0.05 * (hi - lo) * rng.uniform(-1.0, 1.0, (ny, nx))
    h = np.clip(h, lo, hi)
    if zs is not None:
        h[0, 0] = zs[0] - 50.0          # below the cube's lowest level
        h[3, 5] = zs[3]                 # exactly on a level
        h[4, 6] = zs[2] + 0.4           # the 1 m rule: less than a metre above a level ...
        h[5, 7] = zs[4] - 0.4           # ... and below one
    return h


@pytest.fixture(scope='module')
def scene():
    cs = _fields(DMAX)
    xp = np.linspace(-119.0, -115.5, NX); yp = np.linspace(34.6, 31.4, NY)
    xx, yy = np.meshgrid(xp, yp)
    inc = 30.0 + 16.0 * (np.arange(NX) / NX)[None, :] + 0.0 * yy
    hts = _heights(NY, NX, -60.0, 3000.0, cs[0]['zs'])
    los = np.ascontiguousarray(O.look_vectors_from_inc_hd(inc, np.full(yy.shape, -167.9), yy, xx, hts))
    return dict(cs=cs, xp=xp, yp=yp, xx=xx, yy=yy, inc=inc, hts=hts, los=los, zref=float(cs[0]['zs'].max() - 1))


@pytest.fixture(scope='module')
def cubes32(R, scene):
    return _cubes(R, scene['cs'])


@pytest.fixture(scope='module')
def cubes64(R, scene):
    return _cubes(R, scene['cs'], np.float64)


def _rays(R, s, form, hts='own'):
    h = s['hts'] if isinstance(hts, str) else hts
    kw = {} if h is None else dict(hts=h)
    kwp = {} if h is None else dict(hts=h.ravel())
    if form == 'grid_los':
        return R.Rays.grid(s['xp'], s['yp'], los=s['los'], **kw)
    if form == 'grid_rasters':
        return R.Rays.grid(s['xp'], s['yp'], inc=s['inc'], hd=np.full(s['inc'].shape, -167.9), **kw)
    if form == 'grid_scalars':
        return R.Rays.grid(s['xp'], s['yp'], inc=39.0, hd=-167.9, **kw)
    if form == 'llh':
        return R.Rays.points(lat=s['yy'].ravel(), lon=s['xx'].ravel(), los=s['los'].reshape(-1, 3), **kwp)
    if form == 'xyz':
        xyz = np.stack(O.lla2ecef(s['yy'].ravel(), s['xx'].ravel(), s['hts'].ravel() if h is None else h.ravel()), -1)
        return R.Rays.points(xyz=xyz, los=s['los'].reshape(-1, 3), **kwp)
    raise KeyError(form)


def _eq(a, b):
    """the same bits, NaN (the ray below the cube) in the same places"""
    return np.array_equal(a, b, equal_nan=True)


def _same_as_single(R, cubes, rays, ht, zref, Ds=range(1, DMAX + 1)):
    """raytrace_epochs(cubes[:D]) == cubes[e].raytrace, bit for bit, for every D; returns the single-cube results"""
    single = [cb.raytrace(rays, ht, zref) for cb in cubes[:max(Ds)]]
    for D in Ds:
        w, h, npp, fl = R.raytrace_epochs(cubes[:D], rays, ht, zref)
        assert w.shape == (D,) + tuple(rays.shape) and h.shape == w.shape
        for e in range(D):
            sw, sh, snp, sfl = single[e]
            assert np.array_equal(w[e], sw, equal_nan=True) and np.array_equal(h[e], sh, equal_nan=True), (D, e)
            assert np.array_equal(npp, snp) and fl == sfl, (D, e)
    return single


@pytest.mark.parametrize('form', ['grid_los', 'grid_rasters', 'grid_scalars', 'llh', 'xyz'])
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_every_epoch_is_the_single_cube_call_bit_for_bit(R, scene, cubes32, cubes64, dtype, form):
    """D = 1 .. 6: the group patterns 1, 2, 2+1, 4, 4+1, 4+2 (f64 cubes: pairs)"""
    cubes = cubes32 if dtype == 'f32' else cubes64
    single = _same_as_single(R, cubes, _rays(R, scene, form), None, scene['zref'])
    nan = np.isnan(single[0][1])                                           # (the one ray that starts below the cube)
    assert nan.sum() == 1 and nan.ravel()[0] and not np.array_equal(single[0][0], single[1][0])


def test_equal_heights_are_the_sliced_series_bit_for_bit(R, scene, cubes32, cubes64):
    for cubes in (cubes32, cubes64):
        for ht in (0.0, 437.5, float(scene['cs'][0]['zs'][3])):
            los = np.ascontiguousarray(O.look_vectors_from_inc_hd(scene['inc'], np.full(scene['yy'].shape, -167.9), scene['yy'], scene['xx'], ht))
            plain = R.Rays.grid(scene['xp'], scene['yp'], los=los)
            w, h, npp, fl = R.raytrace_epochs(cubes, R.Rays.grid(scene['xp'], scene['yp'], los=los, hts=np.full((NY, NX), ht)), None, scene['zref'])
            sw, sh, sK, snp, sfl = R.raytrace_slices_epochs(cubes, plain, [ht], scene['zref'])
            assert np.array_equal(w, sw[:, 0]) and np.array_equal(h, sh[:, 0]) and np.isfinite(h).all()
            assert np.array_equal(npp, snp[0, :sK[0]]) and (sfl[:, 0] == fl).all()


def test_a_batch_without_heights_is_the_single_cube_call(R, scene, cubes32, cubes64):
    for cubes in (cubes32, cubes64):
        for form in ('grid_los', 'llh'):
            _same_as_single(R, cubes, _rays(R, scene, form, hts=None), 250.0, scene['zref'], Ds=(1, 2, 3, 6))
    with pytest.raises(ValueError, match='slice height'):
        R.raytrace_epochs(cubes32[:2], _rays(R, scene, 'grid_los', hts=None), None, scene['zref'])


def test_conic_and_polar_cubes_and_generic_rays(R):
    # HRRR-like Lambert cube over the US south-west
    cs = _fields(DMAX, 50, 60, 20, y0=-9.0e5, y1=1.0e5, x0=-2.2e6, x1=-1.3e6)
    cubes = _cubes(R, cs, proj=lambda cb: cb.set_projection_lcc(38.5, 38.5, 38.5, 262.5))
    zref = float(cs[0]['zs'].max() - 1)
    xp = np.linspace(-117.5, -114.0, 21); yp = np.linspace(36.0, 33.5, 17)
    xx, yy = np.meshgrid(xp, yp)
    hts = _heights(17, 21, 0.0, 2800.0, cs[0]['zs'])
    single = _same_as_single(R, cubes, R.Rays.grid(xp, yp, inc=38.0, hd=-167.9, hts=hts), None, zref)
    assert np.isfinite(single[0][1]).mean() > 0.9
    _same_as_single(R, cubes, R.Rays.points(lat=yy.ravel(), lon=xx.ravel(), inc=30.0 + 0.4 * np.arange(xx.size) / xx.size, hd=-167.9, hts=hts.ravel()),
                    None, zref, Ds=(2, 5))
    # HRRR-AK-like polar-stereographic cube
    par = dict(lat_0=90.0, lat_ts=60.0, lon_0=225.0, a=6371229.0, es=0.0)
    cx, cy = O.stere_forward(61.0, -150.0, **par)
    cs = _fields(DMAX, 50, 50, 20, seed0=20, ztop=26000.0)
    for c in cs:
        c['xs'] = cx + 6000.0 * (np.arange(50) - 25); c['ys'] = cy + 6000.0 * (np.arange(50) - 25)
    cubes = _cubes(R, cs, proj=lambda cb: cb.set_projection_stere(**par))
    zref = float(cs[0]['zs'].max() - 1)
    xp = np.linspace(-150.8, -149.2, 15); yp = np.linspace(61.4, 60.6, 13)
    hts = _heights(13, 15, 0.0, 2500.0, cs[0]['zs'])
    single = _same_as_single(R, cubes, R.Rays.grid(xp, yp, inc=38.0, hd=-167.9, hts=hts), None, zref)
    assert np.isfinite(single[0][1]).mean() > 0.9
    # a scene at the pole: pass 1 classifies rays generic, the generic kernel marches them epoch by epoch on the shared records
    cs = _fields(DMAX, 12, 40, 6, seed0=30, ztop=15000.0, y0=86.0, y1=89.9, x0=-60.0, x1=60.0)
    zref = float(cs[0]['zs'].max() - 1)
    xp = np.linspace(-20.0, 20.0, 9); yp = np.linspace(88.9, 88.0, 7)
    hts = _heights(7, 9, 8800.0, 10800.0)
    for dtype in (np.float32, np.float64):
        cubes = _cubes(R, cs, dtype)
        rays = R.Rays.grid(xp, yp, inc=30.0, hd=-167.9, hts=hts)
        single = _same_as_single(R, cubes, rays, None, zref)
        assert cubes[0].ctx.generic_ray_count() > 0
        assert np.isfinite(single[0][1]).mean() > 0.5


def test_nan_block_stays_in_its_epoch(R, scene, cubes32):
    c = scene['cs'][2]
    wet = c['wet'].copy(); hyd = c['hydro'].copy()
    wet[:, 18:22, 16:22] = np.nan; hyd[:, 18:22, 16:22] = np.nan
    cubes = list(cubes32[:5])
    cubes[2] = R.Cube(c['ys'], c['xs'], c['zs'], wet, hyd, order='zyx')
    hts = scene['hts'].copy(); hts[0, 0] = -60.0                           # (every ray starts inside the cube: NaN comes from the block alone)
    rays = _rays(R, scene, 'grid_los', hts=hts)
    w, h, npp, fl = R.raytrace_epochs(cubes, rays, None, scene['zref'])
    sw, sh, snp, sfl = cubes[2].raytrace(rays, None, scene['zref'])
    assert 0 < np.isnan(sw).sum() < sw.size
    assert np.array_equal(np.isnan(w[2]), np.isnan(sw)) and np.array_equal(w[2], sw, equal_nan=True) and np.array_equal(h[2], sh, equal_nan=True)
    w0, h0, _, _ = R.raytrace_epochs(cubes32[:5], rays, None, scene['zref'])
    for e in (0, 1, 3, 4):
        assert np.isfinite(w[e]).all() and np.isfinite(h[e]).all()
        assert np.array_equal(w[e], w0[e]) and np.array_equal(h[e], h0[e])


def test_every_epoch_against_the_c_oracle(R, scene, cubes32):
    rays = _rays(R, scene, 'llh')
    w, h, npp, fl = R.raytrace_epochs(cubes32, rays, None, scene['zref'])
    kz = cubes32[0].ray_levels(rays.ht_min, scene['zref'])[2]
    for e, c in enumerate(scene['cs']):
        ow, oh, onp = OC.build_cube_ray_per_pixel(c, scene['yy'], scene['xx'], scene['hts'], scene['los'], scene['zref'])
        assert np.isfinite(ow).mean() >= 0.9 and np.isfinite(oh).mean() >= 0.9
        assert np.array_equal(npp, onp[kz]), (e, npp, onp[kz])
        assert not onp[np.setdiff1d(np.arange(onp.size), kz)].any()
        assert np.array_equal(np.isnan(w[e]), np.isnan(ow.ravel()))
        assert np.isfinite(w[e]).mean() >= 0.9
        np.testing.assert_allclose(w[e], ow.ravel(), rtol=0, atol=TIGHT, equal_nan=True)
        np.testing.assert_allclose(h[e], oh.ravel(), rtol=0, atol=TIGHT, equal_nan=True)


def test_chunked_workspace_schedule_gives_the_same_bits(R, scene, cubes32, cubes64):
    """The workspace limit has a floor of 1 MiB = 17 tiles of ray records, so this case alone uses a larger scene: 95 x 90 rays = 36
    tiles, three chunks (reduction-only pass 1, then three pass-1 / pass-2 pairs)."""
    ny, nx = 95, 90
    xp = np.linspace(-119.0, -115.5, nx); yp = np.linspace(34.6, 31.4, ny)
    hts = _heights(ny, nx, -60.0, 3000.0, scene['cs'][0]['zs'])
    inc = 30.0 + 16.0 * (np.arange(nx) / nx)[None, :] + np.zeros((ny, nx))
    rays = R.Rays.grid(xp, yp, inc=inc, hd=-167.9, hts=hts)
    ctx = R.Context.default()
    for cubes in (cubes32[:5], cubes64[:3]):
        w, h, npp, fl = R.raytrace_epochs(cubes, rays, None, scene['zref'])
        ctx.set_workspace_limit(1 << 20)
        try:
            ctx.set_profiling(True)
            w2, h2, np2, fl2 = R.raytrace_epochs(cubes, rays, None, scene['zref'])
            prepasses = ctx.profile_get(0)[0]
        finally:
            ctx.set_profiling(False)
            ctx.set_workspace_limit(48 << 30)
        assert prepasses >= 4                     # (the reduction + at least three chunks)
        assert _eq(w2, w) and _eq(h2, h) and _eq(np2, npp) and fl2 == fl
        sw, sh, snp, sfl = cubes[-1].raytrace(rays, None, scene['zref'])
        assert _eq(w[-1], sw) and _eq(h[-1], sh) and _eq(npp, snp)


def test_device_arrays_asynchronous_and_out_buffers(R, scene, cubes32, cubes64):
    import torch
    dev = torch.device('cuda:0')
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rays_d = R.Rays.grid(t(scene['xp']), t(scene['yp']), los=t(scene['los']), hts=t(scene['hts']))
    rays = _rays(R, scene, 'grid_los')
    for cubes in (cubes32[:4], cubes64[:3]):
        D = len(cubes)
        w, h, npp, fl = R.raytrace_epochs(cubes, rays, None, scene['zref'])
        ow = torch.full((D, NY, NX), -1.0, dtype=torch.float64, device=dev); oh = torch.full_like(ow, -1.0)
        wd, hd, npd, fld = R.raytrace_epochs(cubes, rays_d, None, scene['zref'], out=(ow, oh), want_nparts=False)
        torch.cuda.synchronize()
        assert wd is ow and hd is oh and npd is None and fld is None
        assert _eq(ow.cpu().numpy(), w) and _eq(oh.cpu().numpy(), h)
        wd2, hd2, np2, fl2 = R.raytrace_epochs(cubes, rays_d, None, scene['zref'])
        assert _eq(wd2.cpu().numpy(), w) and _eq(hd2.cpu().numpy(), h) and _eq(np2, npp) and fl2 == fl
    # host out= buffers are honoured too
    bw = np.full((2, NY, NX), -1.0); bh = np.full((2, NY, NX), -1.0)
    rw, rh, _, _ = R.raytrace_epochs(cubes32[:2], rays, None, scene['zref'], out=(bw, bh))
    assert rw is bw and rh is bh and _eq(bw[1], cubes32[1].raytrace(rays, None, scene['zref'])[0])


def test_pass_one_runs_once(R, scene, cubes32):
    rays = _rays(R, scene, 'grid_los')
    ctx = cubes32[0].ctx
    try:
        ctx.set_profiling(True)
        cubes32[0].raytrace(rays, None, scene['zref'])
        one = ctx.profile_get(0)[0]
        ctx.set_profiling(True)                                            # (restarts the counts)
        R.raytrace_epochs(cubes32[:4], rays, None, scene['zref'])
        four = ctx.profile_get(0)[0]
        marches = ctx.profile_get(1)[0]
    finally:
        ctx.set_profiling(False)
    assert one >= 1 and four == one and marches == 1                       # one stacked launch of four epochs


def test_refusals(R, scene, cubes32):
    rays = _rays(R, scene, 'grid_los')
    zref = scene['zref']
    c = scene['cs'][2]
    odd = O.synthetic_cube(40, 44, 23, seed=1)
    bad = {
        'shape': R.Cube(odd['ys'], odd['xs'], odd['zs'], odd['wet'], odd['hydro'], order='zyx'),
        'dtype': R.Cube(c['ys'], c['xs'], c['zs'], c['wet'].astype(np.float64), c['hydro'].astype(np.float64), order='zyx'),
        'z axis': R.Cube(c['ys'], c['xs'], c['zs'] + 1.0, c['wet'], c['hydro'], order='zyx'),
        'projection': R.Cube(c['ys'], c['xs'], c['zs'], c['wet'], c['hydro'], order='zyx').set_projection_lcc(38.5, 38.5, 38.5, 262.5),
    }
    for what, cb in bad.items():
        with pytest.raises(ValueError, match='rdr_raytrace_epochs: epoch 2'):
            R.raytrace_epochs([cubes32[0], cubes32[1], cb], rays, None, zref)
    with pytest.raises(ValueError, match='above the lowest'):
        R.raytrace_epochs(cubes32[:2], rays, float(scene['hts'].min()) + 1.0, zref)
    with pytest.raises(ValueError, match='at least one epoch'):
        R.raytrace_epochs([], rays, None, zref)
    los2 = np.ascontiguousarray(np.stack([scene['los'], scene['los']]))
    with pytest.raises(ValueError, match='height slices'):
        R.raytrace_epochs(cubes32[:2], R.Rays.grid(scene['xp'], scene['yp'], los=los2, slices=2), 0.0, zref)
    with pytest.raises(ValueError, match='output arrays must hold'):
        R.raytrace_epochs(cubes32[:2], rays, None, zref, out=(np.empty((3, NY, NX)), np.empty((3, NY, NX))))
    with pytest.raises(ValueError, match='per-ray heights'):
        R.raytrace_slices_epochs(cubes32[:2], rays, [0.0], zref)
    # the C contract (ht <= min(hts)) violated behind the wrapper's back: refused as rdr_raytrace refuses it
    low = _rays(R, scene, 'grid_los')
    low.ht_min = 900.0
    with pytest.raises(ValueError, match='per-ray heights'):
        R.raytrace_epochs(cubes32[:2], low, None, zref)


def test_stacked_kernels_are_loaded_without_scratch(R, cubes32, cubes64):
    """the resource report of DESIGN "Time series" / 5d, read from the loaded code object: no scratch at the chosen occupancy, in the
    sliced stacked kernels (4, 5) and the per-ray-height ones (6, 7)"""
    for cubes in (cubes32, cubes64):
        for which in (4, 5, 6, 7):
            a = cubes[0].ray_kernel_attributes(which)
            assert a['scratch'] == 0 and a['vgpr'] > 0, (which, a)
