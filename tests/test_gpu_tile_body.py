"""GPU: the tile bodies of the two ray passes (raider_kernels.h: RayKernArgs / ray_args, TileRecords).

The light kernels read their uniform parameters per tile from the kernarg segment and pass 1 addresses a tile's records through a scalar
base (workspace + local tile * 256 * 8, stepped by nslots * 8 per field) plus the thread's constant 32-bit offset.  Pinned here are the
ways that addressing and the per-tile reloading can go wrong:

  a. a 37 x 53 grid scene - 3 x 4 tiles, padded in both directions - as one slice at 0 m and as a three-slice batch whose slices have
     different level counts, against the C oracle: nParts, the NaN mask, <= 1e-9 m;
  b. the same scene on a fresh Context whose workspace holds two tiles' worth of records (RAIDER_HIP_WORKSPACE_BYTES): several chunks with
     tile_begin != 0, bit for bit the unchunked result;
  c. list origins (1000 points: no multiple of 256; origin mode LLH) against the C oracle, same bounds;
  d. pass 1 once (ray_prepass), then the record-reusing march (ray_march) twice: the same bits both times, and raytrace's.

Scene: a 40 x 44 x 24 cube, rays well inside it (every delay finite) with incidence 20 .. 40 degrees; the references are computed once."""
import numpy as np
import pytest

from oracle import raider_oracle as O
from oracle import oracle_c as OC

pytestmark = pytest.mark.gpu

TOL = 1e-9                      # metres
NY, NX = 37, 53
HD = -167.9
HEIGHTS = (0.0, 300.0, 5000.0)  # three level counts
WS_NFIELDS, BLOCK = 29, 256     # raider_kernels.h


@pytest.fixture(scope='module')
def R():
    import raider_amd
    return raider_amd


_S = {}


def _scene():
    if not _S:
        c = O.synthetic_cube(40, 44, 24, seed=26)
        xs, ys = np.asarray(c['xs']), np.asarray(c['ys'])
        # the middle 40 % of the cube in both directions: a ray at 40 degrees reaches the top some 0.3 degrees away, inside the cube
        fx = lambda f: xs.min() + f * (xs.max() - xs.min())
        fy = lambda f: ys.min() + f * (ys.max() - ys.min())
        xp, yp = np.linspace(fx(0.3), fx(0.7), NX), np.linspace(fy(0.7), fy(0.3), NY)
        xx, yy = np.meshgrid(xp, yp)
        inc = np.broadcast_to(20.0 + 20.0 * np.arange(NX) / (NX - 1), (NY, NX)).copy()
        los = np.ascontiguousarray(O.look_vectors_from_inc_hd(inc, np.full((NY, NX), HD), yy, xx, 0.0))
        zref = float(np.asarray(c['zs'])[-1] - 1.0)
        _S.update(c=c, xp=xp, yp=yp, xx=xx, yy=yy, los=los, zref=zref, ref={})
    return _S


def _ref(ht):
    s = _scene()
    if ht not in s['ref']:
        s['ref'][ht] = OC.build_cube_ray_slice(s['c'], s['xp'], s['yp'], ht, s['los'], s['zref'])
    return s['ref'][ht]


def _gpu(R, ctx=None):
    c = _scene()['c']
    return R.Cube(c['ys'], c['xs'], c['zs'], np.asarray(c['wet'], dtype=np.float32), np.asarray(c['hydro'], dtype=np.float32), order='zyx', ctx=ctx)


def _rays(R):
    s = _scene()
    return R.Rays.grid(s['xp'], s['yp'], los=s['los'])


def _against(what, w, h, npn, ref):
    ow, oh, onp = ref
    assert np.array_equal(np.asarray(npn), onp), (what, npn, onp)
    w, h = np.asarray(w).reshape(ow.shape), np.asarray(h).reshape(oh.shape)
    assert np.array_equal(np.isnan(w), np.isnan(ow)) and np.array_equal(np.isnan(h), np.isnan(oh)), (what, 'NaN mask')
    dw, dh = np.nanmax(np.abs(w - ow)), np.nanmax(np.abs(h - oh))
    print(f'TILEBODY {what}: wet {dw:.2e} hydro {dh:.2e} finite {np.isfinite(oh).mean():.2f}')
    assert dw <= TOL and dh <= TOL, (what, dw, dh)


def test_padded_tiles_one_slice_and_a_batch_against_the_oracle(R):
    s = _scene()
    cube = _gpu(R)
    w, h, npn, fl = cube.raytrace(_rays(R), HEIGHTS[0], s['zref'])
    assert np.isfinite(_ref(HEIGHTS[0])[1]).all()
    _against('one slice', w, h, npn, _ref(HEIGHTS[0]))
    ws, hs, K, nparts, flags = cube.raytrace_slices(_rays(R), np.array(HEIGHTS), s['zref'])
    assert len(set(int(k) for k in K)) == len(HEIGHTS), K
    for i, ht in enumerate(HEIGHTS):
        _against(f'slice {i} of the batch', ws[i], hs[i], nparts[i, :K[i]], _ref(ht))
    assert np.array_equal(ws[0], w, equal_nan=True) and np.array_equal(hs[0], h, equal_nan=True)


def test_chunks_of_two_tiles_are_the_unchunked_result(R, monkeypatch):
    from raider_amd import _lib as L
    s = _scene()
    w, h, npn, fl = _gpu(R).raytrace(_rays(R), HEIGHTS[0], s['zref'])
    ws, hs, K, nparts, flags = _gpu(R).raytrace_slices(_rays(R), np.array(HEIGHTS), s['zref'])
    # two tiles' worth of records; the side buffer takes its share of the budget, so a chunk is one tile: 12 chunks per slice
    monkeypatch.setenv('RAIDER_HIP_WORKSPACE_BYTES', str(2 * BLOCK * WS_NFIELDS * 8))
    ctx = L.Context()
    small = _gpu(R, ctx)
    w2, h2, np2, fl2 = small.raytrace(_rays(R), HEIGHTS[0], s['zref'])
    assert np.array_equal(np2, npn) and fl2 == fl
    assert np.array_equal(w2, w, equal_nan=True) and np.array_equal(h2, h, equal_nan=True)
    ws2, hs2, K2, nparts2, flags2 = small.raytrace_slices(_rays(R), np.array(HEIGHTS), s['zref'])
    assert np.array_equal(K2, K) and np.array_equal(nparts2, nparts) and np.array_equal(flags2, flags)
    assert np.array_equal(ws2, ws, equal_nan=True) and np.array_equal(hs2, hs, equal_nan=True)
    _against('chunked', w2, h2, np2, _ref(HEIGHTS[0]))


def test_list_origins_against_the_oracle(R):
    from raider_amd import _lib as L
    s = _scene()
    n = 1000
    assert n % BLOCK != 0
    lat, lon, los = s['yy'].ravel()[:n].copy(), s['xx'].ravel()[:n].copy(), s['los'].reshape(-1, 3)[:n].copy()
    cube = _gpu(R)
    rays = R.Rays.points(lat=lat, lon=lon, los=los)
    assert rays.struct.origin_mode != L.ORIGIN_GRID
    w, h, npn, fl = cube.raytrace(rays, HEIGHTS[0], s['zref'])
    ow, oh, onp = OC.build_cube_ray_per_pixel(s['c'], lat, lon, np.full(n, HEIGHTS[0]), los, s['zref'])
    kz = cube.ray_levels(HEIGHTS[0], s['zref'])[2]                  # the oracle's partition is by model interval
    assert not onp[np.setdiff1d(np.arange(onp.size), kz)].any()
    _against('list origins', w, h, npn, (ow, oh, onp[kz]))


def test_marching_twice_on_one_pass_1_gives_the_same_bits(R):
    s = _scene()
    cube = _gpu(R)
    rays = _rays(R)
    ml, fl = cube.ray_prepass(rays, HEIGHTS[1], s['zref'])
    npn = R.nparts_from_maxlen(ml, 1000.0)
    w1, h1 = cube.ray_march(rays, HEIGHTS[1], s['zref'], npn, fl)
    w1, h1 = np.array(w1, copy=True), np.array(h1, copy=True)
    w2, h2 = cube.ray_march(rays, HEIGHTS[1], s['zref'], npn, fl)
    assert np.array_equal(w1, w2, equal_nan=True) and np.array_equal(h1, h2, equal_nan=True)
    w, h, np0, f0 = cube.raytrace(_rays(R), HEIGHTS[1], s['zref'])
    assert np.array_equal(np0, npn) and f0 == fl
    assert np.array_equal(w1, w, equal_nan=True) and np.array_equal(h1, h, equal_nan=True)
    _against('marched twice', w2, h2, npn, _ref(HEIGHTS[1]))
